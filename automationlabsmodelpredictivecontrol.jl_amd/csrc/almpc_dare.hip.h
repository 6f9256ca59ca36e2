// almpc_dare.hip.h -- k_dare: batched stabilising solution of the discrete algebraic Riccati equation
//   A'PA - P - A'PB (R + B'PB)^-1 B'PA + Q = 0
// for one model (A_i, B_i) per instance and shared weights: the terminal weight the reference takes from
// are(Discrete, A, B, Q, R) (src/sub/design_mpc.jl:312-327), per instance and on the device.
//
// The algorithm is hm::dare's (csrc/almpc_host_math.h), statement by statement: the structure-preserving doubling algorithm from
// G0 = B R^-1 B', H0 = Q, A0 = A; every doubling forms W = I + G H, solves W X = [A | G] by LU with partial pivoting (hm::lu_solve:
// W is not symmetric), then A <- A W^-1 A, G <- G + A W^-1 G A', H <- H + A'H W^-1 A, G and H symmetrised; it stops at
// max|dH| <= 1e-13 max(1, max|H|) within 200 doublings and accepts P = H only if every entry is finite and the residual of the equation
// itself is at most 1e-7 max(1, max|P|, max|Q|).
//
// Shape: one wave per instance, DARE_WAVES waves per workgroup while their matrices fit LDS (k_sgains' pattern).  A wave keeps six
// d x d matrices (d = max(n, m), leading dimension d | 1 so that a read along a row is free of bank conflicts) and one m x m block:
//   Ak | Gk | Hk | W | XA | XG | Sm            XA, XG adjacent: the right-hand side [A | G] of the solve is one n x 2n matrix
// Lane l owns row l & (RL - 1) of every matrix (RL = 16, 32, 64: the first power of two >= n) and every (64 / RL)-th column, so a
// product, an elimination step and a back-substitution step use no division or modulo and read LDS along columns.  The kernel is
// bound by latency, not by flops: a doubling is a chain of n pivot steps and n back-substitution steps, each a handful of dependent
// LDS round trips (DESIGN.md, section "k_dare").  Waves never wait for each other: there is no workgroup barrier in the kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace almpc {

struct DareParams {
    int n, m, batch;
    const double* A; long A_stride;    // n x n column-major per instance
    const double* B; long B_stride;    // n x m
    const double* Q; const double* R;  // n x n and m x m: shared (strides 0), or one pair per instance
    long Q_stride = 0, R_stride = 0;
    double* P; long P_stride;          // n x n per instance: written only for an instance that is accepted ...
    const double* fallback;            // ... or, when non-null, with this shared n x n matrix for one that is not
    int32_t* status;                   // [batch] 0 accepted; 1 singular pivot, 2 no fixed point / not finite, 3 residual too large
    int lds_per_wave;                  // doubles
};

constexpr int DARE_WAVES = 4;
constexpr int DARE_MAX_N = 48, DARE_MAX_M = 16;
constexpr int DARE_MAX_DOUBLINGS = 200;

__host__ __device__ inline int dare_ld(int n, int m) { return (n > m ? n : m) | 1; }
__host__ __device__ inline int dare_lds_doubles(int n, int m) {
    const int d = n > m ? n : m;
    return (6 * dare_ld(n, m) * d + m * dare_ld(n, m) + 1) & ~1;
}
// waves per workgroup: as many as fit 160 KB, at most DARE_WAVES
__host__ __device__ inline int dare_waves(int n, int m) {
    int w = DARE_WAVES;
    while (w > 1 && (size_t)dare_lds_doubles(n, m) * sizeof(double) * w > 160 * 1024) --w;
    return w;
}

__device__ __forceinline__ void dare_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ double dare_wave_max(double v) {   // (fmax drops a NaN, as hm::amax does: finiteness is tested apart)
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// out(r x c) = [base +] op(X) * Y over k, by one wave; every matrix with leading dimension ld.  TX: X is stored k x r and read
// transposed; TY: Y is stored c x k and read transposed.  Sums ascend in k from zero, the base is added last (hm::mul, then +=).
template <int RL, bool TX, bool TY>
__device__ __forceinline__ void dare_mul(double* out, const double* X, const double* Y, const double* base, int r, int k, int c, int ld,
                                         int lane) {
    constexpr int CG = 64 / RL;
    const int i = lane & (RL - 1), cg = lane / RL;
    if (i >= r) return;
    for (int j = cg; j < c; j += CG) {
        double acc = 0.0;
        for (int l = 0; l < k; ++l) acc += (TX ? X[l + i * ld] : X[i + l * ld]) * (TY ? Y[j + l * ld] : Y[l + j * ld]);
        out[i + j * ld] = base ? base[i + j * ld] + acc : acc;
    }
}

// One DPP move of an int / a double inside its row of 16 lanes (every control used below has a source lane for every lane)
template <int CTRL>
__device__ __forceinline__ int dare_dpp_i(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xF, 0xF, false); }
template <int CTRL>
__device__ __forceinline__ double dare_dpp_d(double v) {
    return __hiloint2double(dare_dpp_i<CTRL>(__double2hiint(v)), dare_dpp_i<CTRL>(__double2loint(v)));
}
// the larger magnitude, the lower row among equals
__device__ __forceinline__ void dare_pick(double& best, int& p, double v2, int p2) {
    if (v2 > best || (v2 == best && p2 < p)) { best = v2; p = p2; }
}

// Solve W X = X (W nr x nr, X nr x c, both with leading dimension ld) in place by LU with partial pivoting: hm::lu_solve, one wave.
// The pivot of a step is the largest magnitude of its column from the diagonal down, the first of equals; it is found by a wave
// reduction (DPP inside the rows of 16 lanes, v_readlane across them), and the pivot row and the column of multipliers are read back from LDS by every lane (broadcast reads).
// Returns false (the same in every lane) when a pivot is zero or not a number.
template <int RL>
__device__ __forceinline__ bool dare_lu_solve(double* W, double* X, int nr, int c, int ld, int lane) {
    constexpr int CG = 64 / RL;
    const int r = lane & (RL - 1), cg = lane / RL;
    for (int k = 0; k < nr; ++k) {
        double best = -1.0;
        int p = lane;
        if (lane >= k && lane < nr) {
            const double v = fabs(W[lane + k * ld]);
            best = v == v ? v : -1.0;
        }
        // all-reduce inside every row of 16 lanes by DPP (lane ^ 1, lane ^ 2, mirror of 8, mirror of 16), then the rows of 16 that
        // hold matrix rows (lanes 0, 16, 32, 48) by v_readlane, in order: half the time of a __shfl_xor butterfly, which was a
        // third of the kernel at n = 4
        dare_pick(best, p, dare_dpp_d<0xB1>(best), dare_dpp_i<0xB1>(p));      // quad_perm [1, 0, 3, 2]
        dare_pick(best, p, dare_dpp_d<0x4E>(best), dare_dpp_i<0x4E>(p));      // quad_perm [2, 3, 0, 1]
        dare_pick(best, p, dare_dpp_d<0x141>(best), dare_dpp_i<0x141>(p));    // row_half_mirror
        dare_pick(best, p, dare_dpp_d<0x140>(best), dare_dpp_i<0x140>(p));    // row_mirror
        {
            double bq = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(best), 0), __builtin_amdgcn_readlane(__double2loint(best), 0));
            int pq = __builtin_amdgcn_readlane(p, 0);
#pragma unroll
            for (int q = 1; q < RL / 16; ++q)
                dare_pick(bq, pq, __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(best), 16 * q), __builtin_amdgcn_readlane(__double2loint(best), 16 * q)),
                          __builtin_amdgcn_readlane(p, 16 * q));
            best = bq; p = pq;
        }
        if (!(best > 0.0)) return false;
        if (p != k) {
            for (int j = lane; j < nr + c; j += 64) {
                double* col = j < nr ? W + j * ld : X + (j - nr) * ld;
                const double a = col[k], b = col[p];
                col[k] = b; col[p] = a;
            }
        }
        dare_fence();
        if (r > k && r < nr) {
            const double f = W[r + k * ld] * (1.0 / W[k + k * ld]);
            if (f != 0.0) {
                for (int j = k + 1 + cg; j < nr; j += CG) W[r + j * ld] -= f * W[k + j * ld];
                for (int j = cg; j < c; j += CG) X[r + j * ld] -= f * X[k + j * ld];
            }
        }
        dare_fence();
    }
    for (int i = nr - 1; i >= 0; --i) {   // back-substitution, one row of X per step
        const double d = W[i + i * ld];
        for (int j = lane; j < c; j += 64) X[i + j * ld] = X[i + j * ld] / d;
        dare_fence();
        if (r < i) {
            const double u = W[r + i * ld];
            for (int j = cg; j < c; j += CG) X[r + j * ld] -= u * X[i + j * ld];
        }
        dare_fence();
    }
    return true;
}

template <int RL>
__global__ __launch_bounds__(64 * DARE_WAVES) void k_dare(DareParams p) {
    extern __shared__ __attribute__((aligned(16))) double dare_smem[];
    constexpr int CG = 64 / RL;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int n = p.n, m = p.m, d = n > m ? n : m, ld = dare_ld(n, m);
    const int row = lane & (RL - 1), cg = lane / RL;
    double* L = dare_smem + (size_t)wv * p.lds_per_wave;
    double* Ak = L;            double* Gk = Ak + ld * d;   double* Hk = Gk + ld * d;
    double* W = Hk + ld * d;   double* XA = W + ld * d;    double* XG = XA + ld * n;   // [XA | XG]: n x 2n (2 ld n <= 2 ld d)
    double* Sm = XA + 2 * ld * d;
    const int wpb = (int)(blockDim.x >> 6), nwaves = gridDim.x * wpb;
    for (int inst = blockIdx.x * wpb + wv; inst < p.batch; inst += nwaves) {
        const double* Ag = p.A + (size_t)inst * p.A_stride;
        const double* Bg = p.B + (size_t)inst * p.B_stride;
        const double* Qg = p.Q + (size_t)inst * p.Q_stride;
        const double* Rg = p.R + (size_t)inst * p.R_stride;
        int st = 0;
        dare_fence();
        // G0 = B R^-1 B': R X = B' by the same solve, then B X.  Ak = A, Hk = Q.
        if (row < n) {
            for (int j = cg; j < n; j += CG) { Ak[row + j * ld] = Ag[row + j * n]; Hk[row + j * ld] = Qg[row + j * n]; }
            for (int a = cg; a < m; a += CG) W[row + a * ld] = Bg[row + a * n];          // B (n x m) in W for now
        }
        if (row < m) {
            for (int b = cg; b < m; b += CG) Sm[row + b * ld] = Rg[row + b * m];
            for (int j = cg; j < n; j += CG) XA[row + j * ld] = Bg[j + row * n];         // B' (m x n)
        }
        dare_fence();
        if (!dare_lu_solve<RL>(Sm, XA, m, n, ld, lane)) st = 1;
        if (!st) dare_mul<RL, false, false>(Gk, W, XA, nullptr, n, m, n, ld, lane);
        dare_fence();
        bool converged = false;
        for (int it = 0; it < DARE_MAX_DOUBLINGS && !st && !converged; ++it) {
            // W = I + G H, right-hand side [A | G]
            if (row < n)
                for (int j = cg; j < n; j += CG) {
                    double acc = 0.0;
                    for (int l = 0; l < n; ++l) acc += Gk[row + l * ld] * Hk[l + j * ld];
                    W[row + j * ld] = acc + (row == j ? 1.0 : 0.0);
                    XA[row + j * ld] = Ak[row + j * ld];
                    XG[row + j * ld] = Gk[row + j * ld];
                }
            dare_fence();
            if (!dare_lu_solve<RL>(W, XA, n, 2 * n, ld, lane)) { st = 1; break; }
            dare_mul<RL, false, false>(W, Ak, XG, nullptr, n, n, n, ld, lane);         // T1 = A W^-1 G
            dare_fence();
            dare_mul<RL, false, true>(Gk, W, Ak, Gk, n, n, n, ld, lane);               // G += T1 A'
            dare_mul<RL, true, false>(XG, Ak, Hk, nullptr, n, n, n, ld, lane);         // T2 = A' H
            dare_fence();
            dare_mul<RL, false, false>(W, XG, XA, Hk, n, n, n, ld, lane);              // H1 = H + T2 W^-1 A  (not yet symmetric)
            dare_fence();
            dare_mul<RL, false, false>(XG, Ak, XA, nullptr, n, n, n, ld, lane);        // A1 = A W^-1 A
            // symmetrise G and H (each pair by one lane), max|H1 - H|, max|H1|, finiteness
            double diff = 0.0, hmax = 0.0;
            bool notfin = false;
            if (row < n)
                for (int j = cg; j < n; j += CG) {
                    if (row > j) continue;
                    const double g = row == j ? Gk[row + j * ld] : 0.5 * (Gk[row + j * ld] + Gk[j + row * ld]);
                    Gk[row + j * ld] = g; Gk[j + row * ld] = g;
                    const double h = row == j ? W[row + j * ld] : 0.5 * (W[row + j * ld] + W[j + row * ld]);
                    diff = fmax(diff, fmax(fabs(h - Hk[row + j * ld]), fabs(h - Hk[j + row * ld])));
                    hmax = fmax(hmax, fabs(h));
                    notfin = notfin || !(fabs(h) <= 1.7976931348623157e308);
                    Hk[row + j * ld] = h; Hk[j + row * ld] = h;
                }
            dare_fence();
            if (row < n)
                for (int j = cg; j < n; j += CG) Ak[row + j * ld] = XG[row + j * ld];
            dare_fence();
            if (__any(notfin ? 1 : 0)) { st = 2; break; }   // (an entry that is not finite never becomes finite again)
            diff = dare_wave_max(diff); hmax = dare_wave_max(hmax);
            converged = __builtin_amdgcn_readfirstlane(diff <= 1e-13 * fmax(1.0, hmax) ? 1 : 0) != 0;
        }
        if (!st && !converged) st = 2;
        // the residual of the equation itself, from the instance's own A and B: P = Hk
        double pmax = 0.0, qmax = 0.0;
        if (!st) {
            if (row < n) {
                for (int j = cg; j < n; j += CG) {
                    Ak[row + j * ld] = Ag[row + j * n];
                    pmax = fmax(pmax, fabs(Hk[row + j * ld]));
                    qmax = fmax(qmax, fabs(Qg[row + j * n]));
                }
                for (int a = cg; a < m; a += CG) Gk[row + a * ld] = Bg[row + a * n];     // B in Gk
            }
            dare_fence();
            dare_mul<RL, false, false>(XG, Hk, Ak, nullptr, n, n, n, ld, lane);          // PA
            dare_mul<RL, false, false>(W, Hk, Gk, nullptr, n, n, m, ld, lane);           // PB
            dare_fence();
            dare_mul<RL, true, false>(XA, Gk, XG, nullptr, m, n, n, ld, lane);           // K = B'PA  (m x n)
            if (row < m)                                                               // S = B'PB + R
                for (int b = cg; b < m; b += CG) {
                    double acc = 0.0;
                    for (int l = 0; l < n; ++l) acc += Gk[l + row * ld] * W[l + b * ld];
                    Sm[row + b * ld] = acc + Rg[row + b * m];
                }
            dare_fence();
            dare_mul<RL, true, false>(Gk, Ak, W, nullptr, n, n, m, ld, lane);            // A'PB over B (B was last read before the fence)
            if (!dare_lu_solve<RL>(Sm, XA, m, n, ld, lane)) st = 1;
        }
        if (!st) {
            double rmax = 0.0;
            bool notfin = false;
            if (row < n)
                for (int j = cg; j < n; j += CG) {
                    double acc = 0.0, corr = 0.0;
                    for (int l = 0; l < n; ++l) acc += Ak[l + row * ld] * XG[l + j * ld];
                    for (int a = 0; a < m; ++a) corr += Gk[row + a * ld] * XA[a + j * ld];
                    const double res = acc + (Qg[row + j * n] - Hk[row + j * ld] - corr);
                    rmax = fmax(rmax, fabs(res));
                    notfin = notfin || !(fabs(res) <= 1.7976931348623157e308);
                }
            rmax = dare_wave_max(rmax); pmax = dare_wave_max(pmax); qmax = dare_wave_max(qmax);
            if (__any(notfin ? 1 : 0) || !__builtin_amdgcn_readfirstlane(rmax <= 1e-7 * fmax(1.0, fmax(pmax, qmax)) ? 1 : 0)) st = 3;
        }
        double* Pg = p.P + (size_t)inst * p.P_stride;
        if (!st) {
            if (row < n)
                for (int j = cg; j < n; j += CG) Pg[row + j * n] = Hk[row + j * ld];
        } else if (p.fallback) {
            if (row < n)
                for (int j = cg; j < n; j += CG) Pg[row + j * n] = p.fallback[row + j * n];
        }
        if (lane == 0) p.status[inst] = st;
    }
}

}  // namespace almpc
