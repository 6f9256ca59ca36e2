// almpc_c2d.hip.h -- k_c2d: batched exact zero-order-hold discretisation of continuous-time models,
//   [Ad Bd; 0 I] = exp([Ac Bc; 0 0] Ts),
// one model (Ac_i, Bc_i) per instance and one sample time: what stands in front of the reference's continuous-time design
// (src/sub/design_mpc.jl:22-41 discretises and recurses into the discrete method), per instance and on the device.
//
// The algorithm is hm::c2d's (csrc/almpc_host_math.h), statement by statement: nrm = Ts |Ac|_1, s halvings until nrm <= 0.5 (found by
// repeated halving, so host and device take the same decision), h = Ts / 2^s, X = h Ac, G = sum_{k <= 16} X^k / (k+1)! by Horner,
// Bd = h G Bc, Ad = I + X G, then s doublings Bd <- Bd + Ad Bd, Ad <- Ad Ad.  No augmented matrix, no linear solve: a singular Ac is
// no special case.  Status 1 and nothing written: nrm not finite, s > 60, or an output entry that is not finite.
//
// Shape: k_dare's.  One wave per instance, C2D_WAVES waves per workgroup while their matrices fit LDS, no workgroup barrier (waves
// never wait for each other).  A wave keeps three n x n and three n x m matrices, leading dimension n | 1 (a read along a row is free
// of bank conflicts):
//   X | G | T   and   Bc | Bd | TB           ping-ponged: the Horner steps swap G and T, the doublings (Ad, X) and (Bd, TB)
// Lane l owns row l & (RL - 1) (RL = 16, 32, 64: the first power of two >= n) and every (64 / RL)-th column.  The inputs are in LDS
// before the first output is written, so Ad, Bd may be the input slots themselves (in place).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace almpc {

struct C2dParams {
    int n, m, batch;
    const double* Ac; long A_stride;   // n x n column-major per instance
    const double* Bc; long B_stride;   // n x m
    double Ts;
    double* Ad; double* Bd;            // same strides; may alias Ac, Bc.  Written only for an instance with status 0 ...
    int poison;                        // ... or, when set, with NaN for one that failed (re-linearisation pipeline: no model left behind)
    int32_t* status;                   // [batch] 0, or 1 (see above)
    int lds_per_wave;                  // doubles
};

constexpr int C2D_WAVES = 4;
constexpr int C2D_MAX_N = 64, C2D_MAX_M = 16;
constexpr int C2D_K = 16, C2D_MAX_S = 60;   // hm::C2D_TERMS, hm::C2D_MAX_HALVINGS

__host__ __device__ inline int c2d_ld(int n) { return n | 1; }
__host__ __device__ inline int c2d_lds_doubles(int n, int m) { return (3 * c2d_ld(n) * (n + m) + 1) & ~1; }
// waves per workgroup: as many as fit 160 KB, at most C2D_WAVES
__host__ __device__ inline int c2d_waves(int n, int m) {
    int w = C2D_WAVES;
    while (w > 1 && (size_t)c2d_lds_doubles(n, m) * sizeof(double) * w > 160 * 1024) --w;
    return w;
}

__device__ __forceinline__ void c2d_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ bool c2d_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// out(n x c) = shift I + scale (X * Y) [+ base], by one wave; every matrix with leading dimension ld.  Sums ascend in k from zero
// (hm::mul); what is added to them is added last.
template <int RL>
__device__ __forceinline__ void c2d_mul(double* out, const double* X, const double* Y, const double* base, double shift, double scale,
                                        int n, int c, int ld, int lane) {
    constexpr int CG = 64 / RL;
    const int i = lane & (RL - 1), cg = lane / RL;
    if (i >= n) return;
    for (int j = cg; j < c; j += CG) {
        double acc = 0.0;
        for (int l = 0; l < n; ++l) acc += X[i + l * ld] * Y[l + j * ld];
        acc = scale * acc;
        if (base) acc += base[i + j * ld];
        out[i + j * ld] = (i == j ? shift : 0.0) + acc;
    }
}

template <int RL>
__global__ __launch_bounds__(64 * C2D_WAVES) void k_c2d(C2dParams p) {
    extern __shared__ __attribute__((aligned(16))) double c2d_smem[];
    constexpr int CG = 64 / RL;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int n = p.n, m = p.m, ld = c2d_ld(n);
    const int row = lane & (RL - 1), cg = lane / RL;
    double* L = c2d_smem + (size_t)wv * p.lds_per_wave;
    const int wpb = (int)(blockDim.x >> 6), nwaves = gridDim.x * wpb;
    for (int inst = blockIdx.x * wpb + wv; inst < p.batch; inst += nwaves) {
        double* X = L;            double* G = X + ld * n;    double* T = G + ld * n;
        double* Bc = T + ld * n;  double* Bd = Bc + ld * m;  double* TB = Bd + ld * m;
        const double* Ag = p.Ac + (size_t)inst * p.A_stride;
        const double* Bg = p.Bc + (size_t)inst * p.B_stride;
        // nrm = Ts max_j sum_i |Ac[i,j]|: lane j sums column j (n <= 64)
        double cs = 0.0;
        if (lane < n)
            for (int i = 0; i < n; ++i) cs += fabs(Ag[i + lane * n]);
        cs *= p.Ts;
        int st = __any(c2d_finite(cs) ? 0 : 1) ? 1 : 0;
        double nrm = cs;   // (fmax drops a NaN, as in hm::c2d: finiteness is tested apart)
        for (int o = 32; o > 0; o >>= 1) nrm = fmax(nrm, __shfl_xor(nrm, o));
        nrm = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(nrm)), __builtin_amdgcn_readfirstlane(__double2loint(nrm)));
        int s = 0;
        double h = p.Ts;
        while (!st && nrm > 0.5) {
            if (++s > C2D_MAX_S) { st = 1; break; }
            nrm *= 0.5; h *= 0.5;
        }
        c2d_fence();   // (the previous instance of this wave has read its last LDS operand)
        if (!st) {
            if (row < n) {
                for (int j = cg; j < n; j += CG) { X[row + j * ld] = h * Ag[row + j * n]; G[row + j * ld] = row == j ? 1.0 : 0.0; }
                for (int a = cg; a < m; a += CG) Bc[row + a * ld] = Bg[row + a * n];
            }
            c2d_fence();
            for (int k = C2D_K; k >= 1; --k) {   // G <- I + X G / (k + 1)
                c2d_mul<RL>(T, X, G, nullptr, 1.0, 1.0 / (double)(k + 1), n, n, ld, lane);
                c2d_fence();
                double* t_ = G; G = T; T = t_;
            }
            c2d_mul<RL>(Bd, G, Bc, nullptr, 0.0, h, n, m, ld, lane);    // Bd = h G Bc
            c2d_mul<RL>(T, X, G, nullptr, 1.0, 1.0, n, n, ld, lane);    // Ad = I + X G
            c2d_fence();
            double* Ad = T; double* A2 = X;   // (X and G are free from here on)
            for (int d = 0; d < s; ++d) {
                c2d_mul<RL>(TB, Ad, Bd, Bd, 0.0, 1.0, n, m, ld, lane);      // Bd + Ad Bd
                c2d_mul<RL>(A2, Ad, Ad, nullptr, 0.0, 1.0, n, n, ld, lane); // Ad Ad
                c2d_fence();
                double* t_ = Ad; Ad = A2; A2 = t_;
                t_ = Bd; Bd = TB; TB = t_;
            }
            bool notfin = false;
            if (row < n) {
                for (int j = cg; j < n; j += CG) notfin = notfin || !c2d_finite(Ad[row + j * ld]);
                for (int a = cg; a < m; a += CG) notfin = notfin || !c2d_finite(Bd[row + a * ld]);
            }
            if (__any(notfin ? 1 : 0)) st = 1;
            X = Ad;   // (what is written below)
        }
        double* Adg = p.Ad + (size_t)inst * p.A_stride;
        double* Bdg = p.Bd + (size_t)inst * p.B_stride;
        if (!st) {
            if (row < n) {
                for (int j = cg; j < n; j += CG) Adg[row + j * n] = X[row + j * ld];
                for (int a = cg; a < m; a += CG) Bdg[row + a * n] = Bd[row + a * ld];
            }
        } else if (p.poison) {
            const double qnan = __longlong_as_double(0x7ff8000000000000LL);
            if (row < n) {
                for (int j = cg; j < n; j += CG) Adg[row + j * n] = qnan;
                for (int a = cg; a < m; a += CG) Bdg[row + a * n] = qnan;
            }
        }
        if (lane == 0) p.status[inst] = st;
    }
}

}  // namespace almpc
