// almpc_cert.hip.h -- k_cert: cost, costates, input gradient and KKT residual of a step, from the returned trajectories and the
// design data alone (no solver internals, so one kernel serves condensed, per-instance, weighted and structured handles).
//
// Per instance, stages 0-based, e_k = e_x[:,k], v_k = e_u[:,k], u_k = u[:,k], Q, R, S, P symmetrised (0.5 (M + M')):
//   J     = e_N'P e_N + sum_k (e_k'Q e_k + [useR] v_k'R v_k) + [useS] sum_{i<N-1} d_i'S d_i,       d_i = u_i - u_{i+1}
//   lam_N = 2 P e_N,   lam_k = 2 Q e_k + A'lam_{k+1}                                               (k = N-1 .. 0)
//   g_k   = B'lam_{k+1} + [useR] 2 R v_k + [useS]([k < N-1] 2 S d_k - [k > 0] 2 S d_{k-1})          (= H v + f of the condensed QP)
//   res   = max_{k,j} |u_k - clip(u_k - g_k, umin, umax)|
// The reference's objective and branch rule: src/sub/design_mpc.jl:436-465 (the stage sum runs over columns 1..horizon of e_x, so
// the constant e_0'Q e_0 is part of J); useR and useS come from the design and are not re-tested here.
//
// Shape: one wave per instance, CERT_WAVES waves per workgroup while their slices fit LDS, a persistent capped grid; waves never wait
// for each other (no workgroup barrier).  A wave's slice holds the instance's operands, staged once per instance (a shared operand --
// stride 0 -- once per wave), and two slots of stage vectors:
//   A | B | Q | P | R | S   column-major, leading dimension ld = max(n, m) | 1: a read along a row (M x) and one along a column
//                           (M'x, lane = column) are both free of bank conflicts
//   slot[2] = lam | e | v | u | d      the costate handed down and the stage's own vectors (broadcast reads of the products)
// Lane l owns row l & (RL - 1) and column group l / RL (RL = 16, 32, 64: the first power of two >= n); a product splits its inner
// sum over the 64 / RL column groups and joins them with __shfl_xor, after which every group holds the same bits.  The stage loop
// runs backward and has no division or modulo.  Per stage the dependent chain is: read lam_{k+1} from LDS, the A' product, the
// join, one add, write lam_k to the other slot, one wave-level fence.  q_k = 2 Q e_k, r_k = 2 R v_k, the rate term and B'lam_{k+1}
// hang off that chain; the stage vectors of stage k-1 are loaded from HBM (coalesced, one element per lane) while stage k+1 computes
// and staged into the other slot under the same fence.
// The cost falls out of the vectors already formed (0.5 e_k.q_k, 0.5 v_k.r_k, 0.5 d_i.(2 S d_i), 0.5 e_N.lam_N), summed per lane
// and reduced once at the end by a butterfly; res the same way with a maximum that keeps a NaN.  An instance's results depend on
// nothing but its own data: no atomics, no order between waves.  Every instance is computed whatever its status; a trajectory that
// is not finite gives results that are not finite.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace almpc {

struct CertParams {
    int n, m, N, batch;
    int useR, useS;                          // the design's branch (one for the batch)
    const double* A; long A_stride;          // n x n column-major; stride 0: shared
    const double* B; long B_stride;          // n x m
    const double* Q; long Q_stride;          // n x n
    const double* R; long R_stride;          // m x m (read only with useR)
    const double* S; long S_stride;          // m x m (read only with useS)
    const double* P; long P_stride;          // n x n
    const double* umin; const double* umax;  // [m]
    const double* ex;                        // [batch][N+1][n]
    const double* eu; const double* u;       // [batch][N][m]
    double* cost; double* res;               // [batch]             null: not wanted (the store is skipped, nothing else)
    double* grad;                            // [batch][N][m]
    double* costate;                         // [batch][N+1][n]
    int lds_per_wave;                        // doubles
};

constexpr int CERT_WAVES = 4;
constexpr int CERT_MAX_N = 64, CERT_MAX_M = 16;

__host__ __device__ inline int cert_ld(int n, int m) { return (n > m ? n : m) | 1; }
__host__ __device__ inline int cert_slot_doubles(int n, int m) { return 2 * n + 3 * m; }
__host__ __device__ inline int cert_lds_doubles(int n, int m) {
    return (cert_ld(n, m) * (3 * n + 3 * m) + 2 * cert_slot_doubles(n, m) + 1) & ~1;
}

__device__ __forceinline__ void cert_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// sum_j M(row, j) x_j (T: M(j, row)) over the lane's column group, joined over the groups: the same bits in every group.  Every
// lane takes part in the join; a lane whose row is beyond `rows` adds nothing and gets the sum of nothing.
template <int RL, bool T>
__device__ __forceinline__ double cert_mv(const double* M, const double* x, int rows, int cols, int ld, int row, int cg) {
    constexpr int CG = 64 / RL;
    double acc = 0.0;
    if (row < rows)
        for (int j = cg; j < cols; j += CG) acc += (T ? M[j + row * ld] : M[row + j * ld]) * x[j];
#pragma unroll
    for (int o = RL; o < 64; o <<= 1) acc += __shfl_xor(acc, o);
    return acc;
}

// the larger of two, a NaN once seen kept (fmax would drop it)
__device__ __forceinline__ double cert_nanmax(double a, double b) { return (b > a || b != b) ? b : a; }

template <int RL>
__global__ __launch_bounds__(64 * CERT_WAVES) void k_cert(CertParams p) {
    extern __shared__ __attribute__((aligned(16))) double cert_smem[];
    constexpr int CG = 64 / RL;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int n = p.n, m = p.m, N = p.N, ld = cert_ld(n, m);
    const int row = lane & (RL - 1), cg = lane / RL;
    const bool useR = p.useR != 0, useS = p.useS != 0;
    double* Al = cert_smem + (size_t)wv * p.lds_per_wave;
    double* Bl = Al + ld * n;   double* Ql = Bl + ld * m;   double* Pl = Ql + ld * n;
    double* Rl = Pl + ld * n;   double* Sl = Rl + ld * m;   double* slots = Sl + ld * m;
    const int so = cert_slot_doubles(n, m);
    // the lane's own entries of the stage vectors: lane = index (for a lane of column group 0 that is its row as well)
    const bool is_e = lane < n, is_u = lane < m;
    const bool own_x = cg == 0 && row < n, own_u = cg == 0 && row < m;
    const double lo = is_u ? p.umin[lane] : 0.0, hi = is_u ? p.umax[lane] : 0.0;
    const int wpb = (int)(blockDim.x >> 6), nwaves = gridDim.x * wpb;
    bool first = true;
    for (int inst = blockIdx.x * wpb + wv; inst < p.batch; inst += nwaves) {
        const double* exg = p.ex + (size_t)inst * (size_t)(N + 1) * n;
        const double* eug = p.eu + (size_t)inst * (size_t)N * m;
        const double* ug = p.u + (size_t)inst * (size_t)N * m;
        // stage N's e and the vectors of stage N-1 are on their way while the operands are staged
        const double eN = is_e ? exg[(size_t)N * n + lane] : 0.0;
        double e_p = is_e ? exg[(size_t)(N - 1) * n + lane] : 0.0;
        double v_p = is_u ? eug[(size_t)(N - 1) * m + lane] : 0.0;
        double u_p = is_u ? ug[(size_t)(N - 1) * m + lane] : 0.0;
        double d_p = (is_u && N >= 2) ? ug[(size_t)(N - 2) * m + lane] - u_p : 0.0;   // d_{N-2}
        cert_fence();   // (the previous instance's reads of the slice are done)
        if (row < n) {
            if (first || p.A_stride) {
                const double* Ag = p.A + (size_t)inst * p.A_stride;
                for (int j = cg; j < n; j += CG) Al[row + j * ld] = Ag[row + j * n];
            }
            if (first || p.B_stride) {
                const double* Bg = p.B + (size_t)inst * p.B_stride;
                for (int a = cg; a < m; a += CG) Bl[row + a * ld] = Bg[row + a * n];
            }
            if (first || p.Q_stride) {
                const double* Qg = p.Q + (size_t)inst * p.Q_stride;
                for (int j = cg; j < n; j += CG) Ql[row + j * ld] = 0.5 * (Qg[row + j * n] + Qg[j + row * n]);
            }
            if (first || p.P_stride) {
                const double* Pg = p.P + (size_t)inst * p.P_stride;
                for (int j = cg; j < n; j += CG) Pl[row + j * ld] = 0.5 * (Pg[row + j * n] + Pg[j + row * n]);
            }
        }
        if (row < m) {
            if (useR && (first || p.R_stride)) {
                const double* Rg = p.R + (size_t)inst * p.R_stride;
                for (int b = cg; b < m; b += CG) Rl[row + b * ld] = 0.5 * (Rg[row + b * m] + Rg[b + row * m]);
            }
            if (useS && (first || p.S_stride)) {
                const double* Sg = p.S + (size_t)inst * p.S_stride;
                for (int b = cg; b < m; b += CG) Sl[row + b * ld] = 0.5 * (Sg[row + b * m] + Sg[b + row * m]);
            }
        }
        first = false;
        double* cur = slots;        // lam | e | v | u | d
        double* nxt = slots + so;
        if (is_e) cur[n + lane] = eN;
        cert_fence();
        // lam_N = 2 P e_N
        double e_c = eN, v_c = 0.0, u_c = 0.0, d_c = 0.0;
        double lam = 2.0 * cert_mv<RL, false>(Pl, cur + n, n, n, ld, row, cg);
        double cost = own_x ? 0.5 * e_c * lam : 0.0, res = 0.0;
        if (p.costate && own_x) p.costate[(size_t)inst * (size_t)(N + 1) * n + (size_t)N * n + row] = lam;
        double s_up = 0.0;   // 2 S d_k of the stage above (zero at k = N-1: no pair beyond the horizon)
        for (int k = N - 1; k >= 0; --k) {
            // hand lam_{k+1} and stage k's vectors over, and take stage k-1's from memory
            if (own_x) nxt[row] = lam;
            if (is_e) nxt[n + lane] = e_p;
            if (is_u) { nxt[2 * n + lane] = v_p; nxt[2 * n + m + lane] = u_p; nxt[2 * n + 2 * m + lane] = d_p; }
            e_c = e_p; v_c = v_p; u_c = u_p; d_c = d_p;
            if (k >= 1) {
                if (is_e) e_p = exg[(size_t)(k - 1) * n + lane];
                if (is_u) {
                    v_p = eug[(size_t)(k - 1) * m + lane];
                    u_p = ug[(size_t)(k - 1) * m + lane];
                    d_p = k >= 2 ? ug[(size_t)(k - 2) * m + lane] - u_p : 0.0;   // d_{k-2}
                }
            }
            cert_fence();
            double* t = cur; cur = nxt; nxt = t;
            // cur: lam_{k+1} | e_k | v_k | u_k | d_{k-1}
            const double q = 2.0 * cert_mv<RL, false>(Ql, cur + n, n, n, ld, row, cg);
            const double rr = useR ? 2.0 * cert_mv<RL, false>(Rl, cur + 2 * n, m, m, ld, row, cg) : 0.0;
            const double s_dn = (useS && k >= 1) ? 2.0 * cert_mv<RL, false>(Sl, cur + 2 * n + 2 * m, m, m, ld, row, cg) : 0.0;   // 2 S d_{k-1}
            const double bl = cert_mv<RL, true>(Bl, cur, m, n, ld, row, cg);
            const double al = cert_mv<RL, true>(Al, cur, n, n, ld, row, cg);
            lam = q + al;
            const double g = bl + rr + (s_up - s_dn);
            s_up = s_dn;
            if (own_x) cost += 0.5 * e_c * q;
            if (own_u) {
                cost += 0.5 * v_c * rr + 0.5 * d_c * s_dn;
                const double w = u_c - g;
                const double c = w < lo ? lo : (w > hi ? hi : w);   // (comparisons: a NaN stays one)
                res = cert_nanmax(res, fabs(u_c - c));
            }
            if (p.costate && own_x) p.costate[(size_t)inst * (size_t)(N + 1) * n + (size_t)k * n + row] = lam;
            if (p.grad && own_u) p.grad[(size_t)inst * (size_t)N * m + (size_t)k * m + row] = g;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            cost += __shfl_xor(cost, o);
            res = cert_nanmax(res, __shfl_xor(res, o));
        }
        if (lane == 0) {
            if (p.cost) p.cost[inst] = cost;
            if (p.res) p.res[inst] = res;
        }
    }
}

}  // namespace almpc
