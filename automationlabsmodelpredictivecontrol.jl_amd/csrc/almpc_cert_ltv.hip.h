// almpc_cert_ltv.hip.h -- k_cert_ltv: predicted states, cost, costates, input gradient and KKT residual of a step of a time-varying
// design (almpc_design_ltv), from the returned u and e_u = v and the design data alone (no solver internals).
//
// Per instance, stages 0-based, v_k = e_u[:,k], u_k = u[:,k], w_k = u_k - uref_k, d_i = u_i - u_{i+1}; Q, R, S, P symmetrised
// (0.5 (M + M')); useR / useS as the design took them:
//   forward   dx_0 = 0,  dx_{k+1} = A_k dx_k + B_k v_k + c_k          (c = 0 if the design got NULL)
//             x_k = xbar_k + dx_k,  e_k = x_k - xref_k
//   cost      J = e_N'P e_N + sum_{k<N} (e_k'Q e_k + [useR] w_k'R w_k) + [useS] sum_{i<N-1} d_i'S d_i
//   backward  lam_N = 2 P e_N,  lam_k = 2 Q e_k + A_k'lam_{k+1}
//             g_k = B_k'lam_{k+1} + [useR] 2 R w_k + [useS]([k < N-1] 2 S d_k - [k > 0] 2 S d_{k-1})
//   res       max_{k,j} |u_k - clip(u_k - g_k, umin, umax)|
// Three identities tie this to the design's QP  min 1/2 v'Hv + q'v  (oracle/mpc_oracle.py::ltv_qp; tests/test_cert_ltv_restatement.py):
//   stacked g = H v + q;     J(v) - J(0) = 1/2 v'Hv + q'v;     lam_{k+1} = dJ/dc_k at fixed v.
//
// Shape: one wave per instance, CERT_LTV_WAVES waves per workgroup, a persistent capped grid; waves never wait for each other (no
// workgroup barrier, no atomics).  n, m <= 16: lane l owns row l & 15 and column group l >> 4, so a lane holds the four entries
// (row, cg + 4 t) of every operand matrix IN REGISTERS and a vector lives one element per lane, the same bits in all four groups.
// A product is four multiply-adds on __shfl'ed vector elements and a two-step __shfl_xor join; no vector goes through LDS.
//   once per wave       Q, R, S, a shared P (symmetrised on the way in), the input box
//   once per instance   its own P (P_stride != 0)
//   per stage           A_k, B_k, c_k and the stage vectors from global memory, straight into registers: the forward sweep reads
//                       rows (lanes of a group along a column: coalesced), the backward sweep the transpose (lane = column).  The loads
//                       of stage k+1 (backward: k-1) are issued before stage k's chain starts: their addresses do not depend on it.
//                       xref / uref are shared by the batch and stay in L2; they are read with the stage, off the chain as well.
//   LDS                 e_0 .. e_N, (N + 1) n <= 1024 doubles per wave, written by the forward sweep and read by the backward one
//                       (one wave-level fence between the sweeps, one in front of the next instance).
// Dependent chain per stage, forward: 8 multiply-adds on shuffled elements, the join, + c_k; x_k, e_k and the stores hang off it.
// Backward: as k_cert -- the A_k' product on lam_{k+1}, the join, one add; q_k = 2 Q e_k, 2 R w_k, the rate terms and B_k'lam_{k+1}
// hang off it.  The cost is summed per lane from the vectors already formed and reduced once by a butterfly, res by a maximum that
// keeps a NaN (cert_nanmax).  Every instance is computed whatever its status; what is not finite stays not finite.
#pragma once
#include "almpc_cert.hip.h"

namespace almpc {

struct CertLtvParams {
    int n, m, N, batch;
    int useR, useS;                          // the design's branch (one for the batch)
    const double* A;                         // [batch][N][n*n] column-major stage models
    const double* B;                         // [batch][N][n*m]
    const double* c;                         // [batch][N][n] or null (no defects)
    const double* Q; const double* R; const double* S;   // shared; R, S read only with useR, useS
    const double* P; long P_stride;          // n x n; stride 0: shared
    const double* umin; const double* umax;  // [m]
    const double* xbar;                      // [batch][N+1][n]
    const double* xref; const double* uref;  // [N+1][n], [N][m] shared
    const double* eu; const double* u;       // [batch][N][m]
    double* cost; double* res;               // [batch]             null: not wanted (the store is skipped, nothing else)
    double* grad;                            // [batch][N][m]
    double* costate;                         // [batch][N+1][n]
    double* x; double* ex;                   // [batch][N+1][n]
    int lds_per_wave;                        // doubles
};

constexpr int CERT_LTV_WAVES = 4;
constexpr int CERT_LTV_WGS_PER_CU = 8;   // the grid's cap: a wave walks the instances beyond it
constexpr int CERT_LTV_MAX_N = 16, CERT_LTV_MAX_M = 16, CERT_LTV_MAX_STATES = 1024;   // the shapes a step behind an LTV design accepts

// the lane's part of sum_j M(row, j) x_j: its entries (row, cg + 4 t) on the elements x_(cg + 4 t), which lane cg + 4 t holds
__device__ __forceinline__ double cert_ltv_dot(const double (&M)[4], double x, int cg) {
    double acc = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t) acc += M[t] * __shfl(x, cg + 4 * t);
    return acc;
}
// ... joined over the four column groups: the same bits in every group
__device__ __forceinline__ double cert_ltv_join(double acc) {
    acc += __shfl_xor(acc, 16);
    acc += __shfl_xor(acc, 32);
    return acc;
}
// G[i] where ok, else zero, without a branch: the load is unconditional (element 0 where !ok), so a wave's loads of a stage go out back to
// back and nothing waits for them before the stage that uses them
__device__ __forceinline__ double cert_ltv_at(const double* G, int i, bool ok) {
    const double v = G[ok ? i : 0];
    return ok ? v : 0.0;
}
// entries (row, cg + 4 t) of a rows x cols column-major matrix (T: of its transpose, cols x rows), zero beyond it
template <bool T>
__device__ __forceinline__ void cert_ltv_load(double (&M)[4], const double* G, int rows, int cols, int ldg, int row, int cg) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int j = cg + 4 * t;
        M[t] = cert_ltv_at(G, T ? j + row * ldg : row + j * ldg, row < rows && j < cols);
    }
}
// ... symmetrised
__device__ __forceinline__ void cert_ltv_load_sym(double (&M)[4], const double* G, int n, int row, int cg) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int j = cg + 4 * t;
        const bool ok = row < n && j < n;
        M[t] = 0.5 * (cert_ltv_at(G, row + j * n, ok) + cert_ltv_at(G, j + row * n, ok));
    }
}

__host__ __device__ inline int cert_ltv_lds_doubles(int n, int N) { return ((N + 1) * n + 1) & ~1; }

// HAS_C: the design got defects c_k (else the loads are not there)
template <bool HAS_C>
__global__ __launch_bounds__(64 * CERT_LTV_WAVES) void k_cert_ltv(CertLtvParams p) {
    extern __shared__ __attribute__((aligned(16))) double cert_ltv_smem[];
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int n = p.n, m = p.m, N = p.N;
    const int row = lane & 15, cg = lane >> 4;
    const bool useR = p.useR != 0, useS = p.useS != 0;
    const bool rx = row < n, ru = row < m, own_x = cg == 0 && rx, own_u = cg == 0 && ru;
    const int ne = (N + 1) * n, nu = N * m;
    double* E = cert_ltv_smem + (size_t)wv * p.lds_per_wave;   // e_k at E[k n + row]
    // once per wave: the shared weights and the box
    double Qr[4], Rr[4] = {0.0, 0.0, 0.0, 0.0}, Sr[4] = {0.0, 0.0, 0.0, 0.0}, Pr[4];
    cert_ltv_load_sym(Qr, p.Q, n, row, cg);
    if (useR) cert_ltv_load_sym(Rr, p.R, m, row, cg);
    if (useS) cert_ltv_load_sym(Sr, p.S, m, row, cg);
    if (!p.P_stride) cert_ltv_load_sym(Pr, p.P, n, row, cg);
    const double lo = cert_ltv_at(p.umin, row, ru), hi = cert_ltv_at(p.umax, row, ru);
    const int nn = n * n, nm = n * m;
    const int wpb = (int)(blockDim.x >> 6), nwaves = gridDim.x * wpb;
    for (int inst = blockIdx.x * wpb + wv; inst < p.batch; inst += nwaves) {
        const double* Ag = p.A + (size_t)inst * N * nn;
        const double* Bg = p.B + (size_t)inst * N * nm;
        const double* cgl = HAS_C ? p.c + (size_t)inst * N * n : nullptr;
        const double* xbg = p.xbar + (size_t)inst * (size_t)ne;
        const double* eug = p.eu + (size_t)inst * (size_t)nu;
        const double* ug = p.u + (size_t)inst * (size_t)nu;
        const size_t xo = (size_t)inst * (size_t)ne;
        if (p.P_stride) cert_ltv_load_sym(Pr, p.P + (size_t)inst * p.P_stride, n, row, cg);
        // ---- forward: stage 0's model and vectors are on their way while e_0 is formed
        double An[4], Bn[4];
        cert_ltv_load<false>(An, Ag, n, n, n, row, cg);
        cert_ltv_load<false>(Bn, Bg, n, m, n, row, cg);
        double c_n = HAS_C ? cert_ltv_at(cgl, row, rx) : 0.0;
        double v_n = cert_ltv_at(eug, row, ru);
        double xb_n = cert_ltv_at(xbg, n + row, rx), xr_n = cert_ltv_at(p.xref, n + row, rx);
        const double x0 = cert_ltv_at(xbg, row, rx);
        double e = x0 - cert_ltv_at(p.xref, row, rx);
        cert_fence();   // (the previous instance's reads of the slice are done)
        if (own_x) {
            E[row] = e;
            if (p.x) p.x[xo + row] = x0;
            if (p.ex) p.ex[xo + row] = e;
        }
        double dx = 0.0;
        for (int k = 0; k < N; ++k) {
            double Ac[4], Bc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) { Ac[t] = An[t]; Bc[t] = Bn[t]; }
            const double c_c = c_n, v_c = v_n, xb_c = xb_n, xr_c = xr_n;
            if (k + 1 < N) {
                cert_ltv_load<false>(An, Ag + (k + 1) * nn, n, n, n, row, cg);
                cert_ltv_load<false>(Bn, Bg + (k + 1) * nm, n, m, n, row, cg);
                c_n = HAS_C ? cert_ltv_at(cgl, (k + 1) * n + row, rx) : 0.0;
                v_n = cert_ltv_at(eug, (k + 1) * m + row, ru);
                xb_n = cert_ltv_at(xbg, (k + 2) * n + row, rx);
                xr_n = cert_ltv_at(p.xref, (k + 2) * n + row, rx);
            }
            const double s = cert_ltv_join(cert_ltv_dot(Ac, dx, cg) + cert_ltv_dot(Bc, v_c, cg));
            dx = rx ? s + c_c : 0.0;
            const double xk = xb_c + dx;
            e = rx ? xk - xr_c : 0.0;
            if (own_x) {
                E[(k + 1) * n + row] = e;
                if (p.x) p.x[xo + (size_t)(k + 1) * n + row] = xk;
                if (p.ex) p.ex[xo + (size_t)(k + 1) * n + row] = e;
            }
        }
        if (!(p.cost || p.res || p.grad || p.costate)) continue;   // (states only: uniform over the wave)
        // ---- backward: stage N-1's transposed model and inputs are on their way while lam_N is formed
        double At[4], Bt[4];
        cert_ltv_load<true>(At, Ag + (N - 1) * nn, n, n, n, row, cg);
        cert_ltv_load<true>(Bt, Bg + (N - 1) * nm, m, n, n, row, cg);
        double u_p = cert_ltv_at(ug, (N - 1) * m + row, ru);                  // u_k of the stage ahead
        double um_p = cert_ltv_at(ug, (N - 2) * m + row, ru && N >= 2);     // u_{k-1}
        double ur_p = cert_ltv_at(p.uref, (N - 1) * m + row, ru);
        cert_fence();   // e_0 .. e_N are in the slice
        double lam = 2.0 * cert_ltv_join(cert_ltv_dot(Pr, e, cg));   // (e is e_N in every group)
        lam = rx ? lam : 0.0;
        double cost = own_x ? 0.5 * e * lam : 0.0, res = 0.0;
        if (p.costate && own_x) p.costate[xo + (size_t)N * n + row] = lam;
        double s_up = 0.0;   // 2 S d_k of the stage above (zero at k = N-1: no pair beyond the horizon)
        for (int k = N - 1; k >= 0; --k) {
            double Ac[4], Bc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) { Ac[t] = At[t]; Bc[t] = Bt[t]; }
            const double u_c = u_p, ur_c = ur_p;
            const double d_c = (ru && k >= 1) ? um_p - u_c : 0.0;   // d_{k-1}
            u_p = um_p;
            if (k >= 1) {
                cert_ltv_load<true>(At, Ag + (k - 1) * nn, n, n, n, row, cg);
                cert_ltv_load<true>(Bt, Bg + (k - 1) * nm, m, n, n, row, cg);
                ur_p = cert_ltv_at(p.uref, (k - 1) * m + row, ru);
                um_p = cert_ltv_at(ug, (k - 2) * m + row, ru && k >= 2);
            }
            const double e_c = rx ? E[k * n + row] : 0.0;
            const double w_c = ru ? u_c - ur_c : 0.0;
            const double q = 2.0 * cert_ltv_join(cert_ltv_dot(Qr, e_c, cg));
            const double rr = useR ? 2.0 * cert_ltv_join(cert_ltv_dot(Rr, w_c, cg)) : 0.0;
            const double s_dn = (useS && k >= 1) ? 2.0 * cert_ltv_join(cert_ltv_dot(Sr, d_c, cg)) : 0.0;   // 2 S d_{k-1}
            const double bl = cert_ltv_join(cert_ltv_dot(Bc, lam, cg));
            const double al = cert_ltv_join(cert_ltv_dot(Ac, lam, cg));
            lam = rx ? q + al : 0.0;
            const double g = bl + rr + (s_up - s_dn);
            s_up = s_dn;
            if (own_x) cost += 0.5 * e_c * q;
            if (own_u) {
                cost += 0.5 * w_c * rr + 0.5 * d_c * s_dn;
                const double w = u_c - g;
                const double cl = w < lo ? lo : (w > hi ? hi : w);   // (comparisons: a NaN stays one)
                res = cert_nanmax(res, fabs(u_c - cl));
            }
            if (p.costate && own_x) p.costate[xo + (size_t)k * n + row] = lam;
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
