// almpc_ltv_stage.hip.h -- k_ltv_stage_prepare, k_ltv_stage_finish: the device side of almpc_design_ltv_stagewise /
// almpc_ltv_stagewise_update around the stage-wise solvers (k_riccati_t, k_sgains + k_sdual), which are launched as they are.
//
// k_ltv_stage_prepare is the device form of the two host loops of almpc_design_ltv (csrc/almpc_api.hip), in the shape the stage-wise
// solvers read.  Per instance, from the caller's trajectory (xbar, ubar) and the design's shared references and weights:
//   xbar_out, ubar_out   the handle's iterate buffers (the solvers' xref / xbref / uref / uguess): plain copies
//   ebar[k]  = xbar[k+1] - xref[k+1]                                  k = 0..N-1
//   qadd     = 2 Rbar (ubar - u_ref) + 2 D'Sbar D ubar                 the convention of the SQP loop's qadd (sqp_prepare_body):
//                                                                      k_sgains takes it with qscale 0.5, k_riccati_t with qu_scale 0.5
//   eqt      = xref[N]                                                 terminal-equality target (absolute coordinates), once
// R, S: symmetrised, column-major; useR / useS: the reference's branch rules (R[1,1] != 0; and S[1,1] != 0).  The sums run in the
// host loops' order: over the second index of the weight, the R term first, then -(rate k-1), then +(rate k).
//
// A streaming kernel: batch ((N+1) n + N m) doubles in, twice that out, 3 m + 1 cached re-reads of ubar per input element.  One wave
// per instance at a time, its lanes across the elements of the trajectory (consecutive addresses: coalesced), the waves of a capped
// grid walking the batch.  LDS holds R and S only; no atomics; no dependence between instances.
//
// k_ltv_stage_finish writes the step's absolute results from the solvers' deviations: u = ubar + e_u, x = xbar + e_x -- both hold
// bit for bit afterwards, which the solvers' own u (clamped first, e_u = u - ubar second) does not promise.
//
// The kernels are declared here for every reader and defined in one translation unit (almpc_tu_ltv_stage.hip; the unity build).
#pragma once
#include <hip/hip_runtime.h>

namespace almpc {

constexpr int LTV_STAGE_THREADS = 256;   // four waves: four instances in flight per workgroup
constexpr int LTV_STAGE_MAX_M = 16;      // R, S in LDS: 2 * 16 * 16 doubles

struct LtvStageParams {
    int n, m, N, batch, useR, useS;
    const double* xbar;   // [batch][N+1][n] the caller's (device form) or the staged (host form) trajectory
    const double* ubar;   // [batch][N][m]
    const double* xref;   // [N+1][n] shared references (zeros for NULL)
    const double* uref;   // [N][m]
    const double* R;      // [m][m] symmetrised
    const double* S;      // [m][m] symmetrised
    double* xbar_out;     // [batch][N+1][n]
    double* ubar_out;     // [batch][N][m]
    double* ebar;         // [batch][N][n]
    double* qadd;         // [batch][N][m]
    double* eqt;          // [n] or null: no terminal equality
};

struct LtvStageFinishParams {
    int n, m, N, batch;
    const double* xbar; const double* ubar;   // the handle's iterate buffers
    const double* ex;   const double* eu;     // the solvers' deviations
    double* x; double* u;
};

__global__ void k_ltv_stage_prepare(LtvStageParams p);
__global__ void k_ltv_stage_finish(LtvStageFinishParams p);

#if defined(ALMPC_LTV_STAGE_TU) || defined(ALMPC_UNITY)

__global__ __launch_bounds__(LTV_STAGE_THREADS) void k_ltv_stage_prepare(LtvStageParams p) {
    __shared__ double Rs[LTV_STAGE_MAX_M * LTV_STAGE_MAX_M], Ss[LTV_STAGE_MAX_M * LTV_STAGE_MAX_M];
    const int n = p.n, m = p.m, N = p.N;
    const int nx = (N + 1) * n, nu = N * m;
    for (int t = (int)threadIdx.x; t < m * m; t += (int)blockDim.x) { Rs[t] = p.R[t]; Ss[t] = p.S[t]; }
    __syncthreads();
    if (p.eqt && blockIdx.x == 0)
        for (int t = (int)threadIdx.x; t < n; t += (int)blockDim.x) p.eqt[t] = p.xref[(size_t)N * n + t];
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6), wpb = (int)(blockDim.x >> 6);
    const int nwaves = (int)gridDim.x * wpb;
    for (int inst = (int)blockIdx.x * wpb + wv; inst < p.batch; inst += nwaves) {
        const double* xb = p.xbar + (size_t)inst * nx;
        const double* ub = p.ubar + (size_t)inst * nu;
        double* xo = p.xbar_out + (size_t)inst * nx;
        double* eb = p.ebar + (size_t)inst * (size_t)(N * n);
        for (int t = lane; t < nx; t += 64) {
            const double x = xb[t];
            xo[t] = x;
            if (t >= n) eb[t - n] = x - p.xref[t];
        }
        double* uo = p.ubar_out + (size_t)inst * nu;
        double* qa = p.qadd + (size_t)inst * nu;
        for (int t = lane; t < nu; t += 64) {
            const int k = t / m, a = t - k * m;
            const double* uk = ub + k * m;
            uo[t] = ub[t];
            double g = 0.0;
            if (p.useR) {
                double sr = 0.0;
                for (int c = 0; c < m; ++c) sr += Rs[c * m + a] * (uk[c] - p.uref[k * m + c]);
                g += 2.0 * sr;
            }
            if (p.useS) {   // row t of 2 D'Sbar D ubar: the rate pair (k-1, k) enters with -, the pair (k, k+1) with +
                if (k > 0) {
                    double sd = 0.0;
                    for (int c = 0; c < m; ++c) sd += Ss[c * m + a] * (uk[c - m] - uk[c]);
                    g -= 2.0 * sd;
                }
                if (k + 1 < N) {
                    double sd = 0.0;
                    for (int c = 0; c < m; ++c) sd += Ss[c * m + a] * (uk[c] - uk[c + m]);
                    g += 2.0 * sd;
                }
            }
            qa[t] = g;
        }
    }
}

__global__ __launch_bounds__(LTV_STAGE_THREADS) void k_ltv_stage_finish(LtvStageFinishParams p) {
    const int nx = (p.N + 1) * p.n, nu = p.N * p.m;
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6), wpb = (int)(blockDim.x >> 6);
    const int nwaves = (int)gridDim.x * wpb;
    for (int inst = (int)blockIdx.x * wpb + wv; inst < p.batch; inst += nwaves) {
        const size_t ox = (size_t)inst * nx, ou = (size_t)inst * nu;
        for (int t = lane; t < nx; t += 64) p.x[ox + t] = p.xbar[ox + t] + p.ex[ox + t];
        for (int t = lane; t < nu; t += 64) p.u[ou + t] = p.ubar[ou + t] + p.eu[ou + t];
    }
}

#endif

}  // namespace almpc
