// almpc_sqp.hip.h -- device side of the SQP outer loop for black-box (Fnn) models.
//
// The reference's NonLinearProgramming branch poses   min  e_x[:,N+1]' P e_x[:,N+1] + sum_k e_x[:,k]' Q e_x[:,k] + e_u[:,k]' R e_u[:,k]
// s.t.  x[:,k+1] = fnn(x[:,k], u[:,k]),  umin <= u <= umax   (.../fnn/mpc_modeler_implementation_fnn.jl:110-189, cost
// src/sub/design_mpc.jl:405-468) and hands it to Ipopt.  Here the same NLP is solved by Gauss-Newton SQP with multiple shooting:
// every outer iteration linearises the network along the current trajectory (k_fnn_jacobian), builds the time-varying condensed
// QP (k_design_ltv) and solves it with the per-instance step kernels.  The kernels below are the glue that keeps the whole
// iteration on the device: defects and gradient pieces before the QP, the trajectory update after it.
// The iterate (xbar, ubar) lives in the handle's per-instance reference buffers (dXref, dUref): the QP variable is v = u - ubar.
#pragma once
#include <hip/hip_runtime.h>
#include "almpc_fnn.hip.h"
#include "almpc_kernels.hip.h"  // wave_max
#include "almpc_instance.hip.h" // SqpParams, sqp_prepare_body

namespace almpc {

// (struct SqpParams and sqp_prepare_body: csrc/almpc_instance.hip.h, beside the design kernel whose head runs them)

// Before the QP: defects, state errors and the input part of the gradient, one workgroup per instance.
// (see sqp_prepare_body)
inline __global__ __launch_bounds__(256) void k_sqp_prepare(SqpParams p) { sqp_prepare_body(p, blockIdx.x); }

// After the QP: dx_{k+1} = A_k dx_k + B_k v_k + c_k (dx_0 = 0), xbar += s dx, ubar += s v; one workgroup per instance.
// The recursion is a dependent chain of N small products.  All of its operands are staged in LDS first -- [A_k | B_k | c_k] of
// `chunk` stages at a time with the whole workgroup (one HBM round trip per chunk; the host sizes the chunk, normally all N
// stages), v once -- and wave 0 then walks the stages on its own: lane j < n owns dx_j, the previous dx comes from the lanes
// themselves (v_readlane), so a stage is n + m FMAs deep with no barrier.  Trajectory update, results and the batch maxima
// are done by all threads around it.
__host__ __device__ inline int sqp_step_chunk(int n, int m, int N) {
    const long E = (long)n * n + (long)n * m + n, fixed = (long)(N + 1) * n + (long)m * N + 16;
    long ch = (12288 - fixed) / E;  // 96 KB of doubles
    return (int)(ch < 1 ? 1 : (ch > N ? N : ch));
}
__host__ __device__ inline size_t sqp_step_lds_doubles(int n, int m, int N) {
    return (size_t)sqp_step_chunk(n, m, N) * ((size_t)n * n + (size_t)n * m + n) + (size_t)(N + 1) * n + (size_t)m * N + 16;
}

inline __global__ __launch_bounds__(256) void k_sqp_step(SqpParams p) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    __shared__ int skip;
    const int n = p.n, m = p.m, N = p.N, nz = p.nz, tid = threadIdx.x, nn = n * n, nm = n * m, E = nn + nm + n;
    const int CH = sqp_step_chunk(n, m, N);
    double* stage = smem;                       // [CH][E]
    double* dxa = stage + (size_t)CH * E;       // [(N+1)][n]: dx_0 = 0, dx_1, ...
    double* vs = dxa + (size_t)(N + 1) * n;     // [nz]
    double* red = vs + nz;                      // [16]
    const size_t i = blockIdx.x;
    const double* v = p.v + i * (size_t)nz;
    const double* cg = p.c + i * (size_t)N * n;
    double* xb = p.xbar + i * (size_t)(N + 1) * n;
    double* ub = p.ubar + i * (size_t)nz;
    const double* Ag = p.A + i * N * (size_t)nn;
    const double* Bg = p.B + i * N * (size_t)nm;
    // largest step / defect of this instance, and the finite check
    double vmax = 0.0, cmax = 0.0;
    int finite = 1;
    for (int t = tid; t < nz; t += 256) {
        const double a = v[t];
        vs[t] = a;
        finite &= (fabs(a) <= 1.79e308) ? 1 : 0;
        vmax = fmax(vmax, fabs(a));
    }
    for (int t = tid; t < N * n; t += 256) {
        const double a = fabs(cg[t]);
        finite &= (a <= 1.79e308) ? 1 : 0;
        cmax = fmax(cmax, a);
    }
    if (tid < n) dxa[tid] = 0.0;
    vmax = wave_max(vmax);
    cmax = wave_max(cmax);
    finite = __all(finite);
    if ((tid & 63) == 0) {
        red[tid >> 6] = vmax; red[4 + (tid >> 6)] = cmax; red[8 + (tid >> 6)] = finite ? 0.0 : 1.0;
    }
    __syncthreads();
    if (tid == 0) {
        const int frozen = p.done && p.done[i];   // converged in almpc_sqp_fnn_solve: never updated again
        const int redo_ = !frozen && p.adaptive && p.mer[4 * i + 2] != 0.0;   // trial point rejected in k_sqp_prepare: this QP is void
        const int bad = !frozen && !redo_ && ((red[8] + red[9] + red[10] + red[11] != 0.0) || p.flag[i] != 0 || p.status[i] == 2 || p.status[i] == 3);
        skip = frozen || bad || redo_;
        if (bad) p.bad[i] = 1;
        if (bad && p.verdict) p.verdict[i] = p.status[i] == 3 ? 3 : 2;
        else if (!redo_) {
            atomicMax(p.stats + 0, (unsigned long long)__double_as_longlong(fmax(fmax(red[0], red[1]), fmax(red[2], red[3]))));
            atomicMax(p.stats + 1, (unsigned long long)__double_as_longlong(fmax(fmax(red[4], red[5]), fmax(red[6], red[7]))));
        }
    }
    __syncthreads();
    // Step length: `step_scale`, times the instance's own factor under step rule 1 (k_sqp_prepare).  An instance whose last
    // trial point was just rejected there sits on a new, shorter trial: its QP of this iteration is void.
    double scale = p.step_scale;
    if (p.adaptive) scale *= p.mer[4 * i];  // the factor in force for the step taken now (k_sqp_prepare has just updated it)
    if (!skip) {
        double dxr = 0.0;                       // wave 0, lane j < n: dx_j of the current stage
        const int lj = tid < n ? tid : 0;
        for (int k0 = 0; k0 < N; k0 += CH) {
            const int cnt = (N - k0 < CH) ? N - k0 : CH;
            if (k0 > 0) __syncthreads();        // the previous chunk has been consumed
            for (int t = tid; t < cnt * E; t += 256) {
                const int k = k0 + t / E, e = t % E;
                stage[t] = e < nn ? Ag[(size_t)k * nn + e] : (e < nn + nm ? Bg[(size_t)k * nm + e - nn] : cg[(size_t)k * n + e - nn - nm]);
            }
            __syncthreads();
            if (tid < 64) {
                for (int kk = 0; kk < cnt; ++kk) {
                    const double* A = stage + (size_t)kk * E;
                    const double* B = A + nn;
                    double s = A[nn + nm + lj];
                    for (int c2 = 0; c2 < n; ++c2) s += A[c2 * n + lj] * readlane_d(dxr, c2);
                    for (int c2 = 0; c2 < m; ++c2) s += B[c2 * n + lj] * vs[(k0 + kk) * m + c2];
                    dxr = s;
                    if (tid < n) dxa[(size_t)(k0 + kk + 1) * n + tid] = s;
                }
            }
        }
        __syncthreads();
    }
    // trajectory update and results: the iterate itself (for a skipped instance: its last good iterate)
    if (p.adaptive && !skip) {  // remember the point this step leaves and the (full) step itself
        for (int t = tid; t < (N + 1) * n; t += 256) {
            p.xback[i * (size_t)(N + 1) * n + t] = xb[t];
            p.dxback[i * (size_t)(N + 1) * n + t] = p.step_scale * dxa[t];
        }
        for (int t = tid; t < nz; t += 256) {
            p.uback[i * (size_t)nz + t] = ub[t];
            p.vback[i * (size_t)nz + t] = p.step_scale * vs[t];
        }
    }
    for (int t = tid; t < (N + 1) * n; t += 256) {
        double xv = xb[t];
        if (!skip && t >= n) { xv += scale * dxa[t]; xb[t] = xv; }
        p.x[i * (size_t)(N + 1) * n + t] = xv;
        p.ex[i * (size_t)(N + 1) * n + t] = xv - p.xref[t];
    }
    for (int t = tid; t < nz; t += 256) {
        double uv = ub[t];
        if (!skip) {
            const int a = t % m;
            uv = fmin(fmax(uv + scale * vs[t], p.umin[a]), p.umax[a]);  // v is feasible: the clip only removes rounding
            ub[t] = uv;
        }
        p.u[i * (size_t)nz + t] = uv;
        p.eu[i * (size_t)nz + t] = uv - p.uref[t];
    }
}

// Stopping test of almpc_sqp_fnn_solve at the top of an iteration, at the iterate (xbar, ubar), on the network outputs and Jacobians
// the iteration's linearisation has just computed there; one workgroup per instance.
//     lam_N = 2 P e_N,  G_k = 2 R eu_k + B_k' lam_{k+1} (+ input-rate terms),  lam_k = 2 Q e_k + A_k' lam_{k+1}
//     residual = |U - clip(U - G / (2 R_aa))|_inf   (tests/sqp_solve_ref.py; with zero defects: the oracle's nlp_kkt_residual)
// An instance converges when max |f(x_k, u_k) - x_{k+1}| <= 1e-10 and residual <= tol: done[i] = 1, iters[i] = the iteration, and the
// live count goes down by one.  The adjoint recursion is a dependent chain of N stages walked backwards as k_sqp_step walks forwards:
// [A_k | B_k | 2 Q e_k] of `chunk` stages staged in LDS by the whole workgroup, then wave 0 alone, lane j < n owning lam_j and the
// previous lam read from the lanes (v_readlane), no barrier per stage.
// With state rows and their multipliers mu handed out by the finishes (RowMultOut; `mu` below not null):
//     lam_N = 2 P e_N + mu_N,   lam_k = 2 Q e_k + A_k' lam_{k+1} + mu_k      (mu_k rides in the 2 Q e_k slot of the staged chunk)
// and the residual is the maximum of the projected residual above with that adjoint, the complementarity |x - bound| over the box rows
// with mu != 0 (side by sign), the primal violation of the box, and |x_{N+1} - x_ref| under the terminal equality (whose rows replace
// the box rows of that stage).  tests/sqp_rows_ref.py restates it.
struct SqpKktParams {
    int n, m, N, nz, useS;
    const double* xref; const double* uref;   // [(N+1)][n], [N][m]
    const double* Q; const double* R; const double* S; const double* P; long sP;   // symmetrised
    const double* umin; const double* umax;
    const double* xbar; const double* ubar;   // [batch][(N+1)][n], [batch][N][m]
    const double* fval;                       // [batch][N][n] network outputs at (xbar_k, ubar_k)
    const double* A; const double* B;         // [batch][N][n*n], [batch][N][n*m]
    double tol;
    int it;                                   // iteration about to start (= QP iterations taken so far)
    int* done; int* iters; double* kkt;       // [batch]; done null: no test, the multipliers only (exact Hessian in iterate)
    int* live;                                // instances not yet converged
    double* lam = nullptr;                    // [batch][N][n] or null: lam_{k+1}, the multiplier of stage k's dynamics
    const double* mu = nullptr;               // [batch][N][n] or null: multipliers of the state rows, entry (k, i) the row of x_{k+1}[i]
    const double* xmin = nullptr; const double* xmax = nullptr;   // [n] state box or null (read with mu only)
    int term_eq = 0;                          // the rows of stage N + 1 are the terminal equality
};

inline __global__ __launch_bounds__(256) void k_sqp_kkt(SqpKktParams p) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const size_t i = blockIdx.x;
    if (p.done && p.done[i]) return;   // frozen: nothing of it changes any more (uniform per workgroup)
    const int n = p.n, m = p.m, N = p.N, nz = p.nz, tid = threadIdx.x, nn = n * n, nm = n * m, E = nn + nm + n;
    const int CH = sqp_step_chunk(n, m, N);
    double* stage = smem;                       // [CH][E]: A_k | B_k | 2 Q e_k (2 P e_N is lam_N)
    double* gs = stage + (size_t)CH * E;        // [nz] G_k, stage by stage
    double* red = gs + nz;                      // [16]
    const double* xb = p.xbar + i * (size_t)(N + 1) * n;
    const double* ub = p.ubar + i * (size_t)nz;
    const double* fv = p.fval + i * (size_t)N * n;
    const double* Ag = p.A + i * N * (size_t)nn;
    const double* Bg = p.B + i * N * (size_t)nm;
    const double* Pm = p.P + i * p.sP;
    const double* mug = p.mu ? p.mu + i * (size_t)N * n : nullptr;
    double dmax = 0.0;
    for (int t = tid; t < N * n; t += 256) {
        const double d = fabs(fv[t] - xb[n + t]);
        dmax = fmax(dmax, d == d ? d : 1.79e308);   // (a NaN defect never converges)
    }
    dmax = wave_max(dmax);
    if ((tid & 63) == 0) red[tid >> 6] = dmax;
    // lam_N = 2 P e_N, wave 0 lane j < n
    const int lj = tid < n ? tid : 0;
    double lam = 0.0;
    if (tid < 64) {
        for (int c2 = 0; c2 < n; ++c2) lam += Pm[(size_t)c2 * n + lj] * (xb[(size_t)N * n + c2] - p.xref[(size_t)N * n + c2]);
        lam *= 2.0;
        if (mug) lam += mug[(size_t)(N - 1) * n + lj];
    }
    int top = N;   // stages [0, top) not walked yet
    while (top > 0) {
        const int k0 = top - CH > 0 ? top - CH : 0, cnt = top - k0;
        __syncthreads();                        // the previous chunk has been consumed
        for (int t = tid; t < cnt * E; t += 256) {
            const int k = k0 + t / E, e = t % E;
            double v;
            if (e < nn) v = Ag[(size_t)k * nn + e];
            else if (e < nn + nm) v = Bg[(size_t)k * nm + e - nn];
            else {   // 2 Q e_k (stage 0: x_0 is fixed, no term)
                const int r = e - nn - nm;
                double s = 0.0;
                if (k > 0)
                    for (int c2 = 0; c2 < n; ++c2) s += p.Q[(size_t)c2 * n + r] * (xb[(size_t)k * n + c2] - p.xref[(size_t)k * n + c2]);
                v = 2.0 * s;
                if (mug && k > 0) v += mug[(size_t)(k - 1) * n + r];
            }
            stage[t] = v;
        }
        __syncthreads();
        if (tid < 64) {
            for (int kk = cnt - 1; kk >= 0; --kk) {
                const double* A = stage + (size_t)kk * E;
                const double* B = A + nn;
                double g = 0.0, s = A[nn + nm + lj];
                for (int c2 = 0; c2 < n; ++c2) {
                    const double l = readlane_d(lam, c2);
                    g += B[(size_t)(tid < m ? tid : 0) * n + c2] * l;   // (B_k' lam_{k+1})_a, lane a < m
                    s += A[(size_t)lj * n + c2] * l;                    // (A_k' lam_{k+1})_j, lane j < n
                }
                if (tid < m) gs[(size_t)(k0 + kk) * m + tid] = g;
                if (p.lam && tid < n) p.lam[(i * N + k0 + kk) * (size_t)n + tid] = lam;
                lam = s;
            }
        }
        top = k0;
    }
    __syncthreads();
    // G = 2 R eu + B' lam (+ 2 D'S D u): the projected residual in the Jacobi-scaled coordinates of nlp_kkt_residual
    double r = 0.0;
    for (int t = tid; t < nz; t += 256) {
        const int k = t / m, a = t % m;
        double g = gs[t], s = 0.0;
        for (int c2 = 0; c2 < m; ++c2) s += p.R[(size_t)c2 * m + a] * (ub[k * m + c2] - p.uref[k * m + c2]);
        g += 2.0 * s;
        if (p.useS) {
            double s2 = 0.0;
            for (int c2 = 0; c2 < m; ++c2) {
                const double sac = p.S[(size_t)c2 * m + a];
                if (k + 1 < N) s2 += sac * (ub[k * m + c2] - ub[(k + 1) * m + c2]);
                if (k > 0) s2 -= sac * (ub[(k - 1) * m + c2] - ub[k * m + c2]);
            }
            g += 2.0 * s2;
        }
        const double u = ub[t], sc = 1.0 / fmax(2.0 * p.R[(size_t)a * m + a], 1e-12);
        const double proj = fmin(fmax(u - sc * g, p.umin[a]), p.umax[a]);
        const double d = fabs(u - proj);
        r = fmax(r, d == d ? d : 1.79e308);
    }
    if (mug) {   // state rows: complementarity and primal feasibility at the iterate
        for (int t = tid; t < N * n; t += 256) {
            const int c2 = t % n;
            const double x = xb[n + t], mv = mug[t];
            double d = 0.0;
            if (p.term_eq && t >= (N - 1) * n) d = fabs(x - p.xref[n + t]);
            else if (p.xmin) {
                const double lo = p.xmin[c2], hi = p.xmax[c2];
                d = fmax(fmax(x - hi, lo - x), 0.0);
                if (mv > 0.0) d = fmax(d, fabs(x - hi));
                else if (mv < 0.0) d = fmax(d, fabs(x - lo));
            }
            r = fmax(r, d == d ? d : 1.79e308);
        }
    }
    r = wave_max(r);
    if ((tid & 63) == 0) red[4 + (tid >> 6)] = r;
    __syncthreads();
    if (tid == 0 && p.done) {
        const double dm = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
        const double rr = fmax(fmax(red[4], red[5]), fmax(red[6], red[7]));
        p.kkt[i] = rr;
        p.iters[i] = p.it;
        if (dm <= 1e-10 && rr <= p.tol) {
            p.done[i] = 1;
            atomicSub(p.live, 1);
        }
    }
}

// Exact-Hessian mode (almpc_sqp_fnn_set_hessian): the stage Lagrangian Hessian of the network at every (instance, stage),
//     W_k = d^2/dz^2 (lam_{k+1}' f(z_k)) = sum_j M_j' diag(ybar_j * act''(a_j)) M_j,   z = [x; u]
// M_j = d a_j / d z the forward Jacobian chain (as k_fnn_jacobian forms it), ybar_j the adjoint of act(a_j) from W_out' lam (the
// ResNet and PolyNet sites: below; the kind is the kernel's template parameter).  One wave per point, four per workgroup, each with
// its own LDS scratch (fnn_hess_wave_doubles); weights read through the cache.
// Entries are summed as (M_r M_c) c so that W_k is exactly symmetric.  tests/sqp_exact_ref.py::stage_hessian restates it.
__device__ __forceinline__ void fnn_act2(int act, double a, double& d1, double& d2) {
    switch (act) {
        case 2: { const double t = tanh(a); d1 = 1.0 - t * t; d2 = -2.0 * t * d1; break; }
        case 3: { const double s = 1.0 / (1.0 + exp(-a)); d1 = s * (1.0 - s); d2 = d1 * (1.0 - 2.0 * s); break; }
        case 4: { const double s = 1.0 / (1.0 + exp(-a)); d1 = s * (1.0 + a * (1.0 - s)); d2 = s * (1.0 - s) * (2.0 + a * (1.0 - 2.0 * s)); break; }
        case 1: d1 = a > 0.0 ? 1.0 : 0.0; d2 = 0.0; break;
        default: d1 = 1.0; d2 = 0.0; break;
    }
}
// (activation sites: L, PolyNet 2 L -- a1 and a2 of every layer; DenseNet: y, ybar and J have (L+1) H rows)
__host__ __device__ inline size_t fnn_hess_wave_doubles(int n, int m, int H, int L, int net = NET_FNN) {
    const size_t nin = (size_t)n + m, S = net == NET_POLYNET ? 2 * (size_t)L : (size_t)L;
    if (net == NET_DENSENET) return nin + (2 * (size_t)(L + 1) + 1) * H + (size_t)(L + 1) * H * nin + 2 * S * H + S * H * nin;
    return nin + 3 * (size_t)H + (size_t)H * nin + 2 * S * H + S * H * nin;
}
struct FnnHessParams {
    int n, m, H, L, act, N, batch;
    const double* W_in; const double* W_h; const double* b_h; const double* W_out;   // layout of FnnParams
    const double* xbar; const double* ubar;   // [batch][(N+1)][n], [batch][N][m]
    const double* lam;                        // [batch][N][n]
    const int* done;                          // [batch] or null: frozen instances are skipped
    double* W;                                // [batch][N][(n+m)^2] column-major
};

// DenseNet (one site per hidden layer, a_l = W_h[l] y_{l+1} + b_h[l], M_l = W_h[l] J_{l+1}): the adjoint of Y starts at W_out' lam and
// walks back one layer at a time: the site weight is ybar_new act''(a_l) (ybar_new: the adjoint of the H rows layer l appended), and
// ybar_old += W_h[l]' (act'(a_l) .* ybar_new) lands on the rows the layer read (the layer's rows of Y are not read again).
// Scratch per wave: z | Y, ybar [(L+1) H] | t [H] | J [(L+1) H][nin] | Aa, Cc [L][H] | M [L][H][nin] (fnn_hess_wave_doubles).
__device__ __forceinline__ void densenet_lag_hessian(const FnnHessParams& p) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int n = p.n, m = p.m, H = p.H, L = p.L, nin = n + m, R = (L + 1) * H, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double* z = smem + (size_t)wv * fnn_hess_wave_doubles(n, m, H, L, NET_DENSENET);
    double* Y = z + nin;                  // [R] append order, as k_fnn_jacobian<NET_DENSENET>
    double* yb = Y + R;                   // [R]
    double* t = yb + R;                   // [H]
    double* J = t + H;                    // [R][nin] row-major: d Y / d z
    double* Aa = J + (size_t)R * nin;     // [L][H] pre-activations
    double* Cc = Aa + (size_t)L * H;      // [L][H] ybar_new * act''
    double* M = Cc + (size_t)L * H;       // [L][H][nin] d a_l / d z
    const long pt = (long)blockIdx.x * 4 + wv;
    if (pt >= (long)p.batch * p.N) return;   // (wave-uniform; no workgroup barrier below)
    const long inst = pt / p.N;
    const int k = (int)(pt % p.N);
    if (p.done && p.done[inst]) return;
    auto wsync = []() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); };
    for (int c = lane; c < nin; c += 64)
        z[c] = c < n ? p.xbar[(inst * (p.N + 1) + k) * n + c] : p.ubar[(inst * p.N + k) * m + c - n];
    wsync();
    for (int i = lane; i < H; i += 64) {
        double s = 0.0;
        for (int c = 0; c < nin; ++c) s += p.W_in[(size_t)c * H + i] * z[c];
        Y[i] = s;
    }
    for (int e = lane; e < H * nin; e += 64) J[e] = p.W_in[(size_t)(e % nin) * H + e / nin];
    wsync();
    for (int l = 0; l < L; ++l) {
        const double* W = p.W_h + densenet_wh_offset(H, l);
        for (int i = lane; i < H; i += 64) Aa[l * H + i] = densenet_dot(p.b_h[(size_t)l * H + i], W, H, i, Y, 1, H, l + 1);
        for (int e = lane; e < H * nin; e += 64) {
            const int i = e / nin, c = e % nin;
            M[((size_t)l * H + i) * nin + c] = densenet_dot(0.0, W, H, i, J + c, nin, H, l + 1);
        }
        wsync();
        for (int i = lane; i < H; i += 64) {
            double val, der;
            fnn_act(p.act, Aa[l * H + i], val, der);
            Y[(l + 1) * H + i] = val;
        }
        for (int e = lane; e < H * nin; e += 64) {
            double val, der;
            fnn_act(p.act, Aa[l * H + e / nin], val, der);
            J[(size_t)(l + 1) * H * nin + e] = M[(size_t)l * H * nin + e] * der;
        }
        wsync();
    }
    const double* lam = p.lam + (inst * p.N + k) * (size_t)n;
    for (int e = lane; e < R; e += 64) {   // Y row e = (block q, j) is column (L - q) H + j of W_out
        const int c = (L - e / H) * H + e % H;
        double s = 0.0;
        for (int r = 0; r < n; ++r) s += p.W_out[(size_t)c * n + r] * lam[r];
        yb[e] = s;
    }
    wsync();
    for (int l = L - 1; l >= 0; --l) {
        const double* W = p.W_h + densenet_wh_offset(H, l);
        const double* ob = yb + (size_t)(l + 1) * H;   // ybar_new
        for (int i = lane; i < H; i += 64) {
            double d1, d2;
            fnn_act2(p.act, Aa[l * H + i], d1, d2);
            Cc[l * H + i] = ob[i] * d2;
            t[i] = ob[i] * d1;
        }
        wsync();
        for (int c = lane; c < (l + 1) * H; c += 64) {   // column c of W_h[l] read Y row (l - c / H) H + c % H
            double s = 0.0;
            for (int i = 0; i < H; ++i) s += W[(size_t)c * H + i] * t[i];
            const int e = (l - c / H) * H + c % H;
            yb[e] = yb[e] + s;
        }
        wsync();
    }
    double* Wo = p.W + pt * (size_t)nin * nin;
    for (int e = lane; e < nin * nin; e += 64) {
        const int r = e % nin, c = e / nin;
        double s = 0.0;
        for (int l = 0; l < L; ++l)
            for (int i = 0; i < H; ++i) {
                const double* Mi = M + ((size_t)l * H + i) * nin;
                s += (Mi[r] * Mi[c]) * Cc[l * H + i];
            }
        Wo[e] = s;
    }
}

// ResNet: one site per layer, y' = y + act(a):  J' = J + diag(act') M,  ybar = ybar' + W' (act' .* ybar'),  site weight ybar' act''.
// PolyNet: two sites per layer, a1 = W y + b and a2 = W p + b (p = act(a1), M2 = W diag(act'(a1)) M1, J' = J + diag(act'(a1)) M1 +
// diag(act'(a2)) M2); backwards  pbar = ybar' + W' (act'(a2) .* ybar'),  ybar = ybar' + W' (act'(a1) .* pbar),  site weights
// ybar' act''(a2) and pbar act''(a1).  Site s of layer l is l (Fnn, ResNet) or 2 l + {0, 1} (PolyNet).
template <int NET>
__global__ __launch_bounds__(256) void k_fnn_lag_hessian(FnnHessParams p) {
    if constexpr (NET == NET_DENSENET) return densenet_lag_hessian(p);   // (its own body, above)
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int SPL = NET == NET_POLYNET ? 2 : 1;   // sites per layer
    const int n = p.n, m = p.m, H = p.H, L = p.L, S = SPL * L, nin = n + m, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double* z = smem + (size_t)wv * fnn_hess_wave_doubles(n, m, H, L, NET);
    double* y = z + nin;                  // [H]
    double* yb = y + H;                   // [H]
    double* t = yb + H;                   // [H]
    double* J = t + H;                    // [H][nin] row-major: d y / d z
    double* Aa = J + (size_t)H * nin;     // [S][H] pre-activations
    double* Cc = Aa + (size_t)S * H;      // [S][H] ybar * act''
    double* M = Cc + (size_t)S * H;       // [S][H][nin] d a_s / d z
    const long pt = (long)blockIdx.x * 4 + wv;
    if (pt >= (long)p.batch * p.N) return;   // (wave-uniform; no workgroup barrier below)
    const long inst = pt / p.N;
    const int k = (int)(pt % p.N);
    if (p.done && p.done[inst]) return;
    auto wsync = []() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); };
    for (int c = lane; c < nin; c += 64)
        z[c] = c < n ? p.xbar[(inst * (p.N + 1) + k) * n + c] : p.ubar[(inst * p.N + k) * m + c - n];
    wsync();
    for (int i = lane; i < H; i += 64) {
        double s = 0.0;
        for (int c = 0; c < nin; ++c) s += p.W_in[(size_t)c * H + i] * z[c];
        y[i] = s;
    }
    for (int e = lane; e < H * nin; e += 64) J[e] = p.W_in[(size_t)(e % nin) * H + e / nin];
    wsync();
    for (int l = 0; l < L; ++l) {
        const double* W = p.W_h + (size_t)l * H * H;
        const int s1 = SPL * l;
        for (int i = lane; i < H; i += 64) {
            double s = p.b_h[(size_t)l * H + i];
            for (int j = 0; j < H; ++j) s += W[(size_t)j * H + i] * y[j];
            Aa[s1 * H + i] = s;
        }
        for (int e = lane; e < H * nin; e += 64) {
            const int i = e / nin, c = e % nin;
            double s = 0.0;
            for (int j = 0; j < H; ++j) s += W[(size_t)j * H + i] * J[(size_t)j * nin + c];
            M[((size_t)s1 * H + i) * nin + c] = s;
        }
        wsync();
        if constexpr (NET == NET_POLYNET) {   // t = p = act(a1), yb = act'(a1) (yb is free until the backward pass)
            for (int i = lane; i < H; i += 64) {
                double val, der;
                fnn_act(p.act, Aa[s1 * H + i], val, der);
                t[i] = val;
                yb[i] = der;
            }
            wsync();
            const double* M1 = M + (size_t)s1 * H * nin;
            for (int i = lane; i < H; i += 64) {
                double s = p.b_h[(size_t)l * H + i];
                for (int j = 0; j < H; ++j) s += W[(size_t)j * H + i] * t[j];
                Aa[(s1 + 1) * H + i] = s;
            }
            for (int e = lane; e < H * nin; e += 64) {
                const int i = e / nin, c = e % nin;
                double s = 0.0;
                for (int j = 0; j < H; ++j) s += W[(size_t)j * H + i] * (yb[j] * M1[(size_t)j * nin + c]);
                M[((size_t)(s1 + 1) * H + i) * nin + c] = s;
            }
            wsync();
            for (int i = lane; i < H; i += 64) {
                double val, der;
                fnn_act(p.act, Aa[(s1 + 1) * H + i], val, der);
                y[i] = y[i] + t[i] + val;
            }
            for (int e = lane; e < H * nin; e += 64) {
                double val, der;
                fnn_act(p.act, Aa[(s1 + 1) * H + e / nin], val, der);
                J[e] = J[e] + yb[e / nin] * M1[e] + M[(size_t)(s1 + 1) * H * nin + e] * der;
            }
            wsync();
        } else {
            for (int i = lane; i < H; i += 64) {
                double val, der;
                fnn_act(p.act, Aa[s1 * H + i], val, der);
                if constexpr (NET == NET_RESNET) y[i] = y[i] + val;
                else y[i] = val;
            }
            for (int e = lane; e < H * nin; e += 64) {
                double val, der;
                fnn_act(p.act, Aa[s1 * H + e / nin], val, der);
                if constexpr (NET == NET_RESNET) J[e] = J[e] + M[(size_t)s1 * H * nin + e] * der;
                else J[e] = M[(size_t)s1 * H * nin + e] * der;
            }
            wsync();
        }
    }
    const double* lam = p.lam + (inst * p.N + k) * (size_t)n;
    for (int i = lane; i < H; i += 64) {
        double s = 0.0;
        for (int r = 0; r < n; ++r) s += p.W_out[(size_t)i * n + r] * lam[r];
        yb[i] = s;
    }
    wsync();
    for (int l = L - 1; l >= 0; --l) {
        const double* W = p.W_h + (size_t)l * H * H;
        const int s1 = SPL * l;
        // ob: the adjoint of the site act(a_{s1}) -- ybar' (Fnn, ResNet) or pbar (PolyNet, in y: the forward values are not read again)
        double* ob = yb;
        if constexpr (NET == NET_POLYNET) {
            for (int i = lane; i < H; i += 64) {
                double d1, d2;
                fnn_act2(p.act, Aa[(s1 + 1) * H + i], d1, d2);
                Cc[(s1 + 1) * H + i] = yb[i] * d2;
                t[i] = yb[i] * d1;
            }
            wsync();
            for (int j = lane; j < H; j += 64) {
                double s = 0.0;
                for (int i = 0; i < H; ++i) s += W[(size_t)j * H + i] * t[i];
                y[j] = yb[j] + s;
            }
            wsync();
            ob = y;
        }
        for (int i = lane; i < H; i += 64) {
            double d1, d2;
            fnn_act2(p.act, Aa[s1 * H + i], d1, d2);
            Cc[s1 * H + i] = ob[i] * d2;
            t[i] = ob[i] * d1;
        }
        wsync();
        for (int j = lane; j < H; j += 64) {
            double s = 0.0;
            for (int i = 0; i < H; ++i) s += W[(size_t)j * H + i] * t[i];
            if constexpr (NET == NET_FNN) yb[j] = s;
            else yb[j] = yb[j] + s;
        }
        wsync();
    }
    double* Wo = p.W + pt * (size_t)nin * nin;
    for (int e = lane; e < nin * nin; e += 64) {
        const int r = e % nin, c = e / nin;
        double s = 0.0;
        for (int l = 0; l < S; ++l)
            for (int i = 0; i < H; ++i) {
                const double* Mi = M + ((size_t)l * H + i) * nin;
                s += (Mi[r] * Mi[c]) * Cc[l * H + i];
            }
        Wo[e] = s;
    }
}

// The exact condensed QP from the Gauss-Newton one k_design_ltv has just written (unscaled H, q), one workgroup per instance:
//     H += sum_k M_k' W_k M_k,  q += sum_k M_k' W_k [g_k; 0],  M_k = [Gam_k; E_k]  (dx_k = Gam_k v + g_k, E_k selects v_k)
// Gam_k, g_k are propagated stage by stage in LDS (Gam_0 = 0, g_0 = 0); every thread keeps its entries of the update in registers
// (entries a <= b only: H stays exactly symmetric).  Then the inertia rule: delta = max(0, max_a sum_{b != a} |H_ab| - H_aa)
// (Gershgorin bound of the result) on the diagonal of every input that sits on a bound at the iterate.  nz <= 128.
constexpr int SQP_EXACT_REGS = 64;   // 128^2 / 256 entries per thread
struct SqpExactParams {
    int n, m, N, nz;
    const double* A; const double* B; const double* c;   // [batch][N][n*n], [batch][N][n*m], [batch][N][n] (defects)
    const double* W;                                     // [batch][N][(n+m)^2]
    const double* ubar; const double* umin; const double* umax;
    const int* done;                                     // [batch] or null
    double* H; double* q;                                // [batch][nz*nz] column-major, [batch][nz]
};
__host__ __device__ inline size_t sqp_exact_lds_doubles(int n, int m, int nz) {
    const size_t nin = (size_t)n + m;
    return 2 * (size_t)n * nz + 2 * (size_t)n + nin * nz + nin + nin * nin + (size_t)n * n + (size_t)n * m + n + 8;
}

inline __global__ __launch_bounds__(256) void k_sqp_exact_qp(SqpExactParams p) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const size_t i = blockIdx.x;
    if (p.done && p.done[i]) return;
    const int n = p.n, m = p.m, N = p.N, nz = p.nz, nin = n + m, tid = threadIdx.x, nn = n * n, nm = n * m;
    double* G = smem;                        // [n][nz] Gam_k (row-major)
    double* Gn = G + (size_t)n * nz;
    double* g = Gn + (size_t)n * nz;         // [n]
    double* gn = g + n;
    double* T = gn + n;                      // [nin][nz] W_k M_k
    double* tg = T + (size_t)nin * nz;       // [nin] W_k [g_k; 0]
    double* Wk = tg + nin;                   // [nin][nin] column-major
    double* Ak = Wk + (size_t)nin * nin;
    double* Bk = Ak + nn;
    double* ck = Bk + nm;
    double* red = ck + n;                    // [8]
    double acc[SQP_EXACT_REGS];
#pragma unroll
    for (int j = 0; j < SQP_EXACT_REGS; ++j) acc[j] = 0.0;
    double qacc = 0.0;
    for (int t = tid; t < n * nz; t += 256) G[t] = 0.0;
    for (int t = tid; t < n; t += 256) g[t] = 0.0;
    for (int k = 0; k < N; ++k) {
        for (int t = tid; t < nin * nin; t += 256) Wk[t] = p.W[(i * N + k) * (size_t)nin * nin + t];
        for (int t = tid; t < nn; t += 256) Ak[t] = p.A[(i * N + k) * (size_t)nn + t];
        for (int t = tid; t < nm; t += 256) Bk[t] = p.B[(i * N + k) * (size_t)nm + t];
        for (int t = tid; t < n; t += 256) ck[t] = p.c[(i * N + k) * (size_t)n + t];
        __syncthreads();
        for (int t = tid; t < nin * nz; t += 256) {   // T = W_k M_k
            const int r = t / nz, col = t % nz, kc = col - k * m;
            double s = 0.0;
            for (int s2 = 0; s2 < n; ++s2) s += Wk[(size_t)s2 * nin + r] * G[(size_t)s2 * nz + col];
            if (kc >= 0 && kc < m) s += Wk[(size_t)(n + kc) * nin + r];
            T[t] = s;
        }
        for (int r = tid; r < nin; r += 256) {
            double s = 0.0;
            for (int s2 = 0; s2 < n; ++s2) s += Wk[(size_t)s2 * nin + r] * g[s2];
            tg[r] = s;
        }
        for (int t = tid; t < n * nz; t += 256) {     // Gam_{k+1} = A_k Gam_k + B_k E_k
            const int r = t / nz, col = t % nz, kc = col - k * m;
            double s = 0.0;
            for (int s2 = 0; s2 < n; ++s2) s += Ak[(size_t)s2 * n + r] * G[(size_t)s2 * nz + col];
            if (kc >= 0 && kc < m) s += Bk[(size_t)kc * n + r];
            Gn[t] = s;
        }
        for (int r = tid; r < n; r += 256) {
            double s = ck[r];
            for (int s2 = 0; s2 < n; ++s2) s += Ak[(size_t)s2 * n + r] * g[s2];
            gn[r] = s;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < SQP_EXACT_REGS; ++j) {
            const int e = tid + 256 * j;
            if (e < nz * nz) {
                const int a = e % nz, b = e / nz;
                if (a <= b) {
                    double s = 0.0;
                    for (int r = 0; r < n; ++r) s += G[(size_t)r * nz + a] * T[(size_t)r * nz + b];
                    const int ka = a - k * m;
                    if (ka >= 0 && ka < m) s += T[(size_t)(n + ka) * nz + b];
                    acc[j] += s;
                }
            }
        }
        if (tid < nz) {
            double s = 0.0;
            for (int r = 0; r < n; ++r) s += G[(size_t)r * nz + tid] * tg[r];
            const int ka = tid - k * m;
            if (ka >= 0 && ka < m) s += tg[n + ka];
            qacc += s;
        }
        __syncthreads();
        for (int t = tid; t < n * nz; t += 256) G[t] = Gn[t];
        for (int t = tid; t < n; t += 256) g[t] = gn[t];
        // (the next stage's loads follow; its first barrier orders these copies before their use)
    }
    double* Hi = p.H + i * (size_t)nz * nz;
#pragma unroll
    for (int j = 0; j < SQP_EXACT_REGS; ++j) {
        const int e = tid + 256 * j;
        if (e < nz * nz) {
            const int a = e % nz, b = e / nz;
            if (a <= b) {
                const double v = Hi[(size_t)b * nz + a] + acc[j];
                acc[j] = v;
                Hi[(size_t)b * nz + a] = v;
                Hi[(size_t)a * nz + b] = v;
            }
        }
    }
    if (tid < nz) p.q[i * (size_t)nz + tid] += qacc;
    __syncthreads();   // (H of this instance written by the workgroup: visible to it from here on)
    double dl = 0.0;
    for (int a = tid; a < nz; a += 256) {   // row sums in a fixed order: the shift is reproducible bit for bit
        double sa = 0.0;
        for (int b = 0; b < nz; ++b) sa += b == a ? 0.0 : fabs(Hi[(size_t)a * nz + b]);
        dl = fmax(dl, sa - Hi[(size_t)a * nz + a]);
    }
    dl = wave_max(dl);
    if ((tid & 63) == 0) red[tid >> 6] = dl;
    __syncthreads();
    const double delta = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    if (delta > 0.0) {
#pragma unroll
        for (int j = 0; j < SQP_EXACT_REGS; ++j) {
            const int e = tid + 256 * j;
            if (e < nz * nz && e % nz == e / nz) {
                const int a = e % nz;
                const double u = p.ubar[i * (size_t)nz + a];
                if (u <= p.umin[a % m] || u >= p.umax[a % m]) Hi[(size_t)a * nz + a] = acc[j] + delta;
            }
        }
    }
}

// Single-shooting start: xbar_0 = x0, xbar_{k+1} = net(xbar_k, ubar_k) for a network of kind NET (the template parameter).  One
// workgroup per instance, thread i owns neuron i.
struct FnnRolloutParams {
    int n, m, H, L, act, N;
    const double* W_in; const double* W_h; const double* b_h; const double* W_out;
    const double* x0;     // [batch][n]
    const double* ubar;   // [batch][N][m]
    double* xbar;         // [batch][(N+1)][n]
};
// LDS of k_fnn_rollout: y, yn | z (DenseNet: Y [(L+1) H] | z)
__host__ __device__ inline size_t fnn_rollout_lds_doubles(int n, int m, int H, int L, int net = NET_FNN) {
    return (net == NET_DENSENET ? (size_t)(L + 1) * H : 2 * (size_t)H) + n + m;
}

// DenseNet rollout: Y [(L+1) H] in append order, z [nin] (fnn_rollout_lds_doubles); every layer appends its H rows, one barrier each
__device__ __forceinline__ void densenet_rollout(const FnnRolloutParams& p) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int n = p.n, m = p.m, H = p.H, L = p.L, nin = n + m;
    double* Y = smem;                          // [(L+1) H]
    double* z = Y + (size_t)(L + 1) * H;       // [nin]
    const size_t inst = blockIdx.x;
    double* xb = p.xbar + inst * (size_t)(p.N + 1) * n;
    const double* ub = p.ubar + inst * (size_t)p.N * m;
    for (int t = threadIdx.x; t < n; t += blockDim.x) {
        const double v = p.x0[inst * n + t];
        z[t] = v;
        xb[t] = v;
    }
    __syncthreads();
    for (int k = 0; k < p.N; ++k) {
        for (int t = threadIdx.x; t < m; t += blockDim.x) z[n + t] = ub[k * m + t];
        __syncthreads();
        for (int i = threadIdx.x; i < H; i += blockDim.x) {
            double s = 0.0;
            for (int c = 0; c < nin; ++c) s += p.W_in[(size_t)c * H + i] * z[c];
            Y[i] = s;
        }
        __syncthreads();
        for (int l = 0; l < L; ++l) {
            const double* W = p.W_h + densenet_wh_offset(H, l);
            for (int i = threadIdx.x; i < H; i += blockDim.x) {
                double val, der;
                fnn_act(p.act, densenet_dot(p.b_h[(size_t)l * H + i], W, H, i, Y, 1, H, l + 1), val, der);
                Y[(size_t)(l + 1) * H + i] = val;
            }
            __syncthreads();
        }
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const double s = densenet_dot(0.0, p.W_out, n, i, Y, 1, H, L + 1);
            z[i] = s;
            xb[(size_t)(k + 1) * n + i] = s;
        }
        __syncthreads();
    }
}

template <int NET>
__global__ __launch_bounds__(256) void k_fnn_rollout(FnnRolloutParams p) {
    if constexpr (NET == NET_DENSENET) return densenet_rollout(p);   // (its own body, above)
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int n = p.n, m = p.m, H = p.H, nin = n + m;
    double* y = smem;        // [H]
    double* yn = y + H;      // [H]
    double* z = yn + H;      // [nin]
    const size_t inst = blockIdx.x;
    double* xb = p.xbar + inst * (size_t)(p.N + 1) * n;
    const double* ub = p.ubar + inst * (size_t)p.N * m;
    for (int t = threadIdx.x; t < n; t += blockDim.x) {
        const double v = p.x0[inst * n + t];
        z[t] = v;
        xb[t] = v;
    }
    __syncthreads();
    for (int k = 0; k < p.N; ++k) {
        for (int t = threadIdx.x; t < m; t += blockDim.x) z[n + t] = ub[k * m + t];
        __syncthreads();
        for (int i = threadIdx.x; i < H; i += blockDim.x) {
            double s = 0.0;
            for (int c = 0; c < nin; ++c) s += p.W_in[(size_t)c * H + i] * z[c];
            y[i] = s;
        }
        __syncthreads();
        for (int l = 0; l < p.L; ++l) {
            const double* W = p.W_h + (size_t)l * H * H;
            const double* b = p.b_h + (size_t)l * H;
            for (int i = threadIdx.x; i < H; i += blockDim.x) {
                double s = b[i];
                for (int j = 0; j < H; ++j) s += W[(size_t)j * H + i] * y[j];
                double val, der;
                fnn_act(p.act, s, val, der);
                yn[i] = val;   // (PolyNet: p)
            }
            __syncthreads();
            if constexpr (NET == NET_POLYNET) {   // y' = y + p + act(W p + b): thread i reads p, writes its own y_i
                for (int i = threadIdx.x; i < H; i += blockDim.x) {
                    double s = b[i];
                    for (int j = 0; j < H; ++j) s += W[(size_t)j * H + i] * yn[j];
                    double val, der;
                    fnn_act(p.act, s, val, der);
                    y[i] = y[i] + yn[i] + val;
                }
            } else {
                for (int i = threadIdx.x; i < H; i += blockDim.x) {
                    if constexpr (NET == NET_RESNET) y[i] = y[i] + yn[i];
                    else y[i] = yn[i];
                }
            }
            __syncthreads();
        }
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            double s = 0.0;
            for (int j = 0; j < H; ++j) s += p.W_out[(size_t)j * n + i] * y[j];
            z[i] = s;
            xb[(size_t)(k + 1) * n + i] = s;
        }
        __syncthreads();
    }
}

}  // namespace almpc
