// almpc_sens.hip.h -- k_sens: sensitivities of the returned solution to the measured state x0, per instance, after a step.
//
// Notation of DESIGN.md section 1: scaled QP  min 1/2 w'H'w + f''w,  lo <= w <= hi,  f' = F' e0 + fS,  e0 = x0 - x_ref[:,1],
// v = d o w,  u = v + u_ref.  W = the rows of the returned u that sit at a bound (rule below).  On the face where those rows are
// held, with G = H'^-1, V = -G F' and S = G[W,W] (a principal block of an SPD matrix):
//     dw/dx0 = V - G[:,W] S^-1 V[W,:]          (nz x n; the rows W are zero)
//     du/dx0 = diag(d) dw/dx0                  (dU; K0 = its first m rows)
//     dx[:,1]/dx0 = I,  dx[:,k+1]/dx0 = A dx[:,k]/dx0 + B du[:,k]/dx0        (dX: k_sens_dx)
// and for a loss with gradients g_u [N][m], g_x [N+1][n] the vector-Jacobian product without any Jacobian:
//     lam_{N+1} = g_x[N+1],  lam_k = A'lam_{k+1} + g_x[k],   p = d o (g_u + [B'lam_2; ...; B'lam_{N+1}])  (zero on the rows W),
//     g_x0 = lam_1 + V'p - V[W,:]' S^-1 (G[W,:] p).
// The input-rate weight enters H and the constant fS only, so it changes nothing here.
//
// Active-set rule: row j = (stage k, input i) is in W iff  u[i,k] - umin_i <= tau d_j  or  umax_i - u[i,k] <= tau d_j  (d_j the row's
// Jacobi scale; exact equality would miss a bound by an ulp: u = d ((umin - u_ref) / d) + u_ref).  The test is on the returned u.  At a
// weakly active row (multiplier zero) the solution map is only directionally differentiable: what comes out is the derivative of the
// face on which every row at its bound is held.
//
// Shape: two tiers, as k_polish_gen / k_polish_gen64.  k_sens<VJP, false, ROWS>: one wave per instance, SENS_WAVES waves per workgroup
// that never wait for each other, S up to 32 x 32 in LDS; an instance with more rows is appended to a list (count word + indices).
// k_sens<VJP, true, ROWS>: one workgroup of 256 threads per listed instance, S up to nz x nz in LDS; its grid strides over the list, so an
// empty list returns at once.  Both run the same body on a "team" (64 lanes and wave fences, or 256 threads and barriers):
//   1  flags of the rows at a bound, in parallel; the row list by one thread, ascending
//   2  S = G[W,W] into LDS, Cholesky S = L L' in place (a pivot that is not positive and finite: rows = -1, outputs zero)
//   3  Jacobians: per chunk of `ch` <= 16 columns, Y = S^-1 V[W, chunk] (column-oriented substitutions on all columns at once), then
//      J = V - G[:,W] Y streamed with thread j on row j (row w of G is column w by symmetry: contiguous), scaled by d, rows W zero
//      (all nz rows for dU, the first m alone when only K0 is asked for)
//      VJP: adjoint rollout (lam in LDS), t = G[W,:] p, one solve, two n-column contractions
// Team LDS (doubles): S cap x (cap | 1), Y cap x ch, p nzs, t cap, lam 2 n; ints: list cap, flags nzs (Rs in the rows form), 4 words.
//
// Rows form (k_sens<.., .., true>; almpc_sensitivity_rows): shared designs with state rows (state box, terminal equality).  The rows
// are those of A = [I; C'] (R = nz + mc rows, padded to Rs); a state row's bound moves with x0, its value being
// (Phi e0 + Gamma D w)_r.  With Ghat = A G A' (the handle's dGhat, [R][Rs]; its first nz rows are G A') and the row values of the
// unconstrained minimiser  T1 = A V + [0; Phi_rows]  (R x n, kept as [n][Rs]: k_sens_rows_table), on the face where W is held
//     S = Ghat[W,W],   dw/dx0 = T1[0:nz] - Ghat[0:nz, W] S^-1 T1[W],
//     g_x0 = lam_1 + T1[0:nz]' p - T1[W]' S^-1 (Ghat[W, 0:nz] p)
// -- the body above with row r of Ghat (stride Rs) in place of G's and T1 in place of V; with an input box alone it is the same
// formula.  W: input rows by the rule above; a state-box row (stage k >= 2, state i) iff  x[i,k] - xmin_i <= tau_x max(1, |xmin_i|)
// or  xmax_i - x[i,k] <= tau_x max(1, |xmax_i|)  on the returned x (a bound that is not finite or at least 1e300 in size -- the
// handle's "no box" filler -- is never active); every terminal-equality row, always.  Where the handle's Ghat is the one projected on
// the terminal equality E (eq_proj) the same formula holds in projected quantities: the list is W' = W \ E, Ghat as stored, T1
// projected by the table kernel; `rows` still reports |W|.  A working set of more than nz rows (nz - n projected) cannot be
// independent: rows = -1 and zeros, as for a failed Cholesky.
//
// Parameter gradients (almpc_sensitivity_params_vjp: k_sens_pz, then k_sens_params): the same loss, differentiated in the problem data
// on the face where W is held.  Stages 1-based, v = e_u, e_x[:,1] = e0, sym(a, b) = a b' + b a', Qbar_1 = 0, Qbar_k = Q (k = 2..N),
// Qbar_{N+1} = P.  With q_k = g_u[:,k] + B'lam_{k+1} (all rows, unscaled):
//     z_W = 0,  z_F = -H_FF^-1 q_F;   nu_j = q_j + (H z)_j on the rows of W, 0 elsewhere (the gradient in the bound the row sits at)
// On the device, from the VJP's factor:  p = d o q (p_W = 0),  t = S^-1 G[W,:] p,  z = -d o (G p - G[:,W] t) (rows W written as zeros),
// nu_j = q_j + t_a / d_j for j = W[a] -- k_sens_pz = the VJP body plus the product G p (thread j on row j of G, read as column j).
//     zeta_1 = 0,  zeta_{k+1} = A zeta_k + B z_k                                     (the step's rollout from (0, z))
//     mu_{N+1} = g_x[N+1] + 2 P zeta_{N+1},   mu_k = A'mu_{k+1} + g_x[k] + 2 Qbar_k zeta_k
//     al_{N+1} = 2 P e_x[:,N+1],              al_k = A'al_{k+1} + 2 Qbar_k e_x[:,k]
//     dL/dx0 = mu_1 = lam_1 + F'z (handed out by the VJP's own expression: the bits of almpc_sensitivity_vjp),   dL/df = z
//     dL/dQ = sum_{k=2..N} sym(zeta_k, e_x[:,k]),  dL/dP = sym(zeta_{N+1}, e_x[:,N+1]),  dL/dR = sum_{k=1..N} sym(z_k, v_k)
//     dL/dS = sum_{k=1..N-1} sym(z_k - z_{k+1}, u_k - u_{k+1})                        (the rate cost is on u, not on e_u)
//     dL/dA = sum_{k=1..N} mu_{k+1} e_x[:,k]' + al_{k+1} zeta_k',   dL/dB = sum_{k=1..N} mu_{k+1} v_k' + al_{k+1} z_k'
//     dL/du_ref[:,k] = g_u[:,k] - nu_k + 2 S (z_k - z_{k+1}) - 2 S (z_{k-1} - z_k)    (S terms only where S is in the design; the
//                                                                                     differences z_0 - z_1, z_N - z_{N+1} are absent)
//     dL/dumin_i = sum_k nu_(k,i) over the rows at the lower bound, dL/dumax_i over those at the upper (at both: lower)
// Conventions: a symmetric matrix gradient G_Q is the symmetric matrix with dL = sum_ij (G_Q)_ij dQ_ij for symmetric dQ.  P is data,
// also where the design computed it as a DARE: its dependence on A, B, Q, R is followed behind these kernels, by k_dare_vjp
// (csrc/almpc_dare_vjp.hip.h, almpc_sensitivity_params_vjp_dare), from the P group they write.  Where the design dropped R or S (the
// reference's [1,1] rule, src/sub/design_mpc.jl:423-456) that gradient is zero.  x_ref needs no output:
// dL/dx_ref[:,1] = g_x[1] - dL/dx0 and dL/dx_ref[:,k] = g_x[k] for k >= 2.  Weakly active rows: as above, the derivative of the face on
// which every flagged row is held.  Every sum runs in ascending stage order in one thread: the same bits wherever the instance sits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace almpc {

constexpr int SENS_WAVES = 4;
constexpr int SENS_CAP1 = 32;       // rows of the first tier
constexpr int SENS_WG = 256;        // threads of a second-tier workgroup
constexpr int SENS_OVF_HEAD = 4;    // ints in front of the overflow list: [0] the count (a 16-byte block, zeroed before every call)
constexpr unsigned SENS_K0 = 1u, SENS_DU = 2u, SENS_DX = 4u;   // ALMPC_SENS_*

struct SensParams {
    int n, m, N, nz, nzs, batch;
    const double* G; long G_stride;     // [nz][nzs] symmetric (stride 0: shared)
    const double* V; long V_stride;     // [n][nzs] plain, V[r, c] at c * nzs + r
    const double* d; long d_stride;     // [nzs]
    const double* A; long A_stride;     // n x n column-major (VJP)
    const double* B; long B_stride;     // n x m
    const double* umin; const double* umax;   // [m]
    const double* u;                    // [batch][nz] returned inputs
    const int32_t* status;              // [batch] almpc_solve_status of the step
    double tau;
    int cap, ch;                        // row capacity of this tier (SENS_CAP1 or nz), column chunk (a multiple of 4, <= 16)
    int lds_per_team;                   // doubles
    unsigned want;                      // SENS_* (Jacobian mode)
    double* K0; double* dU;             // [batch][n][m], [batch][n][nz]
    const double* g_u; const double* g_x;   // [batch][nz], [batch][N+1][n] or null (VJP mode)
    double* g_x0;                       // [batch][n]
    int32_t* rows;                      // [batch] |W|, or -1
    int32_t* ovf;                       // [SENS_OVF_HEAD + batch]
    // rows form: G is Ghat [R][Rs], V is T1 [n][Rs]
    int R, Rs;                          // rows of A, padded
    int cap2;                           // most rows an independent working set can hold (nz, or nz - ne projected)
    int eq_proj, eq0, ne;               // Ghat and T1 are projected on the rows eq0 .. eq0 + ne - 1
    const double* x;                    // [batch][N+1][n] returned states
    const double* xmin; const double* xmax;          // [n]
    const int* row_xidx; const int* row_eq;          // [Rs] a state row's place in x, whether it is an equality row
    double tau_x;
    // parameter gradients (k_sens_pz): z = dL/df and nu [batch][nz], the bound gradients [batch][m]
    double* z; double* nu; double* gmin; double* gmax;
};

__host__ __device__ inline int sens_ch(int n) { const int c = (n + 3) & ~3; return c < 16 ? c : 16; }
// (nfl: rows that carry a flag -- nzs, or Rs in the rows form)
__host__ __device__ inline int sens_lds_doubles(int n, int nzs, int cap, int nfl) {
    const int ints = cap + nfl + 4;
    return (cap * (cap | 1) + cap * sens_ch(n) + nzs + cap + 2 * n + (ints + 1) / 2 + 1) & ~1;
}

// k_sens_pz keeps q on the rows of W (then nu) behind the VJP's team LDS
__host__ __device__ inline int sens_pz_lds_doubles(int n, int nzs, int cap) { return sens_lds_doubles(n, nzs, cap, nzs) + ((nzs + 1) & ~1); }

template <bool WG>
struct SensTeam {
    int tid, nt;
    __device__ __forceinline__ void sync() const {
        if (WG) __syncthreads();
        else {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
};

// X <- S^-1 X for the Cholesky factor L of S (lower triangle of Sl, leading dimension ld): X rows x nc, element (a, c) at a * ldx + c.
// Column-oriented: row k is divided, then taken out of every row behind (in front) of it -- all columns and rows in parallel.
template <bool WG>
__device__ __forceinline__ void sens_solve(const SensTeam<WG>& T, const double* Sl, int ld, int rows, double* X, int ldx, int nc) {
    for (int k = 0; k < rows; ++k) {
        const double dk = Sl[k * ld + k];
        for (int c = T.tid; c < nc; c += T.nt) X[k * ldx + c] /= dk;
        T.sync();
        const int cnt = (rows - k - 1) * nc;
        for (int idx = T.tid; idx < cnt; idx += T.nt) {
            const int i = k + 1 + idx / nc, c = idx % nc;
            X[i * ldx + c] -= Sl[i * ld + k] * X[k * ldx + c];
        }
        T.sync();
    }
    for (int k = rows - 1; k >= 0; --k) {
        const double dk = Sl[k * ld + k];
        for (int c = T.tid; c < nc; c += T.nt) X[k * ldx + c] /= dk;
        T.sync();
        const int cnt = k * nc;
        for (int idx = T.tid; idx < cnt; idx += T.nt) {
            const int i = idx / nc, c = idx % nc;
            X[i * ldx + c] -= Sl[k * ld + i] * X[k * ldx + c];
        }
        T.sync();
    }
}

template <bool VJP, bool WG>
__device__ __forceinline__ void sens_zero(const SensParams& p, const SensTeam<WG>& T, int inst) {
    const int n = p.n, m = p.m, nz = p.nz;
    if (VJP) {
        for (int c = T.tid; c < n; c += T.nt) p.g_x0[(size_t)inst * n + c] = 0.0;
    } else {
        if (p.want & SENS_K0)
            for (int t = T.tid; t < n * m; t += T.nt) p.K0[(size_t)inst * n * m + t] = 0.0;
        if (p.want & (SENS_DU | SENS_DX))
            for (int t = T.tid; t < n * nz; t += T.nt) p.dU[(size_t)inst * n * nz + t] = 0.0;
    }
}

template <bool WG>
__device__ __forceinline__ void sens_zero_pz(const SensParams& p, const SensTeam<WG>& T, int inst) {
    for (int j = T.tid; j < p.nz; j += T.nt) { p.z[(size_t)inst * p.nz + j] = 0.0; p.nu[(size_t)inst * p.nz + j] = 0.0; }
    for (int i = T.tid; i < p.m; i += T.nt) { p.gmin[(size_t)inst * p.m + i] = 0.0; p.gmax[(size_t)inst * p.m + i] = 0.0; }
}

// (PAR: the VJP with z, nu and the bound gradients behind it -- k_sens_pz; no rows form)
template <bool VJP, bool WG, bool ROWS, bool PAR = false>
__device__ __forceinline__ void sens_instance(const SensParams& p, const SensTeam<WG>& T, int inst, double* L) {
    static_assert(!PAR || (VJP && !ROWS), "the parameter gradients extend the VJP of the input-box form");
    const int n = p.n, m = p.m, N = p.N, nz = p.nz, nzs = p.nzs, cap = p.cap, ch = p.ch, ld = cap | 1;
    const int gs = ROWS ? p.Rs : nzs;   // stride of a row of G (Ghat) and of a column of V (T1); the rows that carry a flag
    double* S = L;
    double* Y = S + cap * ld;
    double* pv = Y + cap * ch;
    double* tv = pv + nzs;
    double* lam = tv + cap;
    int* wl = reinterpret_cast<int*>(lam + 2 * n);
    int* act = wl + cap;
    int* word = act + gs;   // [0] rows in the list, [1] the factorisation failed
    const double* G = p.G + (size_t)inst * p.G_stride;
    const double* V = p.V + (size_t)inst * p.V_stride;
    const double* dv = p.d + (size_t)inst * p.d_stride;

    T.sync();   // (the previous instance of this team has read its last LDS operand)
    // 1: the rows at a bound
    if (!WG && p.status[inst] != 0) {   // (the second tier only gets solved instances)
        sens_zero<VJP>(p, T, inst);
        if (PAR) sens_zero_pz(p, T, inst);
        if (T.tid == 0) p.rows[inst] = -1;
        return;
    }
    for (int j = T.tid; j < nz; j += T.nt) {
        const double uj = p.u[(size_t)inst * nz + j], tol = p.tau * dv[j];
        const int i = j % m;
        act[j] = (uj - p.umin[i] <= tol || p.umax[i] - uj <= tol) ? 1 : 0;
    }
    if (ROWS) {
        const double* xs = p.x + (size_t)inst * (N + 1) * n;
        for (int r = nz + T.tid; r < p.R; r += T.nt) {
            int f = 1;   // (an equality row)
            if (!p.row_eq[r]) {
                const int xi = p.row_xidx[r];
                const double xv = xs[xi], lo = p.xmin[xi % n], hi = p.xmax[xi % n];
                // (fabs(b) < 1e300 is false for an infinite bound, for NaN and for the "no box" filler)
                f = ((fabs(lo) < 1e300 && xv - lo <= p.tau_x * fmax(1.0, fabs(lo))) ||
                     (fabs(hi) < 1e300 && hi - xv <= p.tau_x * fmax(1.0, fabs(hi)))) ? 1 : 0;
            }
            act[r] = f;
        }
    }
    T.sync();
    const int held = (ROWS && p.eq_proj) ? p.ne : 0;   // rows of W that the projection took out of the problem
    if (T.tid == 0) {
        int r = 0;
        const int nrows = ROWS ? p.R : nz;
        for (int j = 0; j < nrows; ++j) {
            if (ROWS && held && j >= p.eq0 && j < p.eq0 + p.ne) continue;
            if (act[j]) { if (r < cap) wl[r] = j; ++r; }
        }
        word[0] = r; word[1] = 0;
    }
    T.sync();
    const int rows = word[0];
    if (ROWS && rows > p.cap2) {   // more rows than free directions: not independent
        sens_zero<VJP>(p, T, inst);
        if (PAR) sens_zero_pz(p, T, inst);
        if (T.tid == 0) p.rows[inst] = -1;
        return;
    }
    if (rows > cap) {   // first tier only (the second has cap = nz, cap2 in the rows form): hand the instance on
        if (T.tid == 0) {
            const int k = atomicAdd(p.ovf, 1);
            p.ovf[SENS_OVF_HEAD + k] = inst;
        }
        return;
    }
    // 2: S = G[W,W] = L L'
    for (int idx = T.tid; idx < rows * rows; idx += T.nt) {
        const int a = idx / rows, b = idx % rows;
        S[a * ld + b] = G[(size_t)wl[a] * gs + wl[b]];
    }
    T.sync();
    for (int k = 0; k < rows; ++k) {
        if (T.tid == 0) {
            const double piv = S[k * ld + k];
            if (!(piv > 0.0 && piv <= 1.7976931348623157e308)) word[1] = 1;
            S[k * ld + k] = sqrt(piv);
        }
        T.sync();
        if (word[1]) break;   // (the same word for the whole team)
        const double dk = S[k * ld + k];
        for (int i = k + 1 + T.tid; i < rows; i += T.nt) S[i * ld + k] /= dk;
        T.sync();
        const int rem = rows - k - 1;
        for (int idx = T.tid; idx < rem * rem; idx += T.nt) {
            const int i = k + 1 + idx / rem, j = k + 1 + idx % rem;
            if (j <= i) S[i * ld + j] -= S[i * ld + k] * S[j * ld + k];
        }
        T.sync();
    }
    if (word[1]) {
        sens_zero<VJP>(p, T, inst);
        if (PAR) sens_zero_pz(p, T, inst);
        if (T.tid == 0) p.rows[inst] = -1;
        return;
    }
    if (T.tid == 0) p.rows[inst] = rows + held;

    if (!VJP) {
        // 3: per column chunk Y = S^-1 V[W, chunk], then J = V - G[:,W] Y, scaled (K0 alone: only its m rows of J)
        const int jrows = (p.want & (SENS_DU | SENS_DX)) ? nz : m;
        for (int c0 = 0; c0 < n; c0 += ch) {
            const int nc = n - c0 < ch ? n - c0 : ch;
            for (int idx = T.tid; idx < rows * nc; idx += T.nt) {
                const int a = idx / nc, c = idx % nc;
                Y[a * ch + c] = V[(size_t)(c0 + c) * gs + wl[a]];
            }
            T.sync();
            sens_solve(T, S, ld, rows, Y, ch, nc);
            for (int j = T.tid; j < jrows; j += T.nt) {
                const double dj = dv[j];
                const bool aj = act[j] != 0;
                for (int q0 = 0; q0 < nc; q0 += 4) {   // (ch is a multiple of 4: columns past nc are read inside Y's row and dropped)
                    double acc[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q] = q0 + q < nc ? V[(size_t)(c0 + q0 + q) * gs + j] : 0.0;
                    for (int a = 0; a < rows; ++a) {
                        const double g = G[(size_t)wl[a] * gs + j];
                        const double* y = Y + a * ch + q0;
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[q] -= g * y[q];
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int c = c0 + q0 + q;
                        if (q0 + q < nc) {
                            const double val = aj ? 0.0 : dj * acc[q];
                            if (p.want & (SENS_DU | SENS_DX)) p.dU[((size_t)inst * n + c) * nz + j] = val;
                            if ((p.want & SENS_K0) && j < m) p.K0[((size_t)inst * n + c) * m + j] = val;
                        }
                    }
                }
            }
            T.sync();   // (Y is gathered again)
        }
    } else {
        const double* A = p.A + (size_t)inst * p.A_stride;
        const double* B = p.B + (size_t)inst * p.B_stride;
        const double* gu = p.g_u + (size_t)inst * nz;
        const double* gx = p.g_x ? p.g_x + (size_t)inst * (N + 1) * n : nullptr;
        double* cur = lam;
        double* nxt = lam + n;
        double* qv = L + sens_lds_doubles(n, nzs, cap, nzs);   // (PAR) q on the rows of W, zero elsewhere
        // (0.0 is added where g_x is null, so that a null g_x and a g_x of zeros give the same bits)
        for (int i = T.tid; i < n; i += T.nt) cur[i] = 0.0 + (gx ? gx[(size_t)N * n + i] : 0.0);
        T.sync();
        for (int k = N - 1; k >= 0; --k) {   // cur = lam of state stage k + 1 (0-based): the one input stage k acts on
            for (int a = T.tid; a < m; a += T.nt) {
                double s = 0.0;
                for (int i = 0; i < n; ++i) s += B[i + a * n] * cur[i];
                const int j = k * m + a;
                pv[j] = act[j] ? 0.0 : dv[j] * (gu[j] + s);
                if (PAR) qv[j] = act[j] ? gu[j] + s : 0.0;
            }
            for (int i = T.tid; i < n; i += T.nt) {
                double s = 0.0;
                for (int l = 0; l < n; ++l) s += A[l + i * n] * cur[l];
                nxt[i] = s + (gx ? gx[(size_t)k * n + i] : 0.0);
            }
            T.sync();
            double* t_ = cur; cur = nxt; nxt = t_;
        }
        for (int a = T.tid; a < rows; a += T.nt) {
            const double* g = G + (size_t)wl[a] * gs;
            double s = 0.0;
            for (int j = 0; j < nz; ++j) s += g[j] * pv[j];
            tv[a] = s;
        }
        T.sync();
        sens_solve(T, S, ld, rows, tv, 1, 1);
        for (int c = T.tid; c < n; c += T.nt) {
            const double* v = V + (size_t)c * gs;
            double s1 = 0.0, s2 = 0.0;
            for (int j = 0; j < nz; ++j) s1 += v[j] * pv[j];
            for (int a = 0; a < rows; ++a) s2 += v[wl[a]] * tv[a];
            p.g_x0[(size_t)inst * n + c] = cur[c] + s1 - s2;
        }
        if (PAR) {
            for (int a = T.tid; a < rows; a += T.nt) qv[wl[a]] += tv[a] / dv[wl[a]];   // nu
            T.sync();
            for (int j = T.tid; j < nz; j += T.nt) {   // row j of G p - G[:,W] t, read as column j: contiguous across the team
                double s = 0.0;
                for (int i = 0; i < nz; ++i) s += G[(size_t)i * gs + j] * pv[i];
                for (int a = 0; a < rows; ++a) s -= G[(size_t)wl[a] * gs + j] * tv[a];
                p.z[(size_t)inst * nz + j] = act[j] ? 0.0 : -dv[j] * s;
                p.nu[(size_t)inst * nz + j] = qv[j];
            }
            for (int i = T.tid; i < m; i += T.nt) {   // ascending stages; a row at both bounds counts as lower
                double lo = 0.0, hi = 0.0;
                for (int k = 0; k < N; ++k) {
                    const int j = k * m + i;
                    if (!act[j]) continue;
                    if (p.u[(size_t)inst * nz + j] - p.umin[i] <= p.tau * dv[j]) lo += qv[j];
                    else hi += qv[j];
                }
                p.gmin[(size_t)inst * m + i] = lo; p.gmax[(size_t)inst * m + i] = hi;
            }
        }
    }
}

template <bool VJP, bool WG, bool ROWS>
__global__ __launch_bounds__(256) void k_sens(SensParams p) {
    extern __shared__ __attribute__((aligned(16))) double sens_smem[];
    if (WG) {
        const SensTeam<WG> T{(int)threadIdx.x, (int)blockDim.x};
        const int count = p.ovf[0];
        for (int k = blockIdx.x; k < count; k += gridDim.x) sens_instance<VJP, WG, ROWS>(p, T, p.ovf[SENS_OVF_HEAD + k], sens_smem);
    } else {
        const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        const SensTeam<WG> T{(int)(threadIdx.x & 63), 64};
        double* L = sens_smem + (size_t)wv * p.lds_per_team;
        const int wpb = (int)(blockDim.x >> 6), nwaves = gridDim.x * wpb;
        for (int inst = blockIdx.x * wpb + wv; inst < p.batch; inst += nwaves) sens_instance<VJP, WG, ROWS>(p, T, inst, L);
    }
}

// The VJP with z, nu and the bound gradients behind it (almpc_sensitivity_params_vjp): k_sens's grid, both tiers
template <bool WG>
__global__ __launch_bounds__(256) void k_sens_pz(SensParams p) {
    extern __shared__ __attribute__((aligned(16))) double sens_pz_smem[];
    if (WG) {
        const SensTeam<WG> T{(int)threadIdx.x, (int)blockDim.x};
        const int count = p.ovf[0];
        for (int k = blockIdx.x; k < count; k += gridDim.x) sens_instance<true, WG, false, true>(p, T, p.ovf[SENS_OVF_HEAD + k], sens_pz_smem);
    } else {
        const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        const SensTeam<WG> T{(int)(threadIdx.x & 63), 64};
        double* L = sens_pz_smem + (size_t)wv * p.lds_per_team;
        const int wpb = (int)(blockDim.x >> 6), nwaves = gridDim.x * wpb;
        for (int inst = blockIdx.x * wpb + wv; inst < p.batch; inst += nwaves) sens_instance<true, WG, false, true>(p, T, inst, L);
    }
}

// Stage recursions and outer-product sums of the parameter gradients, behind k_sens_pz on the same stream.  One workgroup per
// instance (grid-stride); stage vectors in LDS (6 n doubles), the trajectories zeta, mu, al in the workgroup's slice of a scratch
// buffer ([grid][3][(N+1) n]: written and read by this workgroup alone, a barrier in between).  Then every output entry is one
// thread's sum over the stages, ascending, in one register.  Q, P, S are read as M + M' (twice their symmetric part).
// Outputs column-major per instance: Q, P, A n x n, B n x m, R, S m x m; u_ref [N][m].  rows < 0: zeros.
struct SensGradParams {
    int n, m, N, nz, batch, useR, useS;
    const double* A; long A_stride;
    const double* B; long B_stride;
    const double* Q; const double* S;           // [n][n], [m][m]: the design's weights, shared (strides 0) or one pair per instance
    long Q_stride = 0, S_stride = 0;
    const double* P; long P_stride;
    const double* ex; const double* ev; const double* u;   // the step's e_x [batch][N+1][n], e_u and u [batch][nz]
    const double* g_u; const double* g_x;       // as k_sens (g_x may be null)
    const double* z; const double* nu;          // [batch][nz] from k_sens_pz
    const int32_t* rows;
    double* traj;
    double *gur, *gQ, *gP, *gA, *gR, *gS, *gB;  // null where not wanted
};
__host__ __device__ inline int sens_grad_lds_doubles(int n) { return 6 * n; }

inline __global__ __launch_bounds__(256) void k_sens_params(SensGradParams p) {
    extern __shared__ __attribute__((aligned(16))) double sens_grad_smem[];
    const int n = p.n, m = p.m, N = p.N, nz = p.nz, tid = threadIdx.x, nt = blockDim.x, xs = (N + 1) * n;
    double* zc = sens_grad_smem;
    double* zn = zc + n;
    double* cur = zn + n;       // [mu | al]
    double* nxt = cur + 2 * n;
    double* Zt = p.traj + (size_t)blockIdx.x * 3 * xs;
    double* Mt = Zt + xs;
    double* At = Mt + xs;
    const int oP = n * n, oA = 2 * n * n, oB = 3 * n * n, oR = oB + n * m, oS = oR + m * m, oU = oS + m * m, total = oU + nz;
    for (int inst = blockIdx.x; inst < p.batch; inst += gridDim.x) {
        const bool ok = p.rows[inst] >= 0;   // (one word for the whole workgroup)
        const double* A = p.A + (size_t)inst * p.A_stride;
        const double* B = p.B + (size_t)inst * p.B_stride;
        const double* P = p.P + (size_t)inst * p.P_stride;
        const double* Q = p.Q + (size_t)inst * p.Q_stride;
        const double* S = p.S + (size_t)inst * p.S_stride;
        const double* ex = p.ex + (size_t)inst * xs;
        const double* ev = p.ev + (size_t)inst * nz;
        const double* u = p.u + (size_t)inst * nz;
        const double* z = p.z + (size_t)inst * nz;
        const double* gx = p.g_x ? p.g_x + (size_t)inst * xs : nullptr;
        __syncthreads();   // (the previous instance's sums have read the trajectories and the stage vectors)
        if (ok) {
            for (int i = tid; i < n; i += nt) { zc[i] = 0.0; Zt[i] = 0.0; }
            __syncthreads();
            for (int k = 0; k < N; ++k) {
                for (int i = tid; i < n; i += nt) {
                    double s = 0.0;
                    for (int l = 0; l < n; ++l) s += A[i + l * n] * zc[l];
                    for (int a = 0; a < m; ++a) s += B[i + a * n] * z[k * m + a];
                    zn[i] = s; Zt[(k + 1) * n + i] = s;
                }
                __syncthreads();
                double* t_ = zc; zc = zn; zn = t_;
            }
            for (int t = tid; t < 2 * n; t += nt) {   // mu_{N+1}, al_{N+1}
                const int i = t % n, al = t / n;
                const double* src = al ? ex + (size_t)N * n : zc;
                double s = 0.0;
                for (int l = 0; l < n; ++l) s += (P[i + l * n] + P[l + i * n]) * src[l];
                if (!al) s += gx ? gx[(size_t)N * n + i] : 0.0;
                cur[t] = s; (al ? At : Mt)[N * n + i] = s;
            }
            __syncthreads();
            for (int k = N - 1; k >= 1; --k) {   // (stage 1 of mu is dL/dx0, which the VJP body hands out; al_1 is not used)
                for (int t = tid; t < 2 * n; t += nt) {
                    const int i = t % n, al = t / n;
                    const double* c = cur + al * n;
                    const double* src = al ? ex + (size_t)k * n : Zt + (size_t)k * n;
                    double s = 0.0, w = 0.0;
                    for (int l = 0; l < n; ++l) s += A[l + i * n] * c[l];
                    for (int l = 0; l < n; ++l) w += (Q[i + l * n] + Q[l + i * n]) * src[l];
                    if (!al) s += gx ? gx[(size_t)k * n + i] : 0.0;
                    s += w;
                    nxt[t] = s; (al ? At : Mt)[k * n + i] = s;
                }
                __syncthreads();
                double* t_ = cur; cur = nxt; nxt = t_;
            }
        }
        for (int e = tid; e < total; e += nt) {
            double s = 0.0;
            if (e < oP) {
                if (!p.gQ) continue;
                const int i = e % n, j = e / n;
                if (ok) for (int k = 1; k < N; ++k) s += Zt[k * n + i] * ex[k * n + j] + ex[k * n + i] * Zt[k * n + j];
                p.gQ[(size_t)inst * n * n + e] = s;
            } else if (e < oA) {
                if (!p.gP) continue;
                const int i = (e - oP) % n, j = (e - oP) / n;
                if (ok) s = Zt[N * n + i] * ex[N * n + j] + ex[N * n + i] * Zt[N * n + j];
                p.gP[(size_t)inst * n * n + (e - oP)] = s;
            } else if (e < oB) {
                if (!p.gA) continue;
                const int i = (e - oA) % n, j = (e - oA) / n;
                if (ok) for (int k = 0; k < N; ++k) s += Mt[(k + 1) * n + i] * ex[k * n + j] + At[(k + 1) * n + i] * Zt[k * n + j];
                p.gA[(size_t)inst * n * n + (e - oA)] = s;
            } else if (e < oR) {
                if (!p.gB) continue;
                const int i = (e - oB) % n, a = (e - oB) / n;
                if (ok) for (int k = 0; k < N; ++k) s += Mt[(k + 1) * n + i] * ev[k * m + a] + At[(k + 1) * n + i] * z[k * m + a];
                p.gB[(size_t)inst * n * m + (e - oB)] = s;
            } else if (e < oS) {
                if (!p.gR) continue;
                const int a = (e - oR) % m, b = (e - oR) / m;
                if (ok && p.useR) for (int k = 0; k < N; ++k) s += z[k * m + a] * ev[k * m + b] + ev[k * m + a] * z[k * m + b];
                p.gR[(size_t)inst * m * m + (e - oR)] = s;
            } else if (e < oU) {
                if (!p.gS) continue;
                const int a = (e - oS) % m, b = (e - oS) / m;
                if (ok && p.useS)
                    for (int k = 0; k + 1 < N; ++k) {
                        const double dza = z[k * m + a] - z[(k + 1) * m + a], dzb = z[k * m + b] - z[(k + 1) * m + b];
                        const double dua = u[k * m + a] - u[(k + 1) * m + a], dub = u[k * m + b] - u[(k + 1) * m + b];
                        s += dza * dub + dua * dzb;
                    }
                p.gS[(size_t)inst * m * m + (e - oS)] = s;
            } else {
                if (!p.gur) continue;
                const int j = e - oU, k = j / m, a = j % m;
                if (ok) {
                    s = p.g_u[(size_t)inst * nz + j] - p.nu[(size_t)inst * nz + j];
                    if (p.useS) {
                        double w = 0.0;
                        for (int b = 0; b < m; ++b) {
                            const double sab = S[a + b * m] + S[b + a * m];
                            if (k + 1 < N) w += sab * (z[k * m + b] - z[(k + 1) * m + b]);
                            if (k > 0) w -= sab * (z[(k - 1) * m + b] - z[k * m + b]);
                        }
                        s += w;
                    }
                }
                p.gur[(size_t)inst * nz + j] = s;
            }
        }
    }
}

// dX from dU: the step's rollout with n right-hand sides.  One workgroup per instance; A, B and two n x n stages in LDS.
// dX [batch][n][N+1][n]: element (state i, stage k, column c) at ((c (N+1)) + k) n + i.  rows < 0: zeros.
struct SensDxParams {
    int n, m, N, nz, batch;
    const double* A; long A_stride;
    const double* B; long B_stride;
    const double* dU;        // [batch][n][nz]
    const int32_t* rows;     // [batch]
    double* dX;
};
__host__ __device__ inline int sens_dx_lds_doubles(int n, int m) { return 3 * n * n + n * m; }

inline __global__ __launch_bounds__(256) void k_sens_dx(SensDxParams p) {
    extern __shared__ __attribute__((aligned(16))) double sens_dx_smem[];
    const int n = p.n, m = p.m, N = p.N, nz = p.nz, tid = threadIdx.x, nt = blockDim.x;
    double* Al = sens_dx_smem;
    double* Bl = Al + n * n;
    double* cur = Bl + n * m;
    double* nxt = cur + n * n;
    for (int inst = blockIdx.x; inst < p.batch; inst += gridDim.x) {
        double* out = p.dX + (size_t)inst * n * (N + 1) * n;
        __syncthreads();
        if (p.rows[inst] < 0) {   // (one word for the whole workgroup)
            for (int t = tid; t < n * (N + 1) * n; t += nt) out[t] = 0.0;
            continue;
        }
        const double* A = p.A + (size_t)inst * p.A_stride;
        const double* B = p.B + (size_t)inst * p.B_stride;
        const double* dU = p.dU + (size_t)inst * n * nz;
        for (int t = tid; t < n * n; t += nt) {
            Al[t] = A[t];
            const double e = (t % n == t / n) ? 1.0 : 0.0;
            cur[t] = e;
            out[(size_t)(t / n) * (N + 1) * n + t % n] = e;
        }
        for (int t = tid; t < n * m; t += nt) Bl[t] = B[t];
        __syncthreads();
        for (int k = 0; k < N; ++k) {
            for (int t = tid; t < n * n; t += nt) {
                const int i = t % n, c = t / n;
                double s = 0.0;
                for (int l = 0; l < n; ++l) s += Al[i + l * n] * cur[l + c * n];
                const double* du = dU + (size_t)c * nz + (size_t)k * m;
                for (int a = 0; a < m; ++a) s += Bl[i + a * n] * du[a];
                nxt[t] = s;
                out[((size_t)c * (N + 1) + k + 1) * n + i] = s;
            }
            __syncthreads();
            double* t_ = cur; cur = nxt; nxt = t_;
        }
    }
}

// Plain V [n][nzs] (zero pad rows) from the MFMA fragment order a shared design keeps it in (k_pack_frags):
// frag[(rb * ksf + s) * 64 + l] = V[16 rb + (l & 15)][4 s + (l >> 4)]
inline __global__ __launch_bounds__(256) void k_sens_unpack_v(const double* frag, int nz, int n, int nzs, int ksf, double* out) {
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n * nzs; t += gridDim.x * blockDim.x) {
        const int r = t % nzs, c = t / nzs;
        out[t] = r < nz ? frag[((size_t)(r >> 4) * ksf + (c >> 2)) * 64 + (((c & 3) << 4) | (r & 15))] : 0.0;
    }
}

// Design-time table of the rows form: T1 = A V + [0; Phi_rows] as [n][Rs] (zero pad rows).  Workgroup c rolls (e0 = unit_c,
// v = d o V[:, c]) out through the shared A, B and reads the state rows where row_xidx says; the first nz entries are V[:, c].
// eq_proj: T1 - Ghat[:, E] Ghat_EE^-1 T1[E] from the rows the projection took out of Ghat (GhatE [ne][Rs]) and WinvE = Ghat_EE^-1
// ([ne][ne]); the rows E themselves exactly zero.
// The handle's V = -G F' is a product with the rounded inverse and carries cond(H') times the FP64 unit into every entry (1e-9 on the
// quadrotor: a VJP, whose terms cancel, then misses a few 1e-9 of its size).  The column is therefore refined once against the
// design's own H, F (unscaled, column-major, as almpc_get_design hands them out):  v <- v - G (D H D v + D F[:, c]),  which leaves
// what a factor-based solve gives (3.6e-11 against 4.1e-9 in the numpy restatement of this step, tests/sens_rows_ref.py).
// LDS: the trajectory [(N+1)][n], ne doubles, and the column with its residual, 2 nz.
struct SensRowsTableParams {
    int n, m, N, nz, nzs, R, Rs, eq_proj, eq0, ne;
    const double* A; const double* B; const double* V; const double* d;   // V [n][nzs] plain
    const double* H; const double* F; const double* G;                    // H [nz][nz], F [n][nz] unscaled; G [nz][nzs] = H'^-1
    const int* row_xidx;
    const double* GhatE; const double* WinvE;
    double* out;
};
__host__ __device__ inline int sens_rows_table_lds_doubles(int n, int N, int nz) { return (N + 1) * n + n + 2 * nz; }

inline __global__ __launch_bounds__(256) void k_sens_rows_table(SensRowsTableParams p) {
    extern __shared__ __attribute__((aligned(16))) double sens_tab_smem[];
    const int n = p.n, m = p.m, N = p.N, nz = p.nz, c = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    double* X = sens_tab_smem;
    double* le = X + (N + 1) * n;
    double* v = le + n;
    double* res = v + nz;
    double* o = p.out + (size_t)c * p.Rs;
    for (int j = tid; j < nz; j += nt) v[j] = p.V[(size_t)c * p.nzs + j];
    for (int i = tid; i < n; i += nt) X[i] = i == c ? 1.0 : 0.0;
    __syncthreads();
    for (int i = tid; i < nz; i += nt) {   // residual of H' v = -F'[:, c] (H is symmetric: column i is row i)
        double s = 0.0;
        for (int j = 0; j < nz; ++j) s += p.H[(size_t)i * nz + j] * (p.d[j] * v[j]);
        res[i] = p.d[i] * (s + p.F[(size_t)c * nz + i]);
    }
    __syncthreads();
    for (int i = tid; i < nz; i += nt) {
        double s = 0.0;
        for (int j = 0; j < nz; ++j) s += p.G[(size_t)i * p.nzs + j] * res[j];
        v[i] -= s;   // (every thread its own entries: nobody reads v in this loop)
    }
    __syncthreads();
    for (int k = 0; k < N; ++k) {
        for (int i = tid; i < n; i += nt) {
            double s = 0.0;
            for (int l = 0; l < n; ++l) s += p.A[i + l * n] * X[k * n + l];
            for (int a = 0; a < m; ++a) s += p.B[i + a * n] * (p.d[k * m + a] * v[k * m + a]);
            X[(k + 1) * n + i] = s;
        }
        __syncthreads();
    }
    if (p.eq_proj) {
        for (int a = tid; a < p.ne; a += nt) {
            double s = 0.0;
            for (int e = 0; e < p.ne; ++e) s += p.WinvE[a * p.ne + e] * X[p.row_xidx[p.eq0 + e]];
            le[a] = s;
        }
        __syncthreads();
    }
    for (int r = tid; r < p.Rs; r += nt) {
        double t = r < nz ? v[r] : (r < p.R ? X[p.row_xidx[r]] : 0.0);
        if (p.eq_proj && r < p.R) {
            for (int a = 0; a < p.ne; ++a) t -= p.GhatE[(size_t)a * p.Rs + r] * le[a];
            if (r >= p.eq0 && r < p.eq0 + p.ne) t = 0.0;
        }
        o[r] = t;
    }
}

// ---- k_sens_face, k_sens_face_rate: the same sensitivities on a structured handle --------
// (almpc_sensitivity_stagewise, almpc_sensitivity_stagewise_vjp; with the input-rate weight S almpc_sensitivity_stagewise_rate, .._rate_vjp)
//
// A structured handle forms no G = H'^-1, and none is needed: on the face where the rows W of the returned u are held the problem is
// an LQ problem whose clamped inputs are taken out stage by stage, and its derivative in x0 is a Riccati recursion with a masked B --
// O(N (n^3 + n^2 m)) per instance, whatever m N and the spectral radius of A.  Input box only.  Both kernels are the same sweep over a
// stage state of width w (w = n without S, w = nt = n + m with it), put together from the pieces below (sens_face_*); what a stage
// computes between them -- P+ B, the right-hand side and Lam, Acl, the Riccati update -- is each kernel's own.  Stages 0-based, W_k the
// inputs of stage k at a bound, f the free ones:
//     backward, k = N-1 .. 0:  Lam (m x m, identity on W_k) and the right-hand side (m x w, rows W_k zero) from P+   [the kernel]
//                              K_k = Lam^-1 rhs                                                                    [sens_face_gain_solve]
//                              Acl_k, and P+ <- the Riccati update (k >= 1 only: P_0 has no reader)                  [the kernel]
//     Jacobians:  dz_0 = [I_n; 0],  du_k = -K_k dz_k,  dx_{k+1} = A dx_k + B du_k          (K0 = -K_0[:, :n])        [sens_face_forward_rate; k_sens_face: in its body]
//     VJP:        lam_N = [g_x[N]; 0],  lam_k = [g_x[k]; 0] - K_k' g_u[k] + Acl_k' lam_{k+1},   g_x0 = lam_0[:n]     [sens_face_costate]
// The VJP rides the backward sweep (no stored gains, no Jacobian); K0 alone is the backward sweep; dU and dX need the gains of every
// stage, which go to a per-instance scratch Kst [N][m w] in global memory (stage k at k m w, column-major m x w, the x columns first)
// and come back one stage ahead in the forward pass.
//
// Conventions, stated once for both kernels:
//   Active-set rule, on the returned u (there is no Jacobi scale here): row (k, i) is in W iff  u[i,k] - umin_i <= tau w_i  or
//     umax_i - u[i,k] <= tau w_i,  w_i = umax_i - umin_i.  Weakly active rows: the derivative of the face on which every flagged row
//     is held, as in k_sens.  A clamped input is an identity row and column of Lam, so the factor is that of the free block.
//   Team: one wave per instance, up to SENS_FACE_WAVES (SENS_FACE_RATE_WAVES) waves per workgroup that never wait for each other;
//     every matrix of a stage in the wave's slice of LDS, column-major.  Every hand-over through LDS is a SensTeam<false> fence
//     (release, wave barrier, acquire); a piece says in its comment which fences it holds and which it leaves to its caller.
//   Failure: an unsolved instance (status != 0), or a pivot of Lam that is not positive and finite, gives rows = -1 and zeros in every
//     output that was asked for (sens_face_unsolved).
//   <NC, MC>: dimensions known at compile time (0, 0: from the parameters), as k_riccati_t.
//
// k_sens_face (S = 0; w = n):
//     P+ = sym(P) at k = N;  Lam = R_ff + B_f' P+ B_f  (R as the design uses it: zero when R[1,1] == 0),  rhs = B_f' P+ A,
//     Acl_k = A - B K_k,   P+ <- Qbar_k + Acl_k' P+ Acl_k + K_k' R K_k  (symmetrised),  Qbar_k = Q (1 <= k <= N-1)
//   every product one entry per lane (sens_face_mul), which fixes its order of summation.  LDS: A, Q, P+, T (= P+ Acl, then the new P
//   before it is symmetrised; dx+ in the forward pass), Acl | B, P+ B, K (solved in place), R K | R, Lam | lam, lam+ | the stage masks.
//
// k_sens_face_rate (S in the design; w = nt):
//   The cost carries sum_k (u_k - u_{k+1})' S (u_k - u_{k+1}), k = 0 .. N-2, so a stage sees the input before it: the face problem is
//   an LQ problem in the stage state z_k = [dx_k; du_{k-1}].  R as the design uses it, S symmetrised; S_k = S for k >= 1 and S_0 = 0
//   (nothing ties u_0 to an input applied before the horizon):
//     At = [A 0; 0 0] (nt x nt)    Bt = [B; I] (nt x m)    Nt_k = [0; -S_k] (nt x m)    Rt_k = R + S_k    Qt_k = blkdiag(Qbar_k, S_k)
//     Pi+ = blkdiag(sym(P), 0) at k = N;  Lam = (Rt_k + Bt' Pi+ Bt)_ff,  rhs = (Bt' Pi+ At + Nt_k')_f,  Acl_k = At - Bt K_k,
//     Pi+ <- Qt_k + K_k' Rt_k K_k - Nt_k K_k - K_k' Nt_k' + Acl_k' Pi+ Acl_k            (symmetrised)
//   The blocks of At, Bt and Nt are used where they are cheap: Pi+ Bt = Pi+[:, :n] B + Pi+[:, n:],  Bt' Pi+ At = [(Pi+ Bt)[:n]' A, 0],
//   the w columns of B'Pi+At + Nt' are -S_k, the lower rows of Acl are -K, and dz is carried as dx (n x n) and the du before (m x n).
//   Pi+ Acl and Acl' (Pi+ Acl) are full nt x nt products (the closed loop has no zero block), computed by 2 x 2 blocks of the result
//   in a lane's registers (sens_face_mul22): the one-entry-per-lane product of k_sens_face read every operand word from LDS once per
//   product and made K0 of 4096 quadrotors at N = 50 cost 3.5 times k_sens_face on the S = 0 design; blocked it costs 1.8 times.
//   LDS: A, Q (n x n) | Pi+, T (= Pi+ Acl, then the symmetrised new Pi), Acl (nt x nt) | B (n x m) | Pi+ Bt, K, Rt K, S K (nt x m or
//   m x nt) | R, S, Lam (m x m) | lam, lam+ (nt) | the stage masks.  The new Pi is written over the old one, which has no reader once
//   Pi+ Acl is formed, and symmetrised into T; then the two change places -- no per-lane copy of a matrix, whatever nt.  The look-ahead
//   gain of the forward pass is the only per-lane array: m nt <= 768 entries, 12 a lane.
// k_sens_ltv (almpc_sens_ltv.hip.h) mirrors the stage bodies of both kernels entry for entry, with a model per stage: a change of the
// arithmetic here belongs there as well.
constexpr int SENS_FACE_WAVES = 4;

struct SensFaceParams {
    int n, m, N, batch;
    const double* A; long A_stride;     // n x n column-major (stride 0: shared)
    const double* B; long B_stride;     // n x m
    const double* Q; const double* R;   // n x n, m x m, symmetric, shared (R: zeros where the design dropped it)
    const double* P; long P_stride;     // n x n terminal weight
    const double* umin; const double* umax;   // [m]
    const double* u;                    // [batch][N][m] returned inputs
    const int32_t* status;              // [batch]
    double tau;
    unsigned want;                      // SENS_* (Jacobian mode)
    double* Kst;                        // [batch][N][m n] gains (only with SENS_DU / SENS_DX)
    double* K0; double* dU; double* dX; // layouts of SensParams / SensDxParams
    const double* g_u; const double* g_x;   // [batch][N][m], [batch][N+1][n] or null (VJP mode)
    double* g_x0;                       // [batch][n]
    int32_t* rows;                      // [batch] |W|, or -1
    int lds_per_wave;                   // doubles
};

__host__ __device__ inline int sens_face_lds_doubles(int n, int m, int N) {
    return (5 * n * n + 4 * n * m + 2 * m * m + 2 * n + (N + 1) / 2 + 1) & ~1;
}

// out (r x c) = op(X) (r x k) Y (k x c), column-major; TX: X is stored k x r and used transposed
template <bool TX>
__device__ __forceinline__ void sens_face_mul(double* out, const double* X, const double* Y, int r, int k, int c, int lane) {
    for (int t = lane; t < r * c; t += 64) {
        const int i = t % r, j = t / r;
        double acc = 0.0;
        for (int l = 0; l < k; ++l) acc += (TX ? X[l + i * k] : X[i + l * r]) * Y[l + j * k];
        out[t] = acc;
    }
}

// ---- the pieces both kernels are put together from.  n, m, N are the kernel's own (compile-time in a <NC, MC> build); w is the width
// of its stage state; every pointer is into the calling wave's slice of LDS unless it says global.

// A, Q, B and R of the instance into LDS.  No fence: the one inside sens_face_active_set, which follows, hands them over.  Behind this
// call and in front of that fence each kernel writes what is its own, in loops of its own: P+ (sym(P), or blkdiag(sym(P), 0)) and,
// with the rate weight, sym(S).  These stores are independent copies into disjoint arrays, so their order among themselves changes
// no bit; both kernels use the same one (stage_in, P+, S).
__device__ __forceinline__ void sens_face_stage_in(const SensFaceParams& p, int inst, double* As, double* Qs, double* Bs, double* Rs,
                                                   int n, int m, int lane) {
    const double* Ag = p.A + (size_t)inst * p.A_stride;
    const double* Bg = p.B + (size_t)inst * p.B_stride;
    for (int t = lane; t < n * n; t += 64) { As[t] = Ag[t]; Qs[t] = p.Q[t]; }
    for (int t = lane; t < n * m; t += 64) Bs[t] = Bg[t];
    for (int t = lane; t < m * m; t += 64) Rs[t] = p.R[t];
}

// The rows at a bound: wset[k] bit a = input a of stage k is held (m <= 16 bits of a word).  Returns |W|, the same in every lane.  One
// fence, between the zeroing of the masks and the flags; the masks themselves are handed over by the caller's next fence.
__device__ __forceinline__ int sens_face_active_set(const SensTeam<false>& T, const SensFaceParams& p, int inst, uint32_t* wset,
                                                    int m, int N, int lane) {
    const int nz = N * m;
    int rows = 0;
    for (int k = lane; k < N; k += 64) wset[k] = 0u;
    T.sync();
    for (int t = lane; t < nz; t += 64) {
        const int k = t / m, a = t - k * m;
        const double uj = p.u[(size_t)inst * nz + t], lo = p.umin[a], hi = p.umax[a], tol = p.tau * (hi - lo);
        if (uj - lo <= tol || hi - uj <= tol) { atomicOr(&wset[k], 1u << a); ++rows; }
    }
    for (int o = 32; o > 0; o >>= 1) rows += __shfl_xor(rows, o);
    return rows;
}

// K = Lam^-1 K in place: Lam (m x m, SPD on the free inputs, identity on the held ones) is factored, then a lane takes a column of K
// (m x cols) through both substitutions.  False on a pivot that is not positive and finite (every lane sees the same one): the caller
// leaves its sweep for sens_face_unsolved.  0 < MC <= 4: every lane factors Lam in its own registers (ten entries, no fence between
// the pivots; the diagonal is kept as its reciprocal).  Otherwise the Cholesky factor replaces the lower triangle of Lam in LDS, three
// fences a pivot.  The caller fences in front (Lam and K written) and behind (K read).
template <int MC>
__device__ __forceinline__ bool sens_face_gain_solve(const SensTeam<false>& T, double* Lam, double* Ks, int m, int cols, int lane) {
    if constexpr (MC > 0 && MC <= 4) {
        bool ok = true;
        double l[MC][MC];
#pragma unroll
        for (int i = 0; i < MC; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) l[i][j] = Lam[i + j * MC];
#pragma unroll
        for (int c = 0; c < MC; ++c) {
            const double piv = l[c][c];
            if (!(piv > 0.0 && piv <= 1.7976931348623157e308)) ok = false;
            const double inv = 1.0 / sqrt(piv);
            l[c][c] = inv;
#pragma unroll
            for (int i = c + 1; i < MC; ++i) l[i][c] *= inv;
#pragma unroll
            for (int j = c + 1; j < MC; ++j)
#pragma unroll
                for (int i = j; i < MC; ++i) l[i][j] -= l[i][c] * l[j][c];
        }
        if (!ok) return false;
        for (int c = lane; c < cols; c += 64) {
            double x[MC];
#pragma unroll
            for (int i = 0; i < MC; ++i) x[i] = Ks[i + c * MC];
#pragma unroll
            for (int i = 0; i < MC; ++i) {
#pragma unroll
                for (int j = 0; j < i; ++j) x[i] -= l[i][j] * x[j];
                x[i] *= l[i][i];
            }
#pragma unroll
            for (int i = MC - 1; i >= 0; --i) {
#pragma unroll
                for (int j = i + 1; j < MC; ++j) x[i] -= l[j][i] * x[j];
                x[i] *= l[i][i];
            }
#pragma unroll
            for (int i = 0; i < MC; ++i) Ks[i + c * MC] = x[i];
        }
    } else {
        for (int c = 0; c < m; ++c) {
            const double piv = Lam[c + c * m];                 // (every lane reads the same word)
            if (!(piv > 0.0 && piv <= 1.7976931348623157e308)) return false;
            const double dk = sqrt(piv);
            T.sync();
            for (int i = c + lane; i < m; i += 64) Lam[i + c * m] = i == c ? dk : Lam[i + c * m] / dk;
            T.sync();
            const int rem = m - c - 1;
            for (int idx = lane; idx < rem * rem; idx += 64) {
                const int i = c + 1 + idx / rem, j = c + 1 + idx % rem;
                if (j <= i) Lam[i + j * m] -= Lam[i + c * m] * Lam[j + c * m];
            }
            T.sync();
        }
        for (int c = lane; c < cols; c += 64) {
            double* x = Ks + c * m;
            for (int i = 0; i < m; ++i) {
                double s = x[i];
                for (int j = 0; j < i; ++j) s -= Lam[i + j * m] * x[j];
                x[i] = s / Lam[i + i * m];
            }
            for (int i = m - 1; i >= 0; --i) {
                double s = x[i];
                for (int j = i + 1; j < m; ++j) s -= Lam[j + i * m] * x[j];
                x[i] = s / Lam[i + i * m];
            }
        }
    }
    return true;
}

// The costate of the VJP, lam_k = [g_x[k]; 0] - K_k' g_u[k] + Acl_k' lam_{k+1}: n of its w rows have a g_x.
// sens_face_costate_end writes lam_N = [g_x[N]; 0] (0.0 is added where g_x is null, so that a null g_x and a g_x of zeros give the same
// bits); sens_face_costate returns row `lane` of lam_k (0 beyond w), which the caller stores behind its own fence.
__device__ __forceinline__ void sens_face_costate_end(const SensFaceParams& p, int inst, double* lam, int n, int w, int N, int lane) {
    const double* gx = p.g_x ? p.g_x + (size_t)inst * (N + 1) * n : nullptr;
    for (int i = lane; i < w; i += 64) lam[i] = i < n ? 0.0 + (gx ? gx[(size_t)N * n + i] : 0.0) : 0.0;
}
__device__ __forceinline__ double sens_face_costate(const SensFaceParams& p, int inst, int k, const double* Ks, const double* Ac,
                                                    const double* lam, int n, int w, int m, int N, int lane) {
    double ln = 0.0;
    if (lane < w) {
        const double* gu = p.g_u + (size_t)inst * (N * m) + (size_t)k * m;
        ln = (p.g_x && lane < n) ? p.g_x[((size_t)inst * (N + 1) + k) * n + lane] : 0.0;
        for (int a = 0; a < m; ++a) ln -= Ks[a + lane * m] * gu[a];
        for (int l = 0; l < w; ++l) ln += Ac[l + lane * w] * lam[l];
    }
    return ln;
}

// An unsolved instance, or a pivot that is not positive and finite: zeros in what was asked for, rows = -1
template <bool VJP>
__device__ __forceinline__ void sens_face_unsolved(const SensFaceParams& p, int inst, int n, int m, int N, int lane) {
    const int nn = n * n, nm = n * m, nz = N * m;
    if (VJP) {
        for (int c = lane; c < n; c += 64) p.g_x0[(size_t)inst * n + c] = 0.0;
    } else {
        if (p.want & SENS_K0)
            for (int t = lane; t < nm; t += 64) p.K0[(size_t)inst * nm + t] = 0.0;
        if (p.want & (SENS_DU | SENS_DX))
            for (int t = lane; t < n * nz; t += 64) p.dU[(size_t)inst * n * nz + t] = 0.0;
        if (p.want & SENS_DX)
            for (int t = lane; t < (N + 1) * nn; t += 64) p.dX[(size_t)inst * (N + 1) * nn + t] = 0.0;
    }
    if (lane == 0) p.rows[inst] = -1;
}

// The forward pass behind a backward sweep in the stage state [dx; du-] that stored its gains in p.Kst: dU, and dX where it is asked
// for.  dx and dxn are n x n, du and dup (the du of the stage before) m x n; Ks takes the stage's gain, m x (n + m).  The gains were
// stored by other lanes of this wave: made visible at device scope, read back past the L1 and one stage ahead, in look-ahead
// registers whose number follows from KM_MAX, the caller's compile-time bound on m (n + m) -- a caller cannot truncate the gain.
// dz_0 = [I; 0] gives du_0 the bits of K0.  (k_sens_face keeps its own forward pass in its body: see there.)
template <int KM_MAX>
__device__ __forceinline__ void sens_face_forward_rate(const SensTeam<false>& T, const SensFaceParams& p, int inst, const double* As,
                                                       const double* Bs, double* Ks, double* dx, double* dxn, double* du, double* dup,
                                                       int n, int m, int N, int lane) {
    constexpr int KREG = (KM_MAX + 63) / 64;
    const int nn = n * n, nm = n * m, nz = N * m, km = (n + m) * m;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __builtin_amdgcn_wave_barrier();
    const double* Kg = p.Kst + (size_t)inst * N * km;
    double* dUo = p.dU + (size_t)inst * n * nz;
    double* dXo = p.dX + (size_t)inst * (N + 1) * nn;
    const bool wdx = (p.want & SENS_DX) != 0;
    double kreg[KREG];
    auto kload = [&](int k) {
#pragma unroll
        for (int c = 0; c < KREG; ++c) {
            const int t = lane + 64 * c;
            kreg[c] = t < km ? __hip_atomic_load(Kg + (size_t)k * km + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        }
    };
    kload(0);
    for (int t = lane; t < nn; t += 64) {
        const int i = t % n, c = t / n;
        const double v = i == c ? 1.0 : 0.0;
        dx[t] = v;
        if (wdx) dXo[(size_t)c * (N + 1) * n + i] = v;
    }
    T.sync();
    for (int k = 0; k < N; ++k) {
#pragma unroll
        for (int c = 0; c < KREG; ++c) {
            const int t = lane + 64 * c;
            if (t < km) Ks[t] = kreg[c];
        }
        if (k + 1 < N) kload(k + 1);
        T.sync();
        for (int t = lane; t < nm; t += 64) {                  // du = -K dz = -K_x dx - K_w du-
            const int a = t % m, c = t / m;
            double s = 0.0;
            if (k == 0) s -= Ks[t];
            else {
                for (int j = 0; j < n; ++j) s -= Ks[a + j * m] * dx[j + c * n];
                for (int b = 0; b < m; ++b) s -= Ks[a + (n + b) * m] * dup[b + c * m];
            }
            du[t] = s;
            dUo[(size_t)c * nz + (size_t)k * m + a] = s;
        }
        T.sync();
        if (k + 1 < N || wdx) {
            for (int t = lane; t < nn; t += 64) {              // dx+ = A dx + B du
                const int i = t % n, c = t / n;
                double s = 0.0;
                for (int j = 0; j < n; ++j) s += As[i + j * n] * dx[j + c * n];
                for (int a = 0; a < m; ++a) s += Bs[i + a * n] * du[a + c * m];
                dxn[t] = s;
                if (wdx) dXo[((size_t)c * (N + 1) + k + 1) * n + i] = s;
            }
            T.sync();
            double* sw = dx; dx = dxn; dxn = sw;
        }
        { double* sw = du; du = dup; dup = sw; }
    }
}

template <bool VJP, int NC, int MC>
__global__ __launch_bounds__(64 * SENS_FACE_WAVES) void k_sens_face(SensFaceParams p) {
    extern __shared__ __attribute__((aligned(16))) double sens_face_smem[];
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int n = NC ? NC : p.n, m = MC ? MC : p.m, N = p.N, nn = n * n, nm = n * m, mm = m * m, nz = N * m;
    const SensTeam<false> T{lane, 64};
    double* L = sens_face_smem + (size_t)wv * p.lds_per_wave;
    double* As = L;            double* Qs = As + nn;    double* Pn = Qs + nn;   double* Tm = Pn + nn;   double* Ac = Tm + nn;
    double* Bs = Ac + nn;      double* PB = Bs + nm;    double* Ks = PB + nm;   double* RK = Ks + nm;
    double* Rs = RK + nm;      double* Lam = Rs + mm;
    double* lam = Lam + mm;    double* lamn = lam + n;
    uint32_t* wset = reinterpret_cast<uint32_t*>(lamn + n);   // [N] the stage masks
    const bool jac = !VJP && (p.want & (SENS_DU | SENS_DX)) != 0;

    const int wpb = (int)(blockDim.x >> 6), nwaves = gridDim.x * wpb;
    for (int inst = blockIdx.x * wpb + wv; inst < p.batch; inst += nwaves) {
        T.sync();   // (the previous instance of this wave has read its last LDS operand)
        bool ok = p.status[inst] == 0;
        int rows = 0;
        if (ok) {
            const double* Pg = p.P + (size_t)inst * p.P_stride;
            sens_face_stage_in(p, inst, As, Qs, Bs, Rs, n, m, lane);
            for (int t = lane; t < nn; t += 64) Pn[t] = 0.5 * (Pg[t] + Pg[(t % n) * n + t / n]);   // P+ = sym(P)
            rows = sens_face_active_set(T, p, inst, wset, m, N, lane);
            if (VJP) sens_face_costate_end(p, inst, lam, n, n, N, lane);
            T.sync();
        }
        // ---- backward sweep
        for (int k = N - 1; ok && k >= 0; --k) {
            const uint32_t wk = wset[k];
            sens_face_mul<false>(PB, Pn, Bs, n, n, m, lane);   // P+ B
            T.sync();
            sens_face_mul<true>(Ks, PB, As, m, n, n, lane);    // B' P+ A = (P+ B)' A   (P+ is symmetric)
            sens_face_mul<true>(Lam, Bs, PB, m, n, m, lane);   // B' P+ B
            T.sync();
            for (int t = lane; t < mm; t += 64) {              // Lam = R + B'P+B, identity on the held inputs
                const int i = t % m, j = t / m;
                const bool hi_ = (wk >> i) & 1u, hj = (wk >> j) & 1u;
                Lam[t] = (hi_ || hj) ? (i == j ? 1.0 : 0.0) : Lam[t] + Rs[t];
            }
            for (int t = lane; t < nm; t += 64)                // the rows of the held inputs vanish
                if ((wk >> (t % m)) & 1u) Ks[t] = 0.0;
            T.sync();
            if (!sens_face_gain_solve<MC>(T, Lam, Ks, m, n, lane)) { ok = false; break; }   // K = Lam^-1 (B'P+A)
            T.sync();
            if (jac) {
                double* Kg = p.Kst + ((size_t)inst * N + k) * nm;
                for (int t = lane; t < nm; t += 64) Kg[t] = Ks[t];
            }
            if (!VJP && k == 0 && (p.want & SENS_K0))
                for (int t = lane; t < nm; t += 64) p.K0[(size_t)inst * nm + t] = 0.0 - Ks[t];
            if (!VJP && k == 0) break;                         // (P_0 has no reader)
            for (int t = lane; t < nn; t += 64) {              // Acl = A - B K
                const int i = t % n, j = t / n;
                double s = As[t];
                for (int a = 0; a < m; ++a) s -= Bs[i + a * n] * Ks[a + j * m];
                Ac[t] = s;
            }
            if (k > 0) sens_face_mul<false>(RK, Rs, Ks, m, m, n, lane);   // R K
            T.sync();
            double ln = 0.0;
            if (VJP) ln = sens_face_costate(p, inst, k, Ks, Ac, lam, n, n, m, N, lane);
            if (k > 0) {
                sens_face_mul<false>(Tm, Pn, Ac, n, n, n, lane);   // P+ Acl
                T.sync();
                double pnew[16];   // n n <= 1024: at most 16 entries per lane
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const int t = lane + 64 * c;
                    double s = 0.0;
                    if (t < nn) {
                        const int i = t % n, j = t / n;
                        s = Qs[t];
                        for (int l = 0; l < n; ++l) s += Ac[l + i * n] * Tm[l + j * n];
                        for (int a = 0; a < m; ++a) s += Ks[a + i * m] * RK[a + j * m];
                    }
                    pnew[c] = s;
                }
                T.sync();
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const int t = lane + 64 * c;
                    if (t < nn) Tm[t] = pnew[c];               // (Tm is free now: the new P before it is symmetrised)
                }
                T.sync();
                for (int t = lane; t < nn; t += 64) Pn[t] = 0.5 * (Tm[t] + Tm[(t % n) * n + t / n]);
            }
            if (VJP && lane < n) lamn[lane] = ln;
            T.sync();
            if (VJP) { double* sw = lam; lam = lamn; lamn = sw; }
        }
        if (!ok) { sens_face_unsolved<VJP>(p, inst, n, m, N, lane); continue; }
        if (lane == 0) p.rows[inst] = rows;
        if (VJP) {
            for (int c = lane; c < n; c += 64) p.g_x0[(size_t)inst * n + c] = lam[c];
            continue;
        }
        if (!jac) continue;
        // ---- forward pass: dx in Pn, dx+ in Tm, du in PB.  The gains were stored by other lanes of this wave: made visible at device
        // scope, read back past the L1 and one stage ahead.  The same scaffold as sens_face_forward_rate without the du- term, kept in the
        // body: taken out as a function it costs the <.., 12, 4> build its schedule (229 VGPRs for 235, K0 of 4096 quadrotors 0.5 to 0.8 %
        // slower: DESIGN.md section 4)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __builtin_amdgcn_wave_barrier();
        const double* Kg = p.Kst + (size_t)inst * N * nm;
        double* dUo = p.dU + (size_t)inst * n * nz;
        double* dXo = p.dX + (size_t)inst * (N + 1) * nn;
        const bool wdx = (p.want & SENS_DX) != 0;
        double kreg[8];   // n m <= 512: at most 8 entries per lane
        auto kload = [&](int k) {
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int t = lane + 64 * c;
                kreg[c] = t < nm ? __hip_atomic_load(Kg + (size_t)k * nm + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
            }
        };
        kload(0);
        double* dx = Pn;
        double* dxn = Tm;
        for (int t = lane; t < nn; t += 64) {
            const int i = t % n, c = t / n;
            const double v = i == c ? 1.0 : 0.0;
            dx[t] = v;
            if (wdx) dXo[(size_t)c * (N + 1) * n + i] = v;
        }
        T.sync();
        for (int k = 0; k < N; ++k) {
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int t = lane + 64 * c;
                if (t < nm) Ks[t] = kreg[c];
            }
            if (k + 1 < N) kload(k + 1);
            T.sync();
            for (int t = lane; t < nm; t += 64) {              // du = -K dx  (dx_0 = I: the bits of K0)
                const int a = t % m, c = t / m;
                double s = 0.0;
                if (k == 0) s -= Ks[t];
                else for (int j = 0; j < n; ++j) s -= Ks[a + j * m] * dx[j + c * n];
                PB[t] = s;
                dUo[(size_t)c * nz + (size_t)k * m + a] = s;
            }
            T.sync();
            if (k + 1 < N || wdx) {
                for (int t = lane; t < nn; t += 64) {          // dx+ = A dx + B du
                    const int i = t % n, c = t / n;
                    double s = 0.0;
                    for (int j = 0; j < n; ++j) s += As[i + j * n] * dx[j + c * n];
                    for (int a = 0; a < m; ++a) s += Bs[i + a * n] * PB[a + c * m];
                    dxn[t] = s;
                    if (wdx) dXo[((size_t)c * (N + 1) + k + 1) * n + i] = s;
                }
                T.sync();
                double* sw = dx; dx = dxn; dxn = sw;
            }
        }
    }
}

// ---- k_sens_face_rate (the description is in front of k_sens_face)
constexpr int SENS_FACE_RATE_WAVES = 4;
constexpr int SENS_FACE_RATE_MAX_M = 16, SENS_FACE_RATE_MAX_NT = 48;   // (the shapes the structured solve with S serves: n <= 32, m <= 16, n + m <= 48)

struct SensFaceRateParams {
    SensFaceParams f;                   // as k_sens_face; Kst is [batch][N][m nt], lds_per_wave that of sens_face_rate_lds_doubles
    const double* S;                    // m x m, shared
};

__host__ __device__ inline int sens_face_rate_lds_doubles(int n, int m, int N) {
    const int nt = n + m;
    return (2 * n * n + 3 * nt * nt + n * m + 4 * nt * m + 3 * m * m + 2 * nt + (N + 1) / 2 + 1) & ~1;
}

// out (r x c) = X (r x k) Y (k x c), column-major, a 2 x 2 block of the result in a lane's registers: every operand word read from LDS
// feeds two products, half the reads of sens_face_mul; each entry is summed in the same order.  An odd edge takes its last row or
// column twice and stores it once.
__device__ __forceinline__ void sens_face_mul22(double* out, const double* X, const double* Y, int r, int k, int c, int lane) {
    const int rb = (r + 1) >> 1, cb = (c + 1) >> 1;
    for (int t = lane; t < rb * cb; t += 64) {
        const int i = 2 * (t % rb), j = 2 * (t / rb);
        const bool i1 = i + 1 < r, j1 = j + 1 < c;
        const int ii = i1 ? i + 1 : i, jj = j1 ? j + 1 : j;
        double a00 = 0.0, a10 = 0.0, a01 = 0.0, a11 = 0.0;
        for (int l = 0; l < k; ++l) {
            const double x0 = X[i + l * r], x1 = X[ii + l * r], y0 = Y[l + j * k], y1 = Y[l + jj * k];
            a00 += x0 * y0; a10 += x1 * y0; a01 += x0 * y1; a11 += x1 * y1;
        }
        out[i + j * r] = a00;
        if (i1) out[ii + j * r] = a10;
        if (j1) out[i + jj * r] = a01;
        if (i1 && j1) out[ii + jj * r] = a11;
    }
}

template <bool VJP, int NC, int MC>
__global__ __launch_bounds__(64 * SENS_FACE_RATE_WAVES) void k_sens_face_rate(SensFaceRateParams q) {
    extern __shared__ __attribute__((aligned(16))) double sens_face_rate_smem[];
    static_assert((NC == 0) == (MC == 0), "both dimensions at compile time, or neither");
    static_assert(MC <= SENS_FACE_RATE_MAX_M && NC + MC <= SENS_FACE_RATE_MAX_NT, "a build beyond the served shapes");
    constexpr int KM_MAX = NC ? MC * (NC + MC) : SENS_FACE_RATE_MAX_M * SENS_FACE_RATE_MAX_NT;   // m nt at most: sizes the look-ahead gain
    const SensFaceParams& p = q.f;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int n = NC ? NC : p.n, m = MC ? MC : p.m, N = p.N, nt = n + m, nn = n * n, nm = n * m, mm = m * m, tt = nt * nt, tm = nt * m;
    const SensTeam<false> T{lane, 64};
    double* L = sens_face_rate_smem + (size_t)wv * p.lds_per_wave;
    double* As = L;            double* Qs = As + nn;
    double* Pn = Qs + nn;      double* Tm = Pn + tt;    double* Ac = Tm + tt;
    double* Bs = Ac + tt;
    double* PB = Bs + nm;      double* Ks = PB + tm;    double* RK = Ks + tm;   double* SK = RK + tm;
    double* Rs = SK + tm;      double* Ss = Rs + mm;    double* Lam = Ss + mm;
    double* lam = Lam + mm;    double* lamn = lam + nt;
    uint32_t* wset = reinterpret_cast<uint32_t*>(lamn + nt);   // [N] bit a: input a of the stage is held (m <= 16 bits)
    const bool jac = !VJP && (p.want & (SENS_DU | SENS_DX)) != 0;

    const int wpb = (int)(blockDim.x >> 6), nwaves = gridDim.x * wpb;
    for (int inst = blockIdx.x * wpb + wv; inst < p.batch; inst += nwaves) {
        T.sync();   // (the previous instance of this wave has read its last LDS operand)
        bool ok = p.status[inst] == 0;
        int rows = 0;
        if (ok) {
            const double* Pg = p.P + (size_t)inst * p.P_stride;
            sens_face_stage_in(p, inst, As, Qs, Bs, Rs, n, m, lane);
            for (int t = lane; t < tt; t += 64) {              // Pi+ = blkdiag(sym(P), 0)
                const int i = t % nt, j = t / nt;
                Pn[t] = (i < n && j < n) ? 0.5 * (Pg[i + j * n] + Pg[j + i * n]) : 0.0;
            }
            for (int t = lane; t < mm; t += 64) Ss[t] = 0.5 * (q.S[t] + q.S[(t % m) * m + t / m]);
            rows = sens_face_active_set(T, p, inst, wset, m, N, lane);
            if (VJP) sens_face_costate_end(p, inst, lam, n, nt, N, lane);
            T.sync();
        }
        // ---- backward sweep
        for (int k = N - 1; ok && k >= 0; --k) {
            const uint32_t wk = wset[k];
            const bool rate = k > 0;                           // S_0 = 0: stage 0 has no S term in Rt, Nt or Qt
            for (int t = lane; t < tm; t += 64) {              // Pi+ Bt = Pi+[:, :n] B + Pi+[:, n:]
                const int i = t % nt, a = t / nt;
                double acc = Pn[i + (n + a) * nt];
                for (int l = 0; l < n; ++l) acc += Pn[i + l * nt] * Bs[l + a * n];
                PB[t] = acc;
            }
            T.sync();
            for (int t = lane; t < tm; t += 64) {              // Bt' Pi+ At + Nt' = [(Pi+ Bt)[:n]' A, -S_k]
                const int a = t % m, j = t / m;
                double acc = 0.0;
                if (j < n) for (int l = 0; l < n; ++l) acc += PB[l + a * nt] * As[l + j * n];
                else if (rate) acc = 0.0 - Ss[a + (j - n) * m];
                Ks[t] = ((wk >> a) & 1u) ? 0.0 : acc;          // the rows of the held inputs vanish
            }
            for (int t = lane; t < mm; t += 64) {              // Lam = Rt + Bt' Pi+ Bt = R + S_k + B' (Pi+ Bt)[:n] + (Pi+ Bt)[n:], identity on the held inputs
                const int i = t % m, j = t / m;
                double acc = PB[n + i + j * nt];
                for (int l = 0; l < n; ++l) acc += Bs[l + i * n] * PB[l + j * nt];
                acc += Rs[t];
                if (rate) acc += Ss[t];
                const bool hi_ = (wk >> i) & 1u, hj = (wk >> j) & 1u;
                Lam[t] = (hi_ || hj) ? (i == j ? 1.0 : 0.0) : acc;
            }
            T.sync();
            if (!sens_face_gain_solve<MC>(T, Lam, Ks, m, nt, lane)) { ok = false; break; }   // K = Lam^-1 (Bt'Pi+At + Nt')
            T.sync();
            if (jac) {
                double* Kg = p.Kst + ((size_t)inst * N + k) * tm;
                for (int t = lane; t < tm; t += 64) Kg[t] = Ks[t];
            }
            if (!VJP && k == 0 && (p.want & SENS_K0))
                for (int t = lane; t < nm; t += 64) p.K0[(size_t)inst * nm + t] = 0.0 - Ks[t];   // (the x columns come first)
            if (!VJP && k == 0) break;                         // (Pi_0 has no reader)
            for (int t = lane; t < tt; t += 64) {              // Acl = At - Bt K = [A - B K_x, -B K_w; -K]
                const int i = t % nt, j = t / nt;
                double s;
                if (i < n) {
                    s = j < n ? As[i + j * n] : 0.0;
                    for (int a = 0; a < m; ++a) s -= Bs[i + a * n] * Ks[a + j * m];
                } else s = 0.0 - Ks[(i - n) + j * m];
                Ac[t] = s;
            }
            if (k > 0)
                for (int t = lane; t < tm; t += 64) {          // Rt K and S K
                    const int a = t % m, j = t / m;
                    double r = 0.0, s = 0.0;
                    for (int b = 0; b < m; ++b) {
                        const double kb = Ks[b + j * m];
                        r += Rs[a + b * m] * kb;
                        s += Ss[a + b * m] * kb;
                    }
                    RK[t] = r + s;
                    SK[t] = s;
                }
            T.sync();
            double ln = 0.0;
            if (VJP) ln = sens_face_costate(p, inst, k, Ks, Ac, lam, n, nt, m, N, lane);
            if (k > 0) {
                sens_face_mul22(Tm, Pn, Ac, nt, nt, nt, lane);        // Pi+ Acl
                T.sync();
                // the new Pi over the old one, which has no reader left: Acl' (Pi+ Acl) by 2 x 2 blocks, then the terms of the stage
                const int hb = (nt + 1) >> 1;
                for (int t = lane; t < hb * hb; t += 64) {
                    const int i0 = 2 * (t % hb), j0 = 2 * (t / hb);
                    const int i1 = i0 + 1 < nt ? i0 + 1 : i0, j1 = j0 + 1 < nt ? j0 + 1 : j0;
                    double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
                    for (int l = 0; l < nt; ++l) {
                        const double a0 = Ac[l + i0 * nt], a1 = Ac[l + i1 * nt], b0 = Tm[l + j0 * nt], b1 = Tm[l + j1 * nt];
                        acc[0][0] += a0 * b0; acc[1][0] += a1 * b0; acc[0][1] += a0 * b1; acc[1][1] += a1 * b1;
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int i = i0 + (e & 1), j = j0 + (e >> 1);
                        if (i >= nt || j >= nt) continue;
                        double s = (i < n && j < n) ? Qs[i + j * n] : ((i >= n && j >= n) ? Ss[(i - n) + (j - n) * m] : 0.0);
                        s += acc[e & 1][e >> 1];
                        for (int a = 0; a < m; ++a) s += Ks[a + i * m] * RK[a + j * m];
                        if (i >= n) s += SK[(i - n) + j * m];  // - Nt K = [0; S K]
                        if (j >= n) s += SK[(j - n) + i * m];  // - K' Nt'
                        Pn[i + j * nt] = s;
                    }
                }
                T.sync();
                for (int t = lane; t < tt; t += 64) Tm[t] = 0.5 * (Pn[t] + Pn[(t % nt) * nt + t / nt]);
                double* sw = Pn; Pn = Tm; Tm = sw;
            }
            if (VJP && lane < nt) lamn[lane] = ln;
            T.sync();
            if (VJP) { double* sw = lam; lam = lamn; lamn = sw; }
        }
        if (!ok) { sens_face_unsolved<VJP>(p, inst, n, m, N, lane); continue; }
        if (lane == 0) p.rows[inst] = rows;
        if (VJP) {
            for (int c = lane; c < n; c += 64) p.g_x0[(size_t)inst * n + c] = lam[c];
            continue;
        }
        if (jac) sens_face_forward_rate<KM_MAX>(T, p, inst, As, Bs, Ks, Pn, Tm, PB, RK, n, m, N, lane);   // (dx, dx+ are n x n in Pi+, T)
    }
}

}  // namespace almpc
