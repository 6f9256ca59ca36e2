// almpc_dare_vjp.hip.h -- k_dare_vjp: the adjoint of P = DARE(A, B, Q, R), batched.  For a symmetric gP = dL/dP it returns what the loss
// gains in A, B, Q, R through P (almpc_dare_vjp_batched; almpc_sensitivity_params_vjp_dare adds it to the P-as-data gradients):
//   Sm = R + B'PB,  K = Sm^-1 B'PA,  Acl = A - B K,   X = Acl X Acl' + gP   (discrete Lyapunov equation)
//   gQ = X,   gR = K X K',   gA = 2 P Acl X,   gB = -2 P Acl X K'
// gQ and gR are symmetric (the convention of include/almpc.h for the gradient of a symmetric matrix).
//
// The algorithm is hm::dare_vjp's (csrc/almpc_host_math.h), statement by statement:
//   1. PA, PB, Sm, K and the residual of the equation as k_dare's last block forms them: status 1 on a zero / NaN pivot of Sm, status 3
//      when the residual exceeds 1e-7 max(1, max|P|, max|Q|) (k_dare's acceptance bound: P is no solution for this model);
//   2. the Lyapunov equation by doubling: X_0 = gP, A_0 = Acl;  D = A_j X_j A_j',  X_{j+1} = sym(X_j + D),  A_{j+1} = A_j A_j; it stops at
//      max|D| <= 1e-13 max(1, max|X_{j+1}|) (k_dare's stopping rule) within DARE_VJP_MAX_DOUBLINGS doublings; status 2 when an entry of
//      X is not finite or the rule is not met -- the closed loop is not stable, P is not the STABILISING solution;
//   3. the four products.  An instance with a non-zero status writes nothing but its status word.
//
// Shape: k_dare's -- one wave per instance, up to DARE_WAVES waves per workgroup while their matrices fit 160 KB, a grid-stride loop
// over the instances, no workgroup barrier, leading dimension dare_ld(n, m), lane l owns row l & (RL - 1) and every (64 / RL)-th
// column.  A wave keeps six d x d matrices (d = max(n, m)) and one m x m block, k_dare's budget, under other names:
//   S0 | S1 | S2 | S3 | S4 | S5 | Sm
//   residual:  S0 = A, S1 = P, S2 = B then A'PB, S3 = PA, S4 = PB, S5 = B'PA then K (m x n)
//   doubling:  S0 = D, S1 = X, S2 = A_j, S3 = P Acl, S4 = A_j X then A_j A_j, S5 = K
//   products:  S4 = P Acl X, S0 = P Acl X K' (n x m), S2 = K X (m x n), Sm = K X K'
// A doubling has no LU: three dependent products.  helpers (dare_mul, dare_lu_solve, dare_fence, dare_wave_max) are k_dare's.
#pragma once
#include "almpc_dare.hip.h"

namespace almpc {

struct DareVjpParams {
    int n, m, batch;
    const double* A; long A_stride;    // n x n column-major per instance (stride 0: shared)
    const double* B; long B_stride;    // n x m
    const double* P; long P_stride;    // n x n: a solution of the instance's DARE (tested)
    const double* gP; long gP_stride;  // n x n symmetric dL/dP
    const double* Q; const double* R;  // n x n and m x m: shared (strides 0), or one pair per instance
    long Q_stride = 0, R_stride = 0;
    double* gA; long gA_stride;        // outputs, each may be null
    double* gB; long gB_stride;
    double* gQ; long gQ_stride;
    double* gR; long gR_stride;
    int accumulate;                    // 1: += into the outputs, 0: plain write
    const int32_t* rows;               // null, or [batch]: an instance with rows[i] < 0 is skipped (nothing read, nothing written)
    int32_t* status;                   // [batch] 0; 1 singular Sm, 2 closed loop not stable / not finite, 3 P does not solve the equation
    int lds_per_wave;                  // doubles
};

constexpr int DARE_VJP_MAX_DOUBLINGS = 64;

template <int RL>
__global__ __launch_bounds__(64 * DARE_WAVES) void k_dare_vjp(DareVjpParams p) {
    extern __shared__ __attribute__((aligned(16))) double dare_vjp_smem[];
    constexpr int CG = 64 / RL;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int n = p.n, m = p.m, d = n > m ? n : m, ld = dare_ld(n, m);
    const int row = lane & (RL - 1), cg = lane / RL;
    double* L = dare_vjp_smem + (size_t)wv * p.lds_per_wave;
    double* S0 = L;             double* S1 = S0 + ld * d;   double* S2 = S1 + ld * d;
    double* S3 = S2 + ld * d;   double* S4 = S3 + ld * d;   double* S5 = S4 + ld * d;
    double* Sm = S5 + ld * d;
    const int wpb = (int)(blockDim.x >> 6), nwaves = gridDim.x * wpb;
    for (int inst = blockIdx.x * wpb + wv; inst < p.batch; inst += nwaves) {
        if (p.rows && __builtin_amdgcn_readfirstlane(p.rows[inst]) < 0) continue;
        const double* Ag = p.A + (size_t)inst * p.A_stride;
        const double* Bg = p.B + (size_t)inst * p.B_stride;
        const double* Pg = p.P + (size_t)inst * p.P_stride;
        const double* Gg = p.gP + (size_t)inst * p.gP_stride;
        const double* Qg = p.Q + (size_t)inst * p.Q_stride;
        const double* Rg = p.R + (size_t)inst * p.R_stride;
        int st = 0;
        dare_fence();
        // ---- 1. the residual of the equation, as k_dare's last block: S0 = A, S1 = P, S2 = B
        double pmax = 0.0, qmax = 0.0;
        if (row < n) {
            for (int j = cg; j < n; j += CG) {
                S0[row + j * ld] = Ag[row + j * n];
                const double pv = Pg[row + j * n];
                S1[row + j * ld] = pv;
                pmax = fmax(pmax, fabs(pv));
                qmax = fmax(qmax, fabs(Qg[row + j * n]));
            }
            for (int a = cg; a < m; a += CG) S2[row + a * ld] = Bg[row + a * n];
        }
        dare_fence();
        dare_mul<RL, false, false>(S3, S1, S0, nullptr, n, n, n, ld, lane);          // PA
        dare_mul<RL, false, false>(S4, S1, S2, nullptr, n, n, m, ld, lane);          // PB
        dare_fence();
        dare_mul<RL, true, false>(S5, S2, S3, nullptr, m, n, n, ld, lane);           // B'PA  (m x n)
        if (row < m)                                                               // Sm = B'PB + R
            for (int b = cg; b < m; b += CG) {
                double acc = 0.0;
                for (int l = 0; l < n; ++l) acc += S2[l + row * ld] * S4[l + b * ld];
                Sm[row + b * ld] = acc + Rg[row + b * m];
            }
        dare_fence();
        dare_mul<RL, true, false>(S2, S0, S4, nullptr, n, n, m, ld, lane);           // A'PB over B (B was last read before the fence)
        if (!dare_lu_solve<RL>(Sm, S5, m, n, ld, lane)) st = 1;                      // K = Sm^-1 B'PA
        if (!st) {
            double rmax = 0.0;
            bool notfin = false;
            if (row < n)
                for (int j = cg; j < n; j += CG) {
                    double acc = 0.0, corr = 0.0;
                    for (int l = 0; l < n; ++l) acc += S0[l + row * ld] * S3[l + j * ld];
                    for (int a = 0; a < m; ++a) corr += S2[row + a * ld] * S5[a + j * ld];
                    const double res = acc + (Qg[row + j * n] - S1[row + j * ld] - corr);
                    rmax = fmax(rmax, fabs(res));
                    notfin = notfin || !(fabs(res) <= 1.7976931348623157e308);
                }
            rmax = dare_wave_max(rmax); pmax = dare_wave_max(pmax); qmax = dare_wave_max(qmax);
            if (__any(notfin ? 1 : 0) || !__builtin_amdgcn_readfirstlane(rmax <= 1e-7 * fmax(1.0, fmax(pmax, qmax)) ? 1 : 0)) st = 3;
        }
        // ---- 2. Acl = A - B K, P Acl, then X = Acl X Acl' + gP by doubling
        bool converged = false;
        if (!st) {
            dare_fence();
            if (row < n)
                for (int a = cg; a < m; a += CG) S4[row + a * ld] = Bg[row + a * n];     // B again (PB is done with)
            dare_fence();
            if (row < n)
                for (int j = cg; j < n; j += CG) {
                    double acc = 0.0;
                    for (int a = 0; a < m; ++a) acc += S4[row + a * ld] * S5[a + j * ld];
                    S2[row + j * ld] = S0[row + j * ld] - acc;                           // Acl (A'PB is done with)
                }
            dare_fence();
            dare_mul<RL, false, false>(S3, S1, S2, nullptr, n, n, n, ld, lane);          // P Acl (PA is done with)
            dare_fence();
            if (row < n)
                for (int j = cg; j < n; j += CG) S1[row + j * ld] = Gg[row + j * n];     // X_0 = gP (P is done with)
            dare_fence();
        }
        for (int it = 0; it < DARE_VJP_MAX_DOUBLINGS && !st && !converged; ++it) {
            dare_mul<RL, false, false>(S4, S2, S1, nullptr, n, n, n, ld, lane);          // T = A_j X_j
            dare_fence();
            dare_mul<RL, false, true>(S0, S4, S2, nullptr, n, n, n, ld, lane);           // D = T A_j'
            dare_fence();
            dare_mul<RL, false, false>(S4, S2, S2, nullptr, n, n, n, ld, lane);          // A_j A_j (T is done with)
            // X_{j+1} = sym(X_j + D) (each pair by one lane), max|D|, max|X_{j+1}|, finiteness
            double diff = 0.0, xmax = 0.0;
            bool notfin = false;
            if (row < n)
                for (int j = cg; j < n; j += CG) {
                    if (row > j) continue;
                    const double a = S1[row + j * ld] + S0[row + j * ld], b = S1[j + row * ld] + S0[j + row * ld];
                    const double x = row == j ? a : 0.5 * (a + b);
                    diff = fmax(diff, fmax(fabs(S0[row + j * ld]), fabs(S0[j + row * ld])));
                    xmax = fmax(xmax, fabs(x));
                    notfin = notfin || !(fabs(x) <= 1.7976931348623157e308);
                    S1[row + j * ld] = x; S1[j + row * ld] = x;
                }
            dare_fence();
            if (row < n)
                for (int j = cg; j < n; j += CG) S2[row + j * ld] = S4[row + j * ld];
            dare_fence();
            if (__any(notfin ? 1 : 0)) { st = 2; break; }   // (an entry that is not finite never becomes finite again)
            diff = dare_wave_max(diff); xmax = dare_wave_max(xmax);
            converged = __builtin_amdgcn_readfirstlane(diff <= 1e-13 * fmax(1.0, xmax) ? 1 : 0) != 0;
        }
        if (!st && !converged) st = 2;
        // ---- 3. gQ = X, gA = 2 P Acl X, gB = -2 P Acl X K', gR = sym(K X K')
        if (!st) {
            dare_mul<RL, false, false>(S4, S3, S1, nullptr, n, n, n, ld, lane);          // P Acl X
            dare_mul<RL, false, false>(S2, S5, S1, nullptr, m, n, n, ld, lane);          // K X  (m x n; A_j is done with)
            dare_fence();
            dare_mul<RL, false, true>(S0, S4, S5, nullptr, n, n, m, ld, lane);           // P Acl X K'  (n x m)
            dare_mul<RL, false, true>(Sm, S2, S5, nullptr, m, n, m, ld, lane);           // K X K'  (m x m, not yet symmetric)
            dare_fence();
            const bool acc = p.accumulate != 0;
            if (row < n) {
                if (p.gQ) {
                    double* o = p.gQ + (size_t)inst * p.gQ_stride;
                    for (int j = cg; j < n; j += CG) { const double v = S1[row + j * ld]; o[row + j * n] = acc ? o[row + j * n] + v : v; }
                }
                if (p.gA) {
                    double* o = p.gA + (size_t)inst * p.gA_stride;
                    for (int j = cg; j < n; j += CG) { const double v = 2.0 * S4[row + j * ld]; o[row + j * n] = acc ? o[row + j * n] + v : v; }
                }
                if (p.gB) {
                    double* o = p.gB + (size_t)inst * p.gB_stride;
                    for (int a = cg; a < m; a += CG) { const double v = -2.0 * S0[row + a * ld]; o[row + a * n] = acc ? o[row + a * n] + v : v; }
                }
            }
            if (row < m && p.gR) {
                double* o = p.gR + (size_t)inst * p.gR_stride;
                for (int b = cg; b < m; b += CG) {
                    const double v = row == b ? Sm[row + b * ld] : 0.5 * (Sm[row + b * ld] + Sm[b + row * ld]);
                    o[row + b * m] = acc ? o[row + b * m] + v : v;
                }
            }
        }
        if (lane == 0) p.status[inst] = st;
    }
}

}  // namespace almpc
