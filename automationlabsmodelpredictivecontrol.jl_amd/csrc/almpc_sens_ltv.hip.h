// almpc_sens_ltv.hip.h -- k_sens_ltv: the sensitivities of a step of a time-varying design (almpc_design_ltv) in its initial deviation:
// K0, du/dx0, dx/dx0 and the VJP (almpc_sensitivity_ltv, almpc_sensitivity_ltv_vjp).
//
// The design's QP is solved at dx_0 = 0; with dx_0 = p in its place the face problem -- the rows W of the returned u held -- is an LQ
// problem in p with the stage models A_k, B_k, and its derivative at p = 0 is the Riccati recursion of k_sens_face / k_sens_face_rate
// (almpc_sens.hip.h: the description in front of k_sens_face holds for this kernel word for word) with A_k, B_k in place of A, B.  The
// linearisation trajectory, the defects c_k and the references do not enter: the face problem is linear in p.
//     RATE == false (the design took no S):  w = n,  the sweep of k_sens_face
//     RATE == true  (useS):                  w = n + m, the sweep of k_sens_face_rate with At_k = [A_k 0; 0 0], Bt_k = [B_k; I], S_0 = 0
// Conventions (active-set rule, weakly active rows, team, fences, failure, <NC, MC>): those of k_sens_face.  The pieces are that
// file's: sens_face_mul, sens_face_mul22, sens_face_active_set, sens_face_gain_solve, sens_face_costate*, sens_face_unsolved; what a stage
// computes between them is the arithmetic of the sibling kernel, entry for entry, so that a design whose stage models are all one
// (A, B) gives the bits of the sibling.  Two pieces are this file's own, because theirs read one model per instance:
//     sens_ltv_stage_in   (beside sens_face_stage_in)       stage N-1's model, the shared weights
//     sens_ltv_forward    (beside sens_face_forward_rate)   the forward pass with A_k, B_k and, per RATE, with or without the du- term
//
// Stage loads.  A_k, B_k come from the handle's kept copies, [batch][N][n n] and [batch][N][n m]; n, m <= 16, so a stage's model is at
// most four words of A and four of B per lane (SensLtvStageRegs).  Backward: the loads of stage k-1 are issued at the top of stage k, into
// registers; A_k and B_k have their last reader (Acl_k) in front of the fence that follows it, so the registers are stored to the
// same LDS arrays behind that fence, in front of the fence that ends the stage -- which hands them to stage k-1.  No fence is added
// and nothing is double-buffered.  Forward: stage k+1's loads are issued at the top of stage k beside the look-ahead gain and stored
// at the top of stage k+1 with it, in front of the fence that hands over the gain.  Every load is unconditional (element 0 where the
// lane has no entry): a load inside a per-element branch is waited for on the spot.  The fences are wavefront-scope and wait for no
// vector-memory counter, so a stage's model and look-ahead gain are waited for once, at their store to LDS.  (The VJP builds also read
// g_u[k], g_x[k] inside sens_face_costate, the siblings' piece used as it is: those loads are waited for where they are used, on the
// chain of every stage, as in k_sens_face -- DESIGN.md section 7, item 9.)
#pragma once
#include "almpc_sens.hip.h"

namespace almpc {

constexpr int SENS_LTV_WAVES = 4;
constexpr int SENS_LTV_MAX_N = 16, SENS_LTV_MAX_M = 16, SENS_LTV_MAX_STATES = 1024;   // the shapes a step behind an LTV design accepts

struct SensLtvParams {
    SensFaceParams f;                   // as k_sens_face, but A, B: the kept stage models [batch][N][n n], [batch][N][n m] (A_stride = N n n,
                                        // B_stride = N n m); Q, R, S symmetrised as the design left them on the device; Kst [batch][N][m w]
    const double* S;                    // m x m, shared (read only with RATE)
    int useR;                           // the design's branch: R is part of the cost (else zeros take its place)
};

__host__ __device__ inline int sens_ltv_lds_doubles(int n, int m, int N, bool rate) {
    return rate ? sens_face_rate_lds_doubles(n, m, N) : sens_face_lds_doubles(n, m, N);
}

// A stage's model on its way from global memory to LDS: entries lane + 64 c of A_k (n n <= 256) and of B_k (n m <= 256)
template <int AR, int BR>
struct SensLtvStageRegs {
    double a[AR], b[BR];
    __device__ __forceinline__ void load(const double* Ag, const double* Bg, int nn, int nm, int lane) {
#pragma unroll
        for (int c = 0; c < AR; ++c) { const int t = lane + 64 * c; a[c] = Ag[t < nn ? t : 0]; }
#pragma unroll
        for (int c = 0; c < BR; ++c) { const int t = lane + 64 * c; b[c] = Bg[t < nm ? t : 0]; }
    }
    __device__ __forceinline__ void store(double* As, double* Bs, int nn, int nm, int lane) const {
#pragma unroll
        for (int c = 0; c < AR; ++c) { const int t = lane + 64 * c; if (t < nn) As[t] = a[c]; }
#pragma unroll
        for (int c = 0; c < BR; ++c) { const int t = lane + 64 * c; if (t < nm) Bs[t] = b[c]; }
    }
};

// A_{N-1}, B_{N-1}, Q and R into LDS (R: zeros where the design dropped it).  No fence, as sens_face_stage_in: the one inside
// sens_face_active_set hands them over, and the caller writes P+ and S behind this call in the sibling's order.
__device__ __forceinline__ void sens_ltv_stage_in(const SensLtvParams& q, const double* Ag, const double* Bg, double* As, double* Qs,
                                                  double* Bs, double* Rs, int n, int m, int lane) {
    for (int t = lane; t < n * n; t += 64) { As[t] = Ag[t]; Qs[t] = q.f.Q[t]; }
    for (int t = lane; t < n * m; t += 64) Bs[t] = Bg[t];
    for (int t = lane; t < m * m; t += 64) Rs[t] = q.useR ? q.f.R[t] : 0.0;
}

// The forward pass behind a backward sweep that stored its gains in p.Kst and left A_0, B_0 in As, Bs: dU, and dX where it is asked for.
// The scaffold of sens_face_forward_rate (RATE: its du- term; else k_sens_face's own pass) with the model of the stage: Ag, Bg are the
// instance's kept stage models, read one stage ahead beside the gain.  dx, dxn n x n; du, dup m x n (dup: RATE only).
template <bool RATE, int KM_MAX, int AR, int BR>
__device__ __forceinline__ void sens_ltv_forward(const SensTeam<false>& T, const SensFaceParams& p, int inst, const double* Ag,
                                                 const double* Bg, double* As, double* Bs, double* Ks, double* dx, double* dxn, double* du,
                                                 double* dup, int n, int m, int N, int lane) {
    constexpr int KREG = (KM_MAX + 63) / 64;
    const int nn = n * n, nm = n * m, nz = N * m, km = (RATE ? n + m : n) * m;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __builtin_amdgcn_wave_barrier();
    const double* Kg = p.Kst + (size_t)inst * N * km;
    double* dUo = p.dU + (size_t)inst * n * nz;
    double* dXo = p.dX + (size_t)inst * (N + 1) * nn;
    const bool wdx = (p.want & SENS_DX) != 0;
    double kreg[KREG];
    SensLtvStageRegs<AR, BR> sr;
    auto kload = [&](int k) {
#pragma unroll
        for (int c = 0; c < KREG; ++c) {
            const int t = lane + 64 * c;
            // (no select on the loaded value: it would be waited for here; the store to Ks is guarded by t < km)
            kreg[c] = __hip_atomic_load(Kg + (size_t)k * km + (t < km ? t : 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
        if (k > 0) sr.store(As, Bs, nn, nm, lane);             // (stage k-1's dx+ is behind its fence: A_{k-1}, B_{k-1} have no reader)
        if (k + 1 < N) {
            kload(k + 1);
            sr.load(Ag + (size_t)(k + 1) * nn, Bg + (size_t)(k + 1) * nm, nn, nm, lane);
        }
        T.sync();
        for (int t = lane; t < nm; t += 64) {                  // du = -K dz = -K_x dx [- K_w du-]   (dz_0 = [I; 0]: the bits of K0)
            const int a = t % m, c = t / m;
            double s = 0.0;
            if (k == 0) s -= Ks[t];
            else {
                for (int j = 0; j < n; ++j) s -= Ks[a + j * m] * dx[j + c * n];
                if (RATE)
                    for (int b = 0; b < m; ++b) s -= Ks[a + (n + b) * m] * dup[b + c * m];
            }
            du[t] = s;
            dUo[(size_t)c * nz + (size_t)k * m + a] = s;
        }
        T.sync();
        if (k + 1 < N || wdx) {
            for (int t = lane; t < nn; t += 64) {              // dx+ = A_k dx + B_k du
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
        if (RATE) { double* sw = du; du = dup; dup = sw; }
    }
}

template <bool VJP, bool RATE, int NC, int MC>
__global__ __launch_bounds__(64 * SENS_LTV_WAVES) void k_sens_ltv(SensLtvParams q) {
    extern __shared__ __attribute__((aligned(16))) double sens_ltv_smem[];
    static_assert((NC == 0) == (MC == 0), "both dimensions at compile time, or neither");
    static_assert(NC <= SENS_LTV_MAX_N && MC <= SENS_LTV_MAX_M, "a build beyond the served shapes");
    constexpr int AR = NC ? (NC * NC + 63) / 64 : (SENS_LTV_MAX_N * SENS_LTV_MAX_N + 63) / 64;
    constexpr int BR = NC ? (NC * MC + 63) / 64 : (SENS_LTV_MAX_N * SENS_LTV_MAX_M + 63) / 64;
    constexpr int KM_MAX = NC ? MC * (NC + (RATE ? MC : 0)) : SENS_LTV_MAX_M * (SENS_LTV_MAX_N + (RATE ? SENS_LTV_MAX_M : 0));
    const SensFaceParams& p = q.f;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int n = NC ? NC : p.n, m = MC ? MC : p.m, N = p.N, nn = n * n, nm = n * m, mm = m * m;
    const int w = RATE ? n + m : n, ww = w * w, wm = w * m;   // the stage state's width (nt with RATE)
    const SensTeam<false> T{lane, 64};
    double* L = sens_ltv_smem + (size_t)wv * p.lds_per_wave;
    // the sibling's slice: A, Q (n x n) | P+, T, Acl (w x w) | B (n x m) | P+ Bt, K, Rt K [, S K] (w x m or m x w) | R [, S], Lam | lam, lam+ | masks
    double* As = L;            double* Qs = As + nn;
    double* Pn = Qs + nn;      double* Tm = Pn + ww;    double* Ac = Tm + ww;
    double* Bs = Ac + ww;
    double* PB = Bs + nm;      double* Ks = PB + wm;    double* RK = Ks + wm;   double* SK = RK + wm;
    double* Rs = SK + (RATE ? wm : 0);                  double* Ss = Rs + mm;   double* Lam = Ss + (RATE ? mm : 0);
    double* lam = Lam + mm;    double* lamn = lam + w;
    uint32_t* wset = reinterpret_cast<uint32_t*>(lamn + w);   // [N] bit a: input a of the stage is held (m <= 16 bits)
    const bool jac = !VJP && (p.want & (SENS_DU | SENS_DX)) != 0;

    const int wpb = (int)(blockDim.x >> 6), nwaves = gridDim.x * wpb;
    for (int inst = blockIdx.x * wpb + wv; inst < p.batch; inst += nwaves) {
        T.sync();   // (the previous instance of this wave has read its last LDS operand)
        const double* Ag = p.A + (size_t)inst * p.A_stride;
        const double* Bg = p.B + (size_t)inst * p.B_stride;
        bool ok = p.status[inst] == 0;
        int rows = 0;
        if (ok) {
            const double* Pg = p.P + (size_t)inst * p.P_stride;
            sens_ltv_stage_in(q, Ag + (size_t)(N - 1) * nn, Bg + (size_t)(N - 1) * nm, As, Qs, Bs, Rs, n, m, lane);
            if constexpr (RATE) {
                for (int t = lane; t < ww; t += 64) {          // Pi+ = blkdiag(sym(P), 0)
                    const int i = t % w, j = t / w;
                    Pn[t] = (i < n && j < n) ? 0.5 * (Pg[i + j * n] + Pg[j + i * n]) : 0.0;
                }
                for (int t = lane; t < mm; t += 64) Ss[t] = 0.5 * (q.S[t] + q.S[(t % m) * m + t / m]);
            } else {
                for (int t = lane; t < nn; t += 64) Pn[t] = 0.5 * (Pg[t] + Pg[(t % n) * n + t / n]);   // P+ = sym(P)
            }
            rows = sens_face_active_set(T, p, inst, wset, m, N, lane);
            if (VJP) sens_face_costate_end(p, inst, lam, n, w, N, lane);
            T.sync();
        }
        // ---- backward sweep
        SensLtvStageRegs<AR, BR> sr;
        for (int k = N - 1; ok && k >= 0; --k) {
            const uint32_t wk = wset[k];
            if (k > 0) sr.load(Ag + (size_t)(k - 1) * nn, Bg + (size_t)(k - 1) * nm, nn, nm, lane);   // stage k-1's model, on its way while stage k computes
            if constexpr (RATE) {
                const bool rate = k > 0;                           // S_0 = 0: stage 0 has no S term in Rt, Nt or Qt
                for (int t = lane; t < wm; t += 64) {              // Pi+ Bt = Pi+[:, :n] B_k + Pi+[:, n:]
                    const int i = t % w, a = t / w;
                    double acc = Pn[i + (n + a) * w];
                    for (int l = 0; l < n; ++l) acc += Pn[i + l * w] * Bs[l + a * n];
                    PB[t] = acc;
                }
                T.sync();
                for (int t = lane; t < wm; t += 64) {              // Bt' Pi+ At + Nt' = [(Pi+ Bt)[:n]' A_k, -S_k]
                    const int a = t % m, j = t / m;
                    double acc = 0.0;
                    if (j < n) for (int l = 0; l < n; ++l) acc += PB[l + a * w] * As[l + j * n];
                    else if (rate) acc = 0.0 - Ss[a + (j - n) * m];
                    Ks[t] = ((wk >> a) & 1u) ? 0.0 : acc;          // the rows of the held inputs vanish
                }
                for (int t = lane; t < mm; t += 64) {              // Lam = Rt + Bt' Pi+ Bt, identity on the held inputs
                    const int i = t % m, j = t / m;
                    double acc = PB[n + i + j * w];
                    for (int l = 0; l < n; ++l) acc += Bs[l + i * n] * PB[l + j * w];
                    acc += Rs[t];
                    if (rate) acc += Ss[t];
                    const bool hi_ = (wk >> i) & 1u, hj = (wk >> j) & 1u;
                    Lam[t] = (hi_ || hj) ? (i == j ? 1.0 : 0.0) : acc;
                }
                T.sync();
            } else {
                sens_face_mul<false>(PB, Pn, Bs, n, n, m, lane);   // P+ B_k
                T.sync();
                sens_face_mul<true>(Ks, PB, As, m, n, n, lane);    // B_k' P+ A_k = (P+ B_k)' A_k   (P+ is symmetric)
                sens_face_mul<true>(Lam, Bs, PB, m, n, m, lane);   // B_k' P+ B_k
                T.sync();
                for (int t = lane; t < mm; t += 64) {              // Lam = R + B'P+B, identity on the held inputs
                    const int i = t % m, j = t / m;
                    const bool hi_ = (wk >> i) & 1u, hj = (wk >> j) & 1u;
                    Lam[t] = (hi_ || hj) ? (i == j ? 1.0 : 0.0) : Lam[t] + Rs[t];
                }
                for (int t = lane; t < nm; t += 64)                // the rows of the held inputs vanish
                    if ((wk >> (t % m)) & 1u) Ks[t] = 0.0;
                T.sync();
            }
            if (!sens_face_gain_solve<MC>(T, Lam, Ks, m, w, lane)) { ok = false; break; }   // K_k = Lam^-1 rhs
            T.sync();
            if (jac) {
                double* Kg = p.Kst + ((size_t)inst * N + k) * wm;
                for (int t = lane; t < wm; t += 64) Kg[t] = Ks[t];
            }
            if (!VJP && k == 0 && (p.want & SENS_K0))
                for (int t = lane; t < nm; t += 64) p.K0[(size_t)inst * nm + t] = 0.0 - Ks[t];   // (the x columns come first)
            if (!VJP && k == 0) break;                         // (P_0 has no reader)
            if constexpr (RATE) {
                for (int t = lane; t < ww; t += 64) {              // Acl = At - Bt K = [A_k - B_k K_x, -B_k K_w; -K]
                    const int i = t % w, j = t / w;
                    double s;
                    if (i < n) {
                        s = j < n ? As[i + j * n] : 0.0;
                        for (int a = 0; a < m; ++a) s -= Bs[i + a * n] * Ks[a + j * m];
                    } else s = 0.0 - Ks[(i - n) + j * m];
                    Ac[t] = s;
                }
                if (k > 0)
                    for (int t = lane; t < wm; t += 64) {          // Rt K and S K
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
            } else {
                for (int t = lane; t < nn; t += 64) {              // Acl = A_k - B_k K
                    const int i = t % n, j = t / n;
                    double s = As[t];
                    for (int a = 0; a < m; ++a) s -= Bs[i + a * n] * Ks[a + j * m];
                    Ac[t] = s;
                }
                if (k > 0) sens_face_mul<false>(RK, Rs, Ks, m, m, n, lane);   // R K
            }
            T.sync();
            // A_k, B_k have no reader behind this fence: stage k-1's model takes their place, handed over by the fence that ends the stage
            if (k > 0) sr.store(As, Bs, nn, nm, lane);
            double ln = 0.0;
            if (VJP) ln = sens_face_costate(p, inst, k, Ks, Ac, lam, n, w, m, N, lane);
            if (k > 0) {
                if constexpr (RATE) {
                    sens_face_mul22(Tm, Pn, Ac, w, w, w, lane);        // Pi+ Acl
                    T.sync();
                    // the new Pi over the old one, which has no reader left: Acl' (Pi+ Acl) by 2 x 2 blocks, then the terms of the stage
                    const int hb = (w + 1) >> 1;
                    for (int t = lane; t < hb * hb; t += 64) {
                        const int i0 = 2 * (t % hb), j0 = 2 * (t / hb);
                        const int i1 = i0 + 1 < w ? i0 + 1 : i0, j1 = j0 + 1 < w ? j0 + 1 : j0;
                        double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
                        for (int l = 0; l < w; ++l) {
                            const double a0 = Ac[l + i0 * w], a1 = Ac[l + i1 * w], b0 = Tm[l + j0 * w], b1 = Tm[l + j1 * w];
                            acc[0][0] += a0 * b0; acc[1][0] += a1 * b0; acc[0][1] += a0 * b1; acc[1][1] += a1 * b1;
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int i = i0 + (e & 1), j = j0 + (e >> 1);
                            if (i >= w || j >= w) continue;
                            double s = (i < n && j < n) ? Qs[i + j * n] : ((i >= n && j >= n) ? Ss[(i - n) + (j - n) * m] : 0.0);
                            s += acc[e & 1][e >> 1];
                            for (int a = 0; a < m; ++a) s += Ks[a + i * m] * RK[a + j * m];
                            if (i >= n) s += SK[(i - n) + j * m];  // - Nt K = [0; S K]
                            if (j >= n) s += SK[(j - n) + i * m];  // - K' Nt'
                            Pn[i + j * w] = s;
                        }
                    }
                    T.sync();
                    for (int t = lane; t < ww; t += 64) Tm[t] = 0.5 * (Pn[t] + Pn[(t % w) * w + t / w]);
                    double* sw = Pn; Pn = Tm; Tm = sw;
                } else {
                    sens_face_mul<false>(Tm, Pn, Ac, n, n, n, lane);   // P+ Acl
                    T.sync();
                    constexpr int PR = NC ? (NC * NC + 63) / 64 : (SENS_LTV_MAX_N * SENS_LTV_MAX_N + 63) / 64;   // n n <= 256: at most 4 entries per lane
                    double pnew[PR];
#pragma unroll
                    for (int c = 0; c < PR; ++c) {
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
                    for (int c = 0; c < PR; ++c) {
                        const int t = lane + 64 * c;
                        if (t < nn) Tm[t] = pnew[c];               // (Tm is free now: the new P before it is symmetrised)
                    }
                    T.sync();
                    for (int t = lane; t < nn; t += 64) Pn[t] = 0.5 * (Tm[t] + Tm[(t % n) * n + t / n]);
                }
            }
            if (VJP && lane < w) lamn[lane] = ln;
            T.sync();
            if (VJP) { double* sw = lam; lam = lamn; lamn = sw; }
        }
        if (!ok) { sens_face_unsolved<VJP>(p, inst, n, m, N, lane); continue; }
        if (lane == 0) p.rows[inst] = rows;
        if (VJP) {
            for (int c = lane; c < n; c += 64) p.g_x0[(size_t)inst * n + c] = lam[c];
            continue;
        }
        // (As, Bs hold stage 0's model: stage 1 stored it, or N = 1 and sens_ltv_stage_in read it)
        if (jac) sens_ltv_forward<RATE, KM_MAX, AR, BR>(T, p, inst, Ag, Bg, As, Bs, Ks, Pn, Tm, PB, RK, n, m, N, lane);   // (dx, dx+ in P+, T; du, du- in P+ Bt, Rt K)
    }
}

}  // namespace almpc
