// Driver of the CPU sanitizer build of the library's HOST half for the certificate of a step (almpc_certificate, almpc_get_certificate,
// almpc_device_certificate and their group forms): csrc/almpc_api.hip compiled host-only under AddressSanitizer +
// UndefinedBehaviorSanitizer and linked against tests/sanitize/fake_hip_runtime.cpp, as host_logic_driver.cpp is (device memory =
// calloc'd host memory, launches = no-ops, so every buffer the calls size, upload and read back is bounds-checked).  Walks the entry
// points on condensed (shared, per-instance, weighted) and structured (shared, per-instance) handles with and without S and with R
// dropped, every `want` mask, null outputs, every refusal, a group of three, and the certificate interleaved with the other readers of
// the handle's kept weights on handles that are redesigned (also with m > n).  Prints "cert host logic ok: <launches> launches".
#include "../../include/almpc.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

extern "C" long fake_hip_launch_count();
extern char** environ;

#define CK(call)                                                                                             \
    do {                                                                                                     \
        const int rc_ = (call);                                                                              \
        if (rc_ != ALMPC_OK) { std::fprintf(stderr, "%s:%d %s -> %d (%s)\n", __FILE__, __LINE__, #call, rc_, h ? almpc_last_error(h) : ""); return 1; } \
    } while (0)
#define CKG(call)                                                                                            \
    do {                                                                                                     \
        const int rc_ = (call);                                                                              \
        if (rc_ != ALMPC_OK) { std::fprintf(stderr, "%s:%d %s -> %d (%s)\n", __FILE__, __LINE__, #call, rc_, almpc_group_last_error(g)); return 1; } \
    } while (0)
#define EXPECT(call, want)                                                                                   \
    do {                                                                                                     \
        const int rc_ = (call);                                                                              \
        if (rc_ != (want)) { std::fprintf(stderr, "%s:%d %s -> %d, expected %d\n", __FILE__, __LINE__, #call, rc_, (int)(want)); return 1; } \
    } while (0)
// a refusal carries its reason
#define REFUSED(call, want)                                                                                  \
    do {                                                                                                     \
        EXPECT(call, want);                                                                                  \
        if (!almpc_last_error(h) || !*almpc_last_error(h)) { std::fprintf(stderr, "%s:%d no message\n", __FILE__, __LINE__); return 1; } \
    } while (0)

struct Plant {
    int n, m;
    std::vector<double> A, B, Q, R, S, P, umin, umax, xmin, xmax;
};

static Plant chain(int n, int m) {   // stable chain of integrators-with-leak, column-major
    Plant p;
    p.n = n; p.m = m;
    p.A.assign((size_t)n * n, 0.0); p.B.assign((size_t)n * m, 0.0); p.Q.assign((size_t)n * n, 0.0); p.R.assign((size_t)m * m, 0.0);
    p.S.assign((size_t)m * m, 0.0); p.P.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) {
        p.A[(size_t)i * n + i] = 0.9;
        if (i + 1 < n) p.A[(size_t)(i + 1) * n + i] = 0.1;
        p.Q[(size_t)i * n + i] = 100.0; p.P[(size_t)i * n + i] = 150.0;
    }
    for (int a = 0; a < m; ++a) { p.B[(size_t)a * n + (n - 1 - a)] = 0.5; p.R[(size_t)a * m + a] = 0.1; p.S[(size_t)a * m + a] = 2.0; }
    p.umin.assign(m, -1.0); p.umax.assign(m, 1.0); p.xmin.assign(n, -3.0); p.xmax.assign(n, 3.0);
    return p;
}

template <class T>
static std::vector<T> tiled(const std::vector<T>& v, int times) {
    std::vector<T> out;
    for (int i = 0; i < times; ++i) out.insert(out.end(), v.begin(), v.end());
    return out;
}

static int step(almpc_handle* h, int n, int batch) {
    std::vector<double> x0((size_t)batch * n, 0.25);
    CK(almpc_update_initialization(h, x0.data()));
    CK(almpc_calculate(h, nullptr));
    return 0;
}

// every mask on a stepped handle, the getters with every combination of null outputs, the device view
static int masks(almpc_handle* h, int n, int m, int N, int batch) {
    std::vector<double> cost(batch), res(batch), grad((size_t)batch * N * m), lam((size_t)batch * (N + 1) * n);
    for (uint32_t want = 1; want < 16; ++want) {
        CK(almpc_certificate(h, want));
        for (uint32_t ask = 0; ask < 16; ++ask) {
            const int rc = almpc_get_certificate(h, (ask & ALMPC_CERT_COST) ? cost.data() : nullptr, (ask & ALMPC_CERT_RES) ? res.data() : nullptr,
                                                 (ask & ALMPC_CERT_GRAD) ? grad.data() : nullptr, (ask & ALMPC_CERT_COSTATE) ? lam.data() : nullptr);
            if (rc != ((ask & ~want) ? ALMPC_ERR_INVALID : ALMPC_OK)) { std::fprintf(stderr, "get_certificate want %u ask %u -> %d\n", want, ask, rc); return 1; }
        }
        const double *dc = &cost[0], *dr = &cost[0], *dg = &cost[0], *dl = &cost[0];
        CK(almpc_device_certificate(h, &dc, &dr, &dg, &dl));
        if (!!dc != !!(want & ALMPC_CERT_COST) || !!dr != !!(want & ALMPC_CERT_RES) || !!dg != !!(want & ALMPC_CERT_GRAD) || !!dl != !!(want & ALMPC_CERT_COSTATE)) return 1;
        CK(almpc_device_certificate(h, nullptr, nullptr, nullptr, nullptr));
    }
    return 0;
}

static int walk_handle(const char* name, almpc_handle* h, int n, int m, int N, int batch) {
    std::vector<double> cost(batch);
    REFUSED(almpc_certificate(h, ALMPC_CERT_COST), ALMPC_ERR_INVALID);   // designed, no step yet
    REFUSED(almpc_get_certificate(h, cost.data(), nullptr, nullptr, nullptr), ALMPC_ERR_INVALID);
    REFUSED(almpc_device_certificate(h, nullptr, nullptr, nullptr, nullptr), ALMPC_ERR_INVALID);
    if (step(h, n, batch)) return 1;
    REFUSED(almpc_certificate(h, 0), ALMPC_ERR_INVALID);
    REFUSED(almpc_certificate(h, 16), ALMPC_ERR_INVALID);
    REFUSED(almpc_certificate(h, 0x80000001u), ALMPC_ERR_INVALID);
    REFUSED(almpc_get_certificate(h, cost.data(), nullptr, nullptr, nullptr), ALMPC_ERR_INVALID);   // nothing computed for this step
    if (masks(h, n, m, N, batch)) return 1;
    if (step(h, n, batch)) return 1;   // a new step voids the certificate of the last one
    REFUSED(almpc_get_certificate(h, cost.data(), nullptr, nullptr, nullptr), ALMPC_ERR_INVALID);
    CK(almpc_certificate(h, ALMPC_CERT_COST | ALMPC_CERT_RES));   // (the shared weights are on the device already)
    CK(almpc_get_certificate(h, cost.data(), nullptr, nullptr, nullptr));
    std::printf("%s ok\n", name);
    return 0;
}

// The handle's one record of its weights and its one device copy, between readers and between designs: the certificate, every group of
// the parameter gradients (with and without the DARE followed) and the certificate again on a condensed handle, redesigned with other
// weights (the readers in the other order), with R dropped, per instance, weighted and per instance again; the certificate between the
// two structured-handle sensitivity calls, redesigned with another S.  m > n as well: the offsets in the device copy are not symmetric.
struct Grads {
    std::vector<double> g_u, g_x, x0, f, u_ref, u_min, u_max, Q, P, A, R, S, B;
    std::vector<int32_t> rows, dare;
    almpc_param_grads out;
    Grads(int n, int m, int N, int b)
        : g_u((size_t)b * N * m, 0.5), g_x((size_t)b * (N + 1) * n, -0.25), x0((size_t)b * n), f((size_t)b * N * m), u_ref((size_t)b * N * m),
          u_min((size_t)b * m), u_max((size_t)b * m), Q((size_t)b * n * n), P((size_t)b * n * n), A((size_t)b * n * n), R((size_t)b * m * m),
          S((size_t)b * m * m), B((size_t)b * n * m), rows(b), dare(b) {
        std::memset(&out, 0, sizeof out);
        out.x0 = x0.data(); out.f = f.data(); out.u_ref = u_ref.data(); out.u_min = u_min.data(); out.u_max = u_max.data();
        out.Q = Q.data(); out.P = P.data(); out.A = A.data(); out.R = R.data(); out.S = S.data(); out.B = B.data(); out.rows = rows.data();
    }
};

static int readers(almpc_handle* h, Grads& g, int n, int batch, bool params_first, bool follow_dare) {
    if (step(h, n, batch)) return 1;
    if (!params_first) CK(almpc_certificate(h, 15));
    CK(almpc_sensitivity_params_vjp(h, g.g_u.data(), g.g_x.data(), 0.0, &g.out));
    if (follow_dare) CK(almpc_sensitivity_params_vjp_dare(h, g.g_u.data(), nullptr, 0.0, &g.out, g.dare.data()));
    CK(almpc_certificate(h, 15));
    CK(almpc_get_certificate(h, g.x0.data(), g.u_min.data(), g.f.data(), nullptr));
    return 0;
}

static int interleaved(int n, int m, int N, int batch) {
    almpc_handle* h = nullptr;
    const Plant p = chain(n, m);
    Plant q = p;   // other weights: Q2 = 3 Q + a symmetric off-diagonal term, R2 = R / 4, S2 = 2 S, another P
    for (double& v : q.Q) v *= 3.0;
    q.Q[1] = q.Q[(size_t)n] = 7.0;
    for (double& v : q.R) v *= 0.25;
    for (double& v : q.S) v *= 2.0;
    for (double& v : q.P) v *= 1.5;
    std::vector<double> R0 = q.R;
    R0[0] = 0.0;
    const std::vector<double> Ab = tiled(p.A, batch), Bb = tiled(p.B, batch), Pb = tiled(p.P, batch);
    const std::vector<double> Qb = tiled(q.Q, batch), Rb = tiled(q.R, batch), Sb = tiled(q.S, batch);
    Grads g(n, m, N, batch);
    CK(almpc_create(&h, n, m, N, batch, 0, 0));
    CK(almpc_design_shared(h, p.A.data(), p.B.data(), p.Q.data(), p.R.data(), p.S.data(), nullptr, p.umin.data(), p.umax.data(), nullptr, nullptr, 0.1, 1e-6));
    if (readers(h, g, n, batch, false, true)) return 1;
    CK(almpc_design_shared(h, q.A.data(), q.B.data(), q.Q.data(), q.R.data(), q.S.data(), q.P.data(), q.umin.data(), q.umax.data(), nullptr, nullptr, 0.1, 1e-6));
    if (readers(h, g, n, batch, true, true)) return 1;
    CK(almpc_design_shared(h, q.A.data(), q.B.data(), q.Q.data(), R0.data(), q.S.data(), q.P.data(), q.umin.data(), q.umax.data(), nullptr, nullptr, 0.1, 1e-6));
    if (readers(h, g, n, batch, false, false)) return 1;
    REFUSED(almpc_sensitivity_params_vjp_dare(h, g.g_u.data(), nullptr, 0.0, &g.out, g.dare.data()), ALMPC_ERR_UNSUPPORTED);
    CK(almpc_design_batched(h, Ab.data(), Bb.data(), p.Q.data(), p.R.data(), p.S.data(), Pb.data(), 1, p.umin.data(), p.umax.data(), 0.1, 1e-6));
    if (readers(h, g, n, batch, false, true)) return 1;
    CK(almpc_design_batched_weighted(h, Ab.data(), Bb.data(), Qb.data(), Rb.data(), Sb.data(), Pb.data(), 1, p.umin.data(), p.umax.data(), 0.1, 1e-6));
    if (readers(h, g, n, batch, true, true)) return 1;
    CK(almpc_design_batched(h, Ab.data(), Bb.data(), p.Q.data(), p.R.data(), p.S.data(), nullptr, 0, p.umin.data(), p.umax.data(), 0.1, 1e-6));
    if (readers(h, g, n, batch, false, true)) return 1;
    almpc_destroy(h); h = nullptr;
    CK(almpc_create(&h, n, m, N, batch, 0, ALMPC_FLAG_STRUCTURED));
    for (int pass = 0; pass < 2; ++pass) {   // S, then 2 S and the calls in the reverse order
        const Plant& w = pass ? q : p;
        CK(almpc_design_shared(h, w.A.data(), w.B.data(), w.Q.data(), w.R.data(), w.S.data(), w.P.data(), w.umin.data(), w.umax.data(), nullptr, nullptr, 0.1, 1e-6));
        if (step(h, n, batch)) return 1;
        if (pass) CK(almpc_sensitivity_stagewise_rate_vjp(h, g.g_u.data(), g.g_x.data(), 0.0, g.x0.data(), g.rows.data()));
        else CK(almpc_sensitivity_stagewise_rate(h, ALMPC_SENS_K0, 0.0));
        CK(almpc_certificate(h, 15));
        if (pass) CK(almpc_sensitivity_stagewise_rate(h, ALMPC_SENS_K0 | ALMPC_SENS_DU | ALMPC_SENS_DX, 0.0));
        else CK(almpc_sensitivity_stagewise_rate_vjp(h, g.g_u.data(), nullptr, 0.0, g.x0.data(), nullptr));
        CK(almpc_certificate(h, 15));
    }
    almpc_destroy(h); h = nullptr;
    std::printf("interleaved %d-%d-%d ok\n", n, m, N);
    return 0;
}

int main() {
    {   // every almpc_create below reads the switches: none may come in from the caller's environment
        std::vector<std::string> inherited;
        for (char** e = environ; *e; ++e)
            if (std::strncmp(*e, "ALMPC_", 6) == 0) inherited.emplace_back(*e, std::strchr(*e, '=') - *e);
        for (const std::string& name : inherited) unsetenv(name.c_str());
    }
    almpc_handle* h = nullptr;
    EXPECT(almpc_certificate(nullptr, 1), ALMPC_ERR_INVALID);
    EXPECT(almpc_get_certificate(nullptr, nullptr, nullptr, nullptr, nullptr), ALMPC_ERR_INVALID);
    EXPECT(almpc_device_certificate(nullptr, nullptr, nullptr, nullptr, nullptr), ALMPC_ERR_INVALID);
    EXPECT(almpc_group_certificate(nullptr, 1), ALMPC_ERR_INVALID);
    EXPECT(almpc_group_get_certificate(nullptr, nullptr, nullptr, nullptr, nullptr), ALMPC_ERR_INVALID);
    const int n = 5, m = 2, N = 9, batch = 19;
    const Plant p = chain(n, m);
    const std::vector<double> Ab = tiled(p.A, batch), Bb = tiled(p.B, batch), Pb = tiled(p.P, batch);
    const std::vector<double> Qb = tiled(p.Q, batch), Rb = tiled(p.R, batch), Sb = tiled(p.S, batch);
    std::vector<double> R0 = p.R;
    R0[0] = 0.0;   // the branch rule drops R and S
    // ---- condensed handles
    for (int variant = 0; variant < 4; ++variant) {   // S | no S | R dropped (P given) | P given
        CK(almpc_create(&h, n, m, N, batch, 0, 0));
        REFUSED(almpc_certificate(h, ALMPC_CERT_COST), ALMPC_ERR_NOT_DESIGNED);
        const double* S = variant == 1 ? nullptr : p.S.data();
        const double* R = variant == 2 ? R0.data() : p.R.data();
        const double* P = variant >= 2 ? p.P.data() : nullptr;
        CK(almpc_design_shared(h, p.A.data(), p.B.data(), p.Q.data(), R, S, P, p.umin.data(), p.umax.data(), nullptr, nullptr, 0.1, 1e-6));
        if (walk_handle("condensed shared", h, n, m, N, batch)) return 1;
        // a new design voids the certificate and the uploaded weights
        std::vector<double> cost(batch);
        CK(almpc_design_shared(h, p.A.data(), p.B.data(), p.Q.data(), p.R.data(), nullptr, nullptr, p.umin.data(), p.umax.data(), nullptr, nullptr, 0.1, 1e-6));
        REFUSED(almpc_get_certificate(h, cost.data(), nullptr, nullptr, nullptr), ALMPC_ERR_INVALID);
        if (walk_handle("condensed shared, redesigned", h, n, m, N, batch)) return 1;
        almpc_destroy(h); h = nullptr;
    }
    for (int variant = 0; variant < 3; ++variant) {   // P = NULL | one P | P per instance
        CK(almpc_create(&h, n, m, N, batch, 0, 0));
        CK(almpc_design_batched(h, Ab.data(), Bb.data(), p.Q.data(), p.R.data(), p.S.data(), variant == 0 ? nullptr : variant == 1 ? p.P.data() : Pb.data(),
                                variant == 2, p.umin.data(), p.umax.data(), 0.1, 1e-6));
        if (walk_handle("condensed per-instance", h, n, m, N, batch)) return 1;
        almpc_destroy(h); h = nullptr;
    }
    for (int variant = 0; variant < 2; ++variant) {   // S_batch | none
        CK(almpc_create(&h, n, m, N, batch, 0, 0));
        CK(almpc_design_batched_weighted(h, Ab.data(), Bb.data(), Qb.data(), Rb.data(), variant == 0 ? Sb.data() : nullptr, nullptr, 0, p.umin.data(),
                                         p.umax.data(), 0.1, 1e-6));
        if (walk_handle("condensed weighted", h, n, m, N, batch)) return 1;
        // ... and back to shared weights on the same handle
        CK(almpc_design_batched(h, Ab.data(), Bb.data(), p.Q.data(), p.R.data(), p.S.data(), nullptr, 0, p.umin.data(), p.umax.data(), 0.1, 1e-6));
        if (walk_handle("condensed per-instance after weighted", h, n, m, N, batch)) return 1;
        almpc_destroy(h); h = nullptr;
    }
    // ---- structured handles
    for (int variant = 0; variant < 5; ++variant) {   // shared with S | shared without | per-instance with S | per-instance P | shared, R dropped
        CK(almpc_create(&h, n, m, N, batch, 0, ALMPC_FLAG_STRUCTURED));
        REFUSED(almpc_certificate(h, ALMPC_CERT_COST), ALMPC_ERR_NOT_DESIGNED);
        if (variant == 4)
            CK(almpc_design_shared(h, p.A.data(), p.B.data(), p.Q.data(), R0.data(), p.S.data(), p.P.data(), p.umin.data(), p.umax.data(), nullptr,
                                   nullptr, 0.1, 1e-6));
        else if (variant < 2)
            CK(almpc_design_shared(h, p.A.data(), p.B.data(), p.Q.data(), p.R.data(), variant == 0 ? p.S.data() : nullptr, nullptr, p.umin.data(),
                                   p.umax.data(), nullptr, nullptr, 0.1, 1e-6));
        else
            CK(almpc_design_batched(h, Ab.data(), Bb.data(), p.Q.data(), p.R.data(), variant == 2 ? p.S.data() : nullptr, variant == 2 ? nullptr : Pb.data(),
                                    variant == 3, p.umin.data(), p.umax.data(), 0.1, 1e-6));
        if (walk_handle("structured", h, n, m, N, batch)) return 1;
        almpc_destroy(h); h = nullptr;
    }
    // ---- state rows: the cost alone
    for (int variant = 0; variant < 4; ++variant) {   // state box | terminal equality, condensed | structured
        CK(almpc_create(&h, n, m, N, batch, 0, (variant & 1) ? ALMPC_FLAG_STRUCTURED : 0));
        if (variant >= 2) CK(almpc_set_terminal_equality(h, 1));
        CK(almpc_design_shared(h, p.A.data(), p.B.data(), p.Q.data(), p.R.data(), nullptr, nullptr, p.umin.data(), p.umax.data(),
                               variant < 2 ? p.xmin.data() : nullptr, variant < 2 ? p.xmax.data() : nullptr, 0.1, 1e-6));
        if (step(h, n, batch)) return 1;
        for (uint32_t want = 2; want < 16; ++want) REFUSED(almpc_certificate(h, want), ALMPC_ERR_UNSUPPORTED);
        std::vector<double> cost(batch), res(batch);
        CK(almpc_certificate(h, ALMPC_CERT_COST));
        CK(almpc_get_certificate(h, cost.data(), nullptr, nullptr, nullptr));
        REFUSED(almpc_get_certificate(h, cost.data(), res.data(), nullptr, nullptr), ALMPC_ERR_INVALID);
        almpc_destroy(h); h = nullptr;
    }
    {   // per-instance models with a state box
        CK(almpc_create(&h, n, m, N, batch, 0, 0));
        CK(almpc_set_state_box(h, p.xmin.data(), p.xmax.data()));
        CK(almpc_design_batched(h, Ab.data(), Bb.data(), p.Q.data(), p.R.data(), nullptr, nullptr, 0, p.umin.data(), p.umax.data(), 0.1, 1e-6));
        if (step(h, n, batch)) return 1;
        REFUSED(almpc_certificate(h, ALMPC_CERT_RES), ALMPC_ERR_UNSUPPORTED);
        CK(almpc_certificate(h, ALMPC_CERT_COST));
        almpc_destroy(h); h = nullptr;
    }
    // ---- time-varying designs, the SQP loop, the re-linearisation pipeline
    {
        CK(almpc_create(&h, n, m, N, batch, 0, 0));
        const std::vector<double> Aall = tiled(p.A, batch * N), Ball = tiled(p.B, batch * N);
        std::vector<double> xbar((size_t)batch * (N + 1) * n, 0.0), ubar((size_t)batch * N * m, 0.0);
        CK(almpc_design_ltv(h, Aall.data(), Ball.data(), nullptr, xbar.data(), ubar.data(), nullptr, nullptr, p.Q.data(), p.R.data(), nullptr, p.P.data(), 0,
                            p.umin.data(), p.umax.data(), 0.1, 1e-6));
        CK(almpc_calculate(h, nullptr));
        for (uint32_t want = 1; want < 16; ++want) REFUSED(almpc_certificate(h, want), ALMPC_ERR_UNSUPPORTED);
        almpc_destroy(h); h = nullptr;
    }
    {
        const int Hn = 8, L = 2;
        std::vector<double> W_in((size_t)Hn * (n + m), 0.05), W_h((size_t)L * Hn * Hn, 0.02), b_h((size_t)L * Hn, 0.01), W_out((size_t)n * Hn, 0.1);
        std::vector<double> xr((size_t)n * (N + 1), 0.0), ur((size_t)m * N, 0.0), x0((size_t)batch * n, 0.1), si(1), di(1);
        CK(almpc_create(&h, n, m, N, batch, 0, 0));
        CK(almpc_sqp_fnn_setup(h, Hn, L, 2, W_in.data(), W_h.data(), b_h.data(), W_out.data(), xr.data(), ur.data(), p.Q.data(), p.R.data(), nullptr,
                               p.P.data(), 0, p.umin.data(), p.umax.data(), 0.1, 1e-6));
        CK(almpc_sqp_fnn_start(h, x0.data(), nullptr));
        const int rc = almpc_sqp_fnn_iterate(h, 1, 1.0, nullptr, si.data(), di.data());
        if (rc != ALMPC_OK && rc != ALMPC_ERR_NUMERIC) { std::fprintf(stderr, "iterate -> %d (%s)\n", rc, almpc_last_error(h)); return 1; }
        REFUSED(almpc_certificate(h, ALMPC_CERT_COST), ALMPC_ERR_UNSUPPORTED);
        almpc_destroy(h); h = nullptr;
        CK(almpc_create(&h, n, m, N, batch, 0, 0));
        CK(almpc_relin_fnn_setup(h, Hn, L, 2, W_in.data(), W_h.data(), b_h.data(), W_out.data(), xr.data(), ur.data(), p.Q.data(), p.R.data(), nullptr,
                                 p.P.data(), p.umin.data(), p.umax.data(), 0.1, 1e-6));
        CK(almpc_update_initialization(h, x0.data()));
        CK(almpc_relin_fnn_step(h, nullptr));
        REFUSED(almpc_certificate(h, ALMPC_CERT_COST), ALMPC_ERR_UNSUPPORTED);
        almpc_destroy(h); h = nullptr;
    }
    {   // beyond the kernel's limits: m = 17
        const Plant w = chain(18, 17);
        CK(almpc_create(&h, 18, 17, 3, 4, 0, 0));
        CK(almpc_design_shared(h, w.A.data(), w.B.data(), w.Q.data(), w.R.data(), nullptr, nullptr, w.umin.data(), w.umax.data(), nullptr, nullptr, 0.1, 1e-6));
        if (step(h, 18, 4)) return 1;
        REFUSED(almpc_certificate(h, ALMPC_CERT_COST), ALMPC_ERR_UNSUPPORTED);
        almpc_destroy(h); h = nullptr;
    }
    {   // the largest slice: n = 64, m = 16 (one wave per workgroup)
        const Plant w = chain(64, 16);
        CK(almpc_create(&h, 64, 16, 2, 7, 0, 0));
        CK(almpc_design_shared(h, w.A.data(), w.B.data(), w.Q.data(), w.R.data(), w.S.data(), nullptr, w.umin.data(), w.umax.data(), nullptr, nullptr, 0.1, 1e-6));
        if (step(h, 64, 7)) return 1;
        CK(almpc_certificate(h, 15));
        almpc_destroy(h); h = nullptr;
    }
    // ---- a group of three handles, uneven shards: shared, per-instance, weighted, structured
    for (int variant = 0; variant < 4; ++variant) {
        almpc_group* g = nullptr;
        const int ids[3] = {0, 0, 0};
        std::vector<double> x0((size_t)batch * n, 0.25), cost(batch, -1.0), res(batch, -1.0), grad((size_t)batch * N * m, -1.0), lam((size_t)batch * (N + 1) * n, -1.0);
        CKG(almpc_group_create(&g, n, m, N, batch, 3, ids, variant == 3 ? ALMPC_FLAG_STRUCTURED : 0));
        if (almpc_group_certificate(g, 15) != ALMPC_ERR_NOT_DESIGNED) return 1;
        if (variant == 0 || variant == 3)
            CKG(almpc_group_design_shared(g, p.A.data(), p.B.data(), p.Q.data(), p.R.data(), p.S.data(), nullptr, p.umin.data(), p.umax.data(), nullptr, nullptr, 0.1, 1e-6));
        else if (variant == 1)
            CKG(almpc_group_design_batched(g, Ab.data(), Bb.data(), p.Q.data(), p.R.data(), p.S.data(), Pb.data(), 1, p.umin.data(), p.umax.data(), 0.1, 1e-6));
        else
            CKG(almpc_group_design_batched_weighted(g, Ab.data(), Bb.data(), Qb.data(), Rb.data(), Sb.data(), nullptr, 0, p.umin.data(), p.umax.data(), 0.1, 1e-6));
        if (almpc_group_certificate(g, 15) != ALMPC_ERR_INVALID) return 1;   // no step yet
        CKG(almpc_group_update_initialization(g, x0.data()));
        CKG(almpc_group_calculate(g, nullptr));
        if (almpc_group_certificate(g, 0) != ALMPC_ERR_INVALID || almpc_group_certificate(g, 32) != ALMPC_ERR_INVALID) return 1;
        if (almpc_group_get_certificate(g, cost.data(), nullptr, nullptr, nullptr) != ALMPC_ERR_INVALID) return 1;
        CKG(almpc_group_certificate(g, 15));
        CKG(almpc_group_get_certificate(g, cost.data(), res.data(), grad.data(), lam.data()));
        for (const std::vector<double>* v : {&cost, &res, &grad, &lam})   // (no kernel ran: the zeroed buffers, every shard's slice written)
            for (double a : *v)
                if (a != 0.0) return 1;
        CKG(almpc_group_get_certificate(g, nullptr, nullptr, nullptr, nullptr));
        CKG(almpc_group_certificate(g, ALMPC_CERT_RES));
        if (almpc_group_get_certificate(g, cost.data(), res.data(), nullptr, nullptr) != ALMPC_ERR_INVALID) return 1;
        CKG(almpc_group_get_certificate(g, nullptr, res.data(), nullptr, nullptr));
        almpc_group_destroy(g);
    }
    // ---- readers interleaved and handles redesigned; (2, 3, 4): m > n
    if (interleaved(n, m, N, batch) || interleaved(2, 3, 4, 5)) return 1;
    std::printf("cert host logic ok: %ld launches\n", fake_hip_launch_count());
    return 0;
}
