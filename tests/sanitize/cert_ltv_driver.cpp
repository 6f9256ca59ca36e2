// Driver of the CPU sanitizer build of the library's HOST half for the certificate of a step of a time-varying design
// (almpc_set_keep_stage_models, almpc_certificate_ltv, almpc_get_certificate_ltv, almpc_device_certificate_ltv) and of the
// re-linearisation pipeline (almpc_relin_fnn_certificate, almpc_group_relin_fnn_certificate): csrc/almpc_api.hip compiled host-only under
// AddressSanitizer + UndefinedBehaviorSanitizer and linked against tests/sanitize/fake_hip_runtime.cpp, as cert_driver.cpp is (device
// memory = calloc'd host memory, launches = no-ops, so every buffer the calls size, upload and read back is bounds-checked).  Walks every
// new entry point, every `want` mask with every combination of null outputs, every refusal, the keep switch on and off, a redesign, with
// and without defects, S and a P per instance, state rows, and the pipeline's forms on condensed and structured handles and a group of
// three.  Prints "cert ltv host logic ok: <launches> launches".
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

// the arguments of almpc_design_ltv for `batch` copies of a plant
struct Ltv {
    std::vector<double> A, B, c, xbar, ubar, xref, uref, Pb;
    Ltv(const Plant& p, int N, int batch)
        : A(tiled(p.A, batch * N)), B(tiled(p.B, batch * N)), c((size_t)batch * N * p.n, 0.01), xbar((size_t)batch * (N + 1) * p.n, 0.2),
          ubar((size_t)batch * N * p.m, 0.1), xref((size_t)(N + 1) * p.n, 0.05), uref((size_t)N * p.m, 0.02), Pb(tiled(p.P, batch)) {}
};

// variant bits: 1 no defects, 2 no S, 4 a P per instance, 8 no references
static int design(almpc_handle* h, const Plant& p, const Ltv& a, int variant, const double* R = nullptr) {
    return almpc_design_ltv(h, a.A.data(), a.B.data(), (variant & 1) ? nullptr : a.c.data(), a.xbar.data(), a.ubar.data(), (variant & 8) ? nullptr : a.xref.data(),
                            (variant & 8) ? nullptr : a.uref.data(), p.Q.data(), R ? R : p.R.data(), (variant & 2) ? nullptr : p.S.data(),
                            (variant & 4) ? a.Pb.data() : p.P.data(), (variant & 4) ? 1 : 0, p.umin.data(), p.umax.data(), 0.1, 1e-6);
}

// every mask on a stepped handle, the getter with every combination of null outputs, the device view
static int masks(almpc_handle* h, int n, int m, int N, int batch, uint32_t served) {
    std::vector<double> cost(batch), res(batch), grad((size_t)batch * N * m), lam((size_t)batch * (N + 1) * n), x(lam.size()), ex(lam.size());
    for (uint32_t want = 1; want < 32; ++want) {
        if (want & ~served) { REFUSED(almpc_certificate_ltv(h, want), ALMPC_ERR_UNSUPPORTED); continue; }
        CK(almpc_certificate_ltv(h, want));
        for (uint32_t ask = 0; ask < 64; ++ask) {   // bit 4: x, bit 5: e_x (both belong to ALMPC_CERT_STATES)
            const uint32_t need = (ask & 15u) | ((ask & 48u) ? ALMPC_CERT_STATES : 0u);
            const int rc = almpc_get_certificate_ltv(h, (ask & 1) ? cost.data() : nullptr, (ask & 2) ? res.data() : nullptr, (ask & 4) ? grad.data() : nullptr,
                                                     (ask & 8) ? lam.data() : nullptr, (ask & 16) ? x.data() : nullptr, (ask & 32) ? ex.data() : nullptr);
            if (rc != ((need & ~want) ? ALMPC_ERR_INVALID : ALMPC_OK)) { std::fprintf(stderr, "get_certificate_ltv want %u ask %u -> %d\n", want, ask, rc); return 1; }
        }
        const double* d[6];
        for (auto& q : d) q = cost.data();
        CK(almpc_device_certificate_ltv(h, &d[0], &d[1], &d[2], &d[3], &d[4], &d[5]));
        for (int k = 0; k < 6; ++k)
            if (!!d[k] != !!(want & (k < 4 ? (1u << k) : ALMPC_CERT_STATES))) return 1;
        CK(almpc_device_certificate_ltv(h, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    }
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
    EXPECT(almpc_set_keep_stage_models(nullptr, 1), ALMPC_ERR_INVALID);
    EXPECT(almpc_certificate_ltv(nullptr, 1), ALMPC_ERR_INVALID);
    EXPECT(almpc_get_certificate_ltv(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), ALMPC_ERR_INVALID);
    EXPECT(almpc_device_certificate_ltv(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), ALMPC_ERR_INVALID);
    EXPECT(almpc_relin_fnn_certificate(nullptr, 1), ALMPC_ERR_INVALID);
    EXPECT(almpc_group_relin_fnn_certificate(nullptr, 1), ALMPC_ERR_INVALID);
    const int n = 5, m = 2, N = 9, batch = 19;
    const Plant p = chain(n, m);
    const Ltv a(p, N, batch);
    std::vector<double> R0 = p.R;
    R0[0] = 0.0;   // the branch rule drops R and S
    std::vector<double> cost(batch), res(batch);
    // ---- time-varying designs with the keep switch on
    for (int variant = 0; variant < 16; ++variant) {
        CK(almpc_create(&h, n, m, N, batch, 0, 0));
        REFUSED(almpc_certificate_ltv(h, ALMPC_CERT_COST), ALMPC_ERR_NOT_DESIGNED);
        CK(almpc_set_keep_stage_models(h, 1));
        CK(design(h, p, a, variant, variant == 5 ? R0.data() : nullptr));
        REFUSED(almpc_certificate_ltv(h, ALMPC_CERT_COST), ALMPC_ERR_INVALID);   // designed, no step yet
        REFUSED(almpc_get_certificate_ltv(h, cost.data(), nullptr, nullptr, nullptr, nullptr, nullptr), ALMPC_ERR_INVALID);
        REFUSED(almpc_device_certificate_ltv(h, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), ALMPC_ERR_INVALID);
        CK(almpc_calculate(h, nullptr));
        REFUSED(almpc_certificate_ltv(h, 0), ALMPC_ERR_INVALID);
        REFUSED(almpc_certificate_ltv(h, 32), ALMPC_ERR_INVALID);
        REFUSED(almpc_certificate_ltv(h, 0x80000001u), ALMPC_ERR_INVALID);
        REFUSED(almpc_certificate(h, ALMPC_CERT_COST), ALMPC_ERR_UNSUPPORTED);   // almpc_certificate keeps refusing the design
        REFUSED(almpc_relin_fnn_certificate(h, ALMPC_CERT_COST), ALMPC_ERR_UNSUPPORTED);
        if (masks(h, n, m, N, batch, 31u)) return 1;
        CK(almpc_calculate(h, nullptr));   // a new step voids the certificate of the last one
        REFUSED(almpc_get_certificate_ltv(h, cost.data(), nullptr, nullptr, nullptr, nullptr, nullptr), ALMPC_ERR_INVALID);
        CK(almpc_certificate_ltv(h, ALMPC_CERT_COST | ALMPC_CERT_RES));
        CK(almpc_get_certificate_ltv(h, cost.data(), res.data(), nullptr, nullptr, nullptr, nullptr));
        // a redesign (the switch stays on), other arguments: no step of it yet
        CK(design(h, p, a, variant ^ 15));
        REFUSED(almpc_get_certificate_ltv(h, cost.data(), nullptr, nullptr, nullptr, nullptr, nullptr), ALMPC_ERR_INVALID);
        REFUSED(almpc_certificate_ltv(h, ALMPC_CERT_COST), ALMPC_ERR_INVALID);
        CK(almpc_calculate(h, nullptr));
        CK(almpc_certificate_ltv(h, 31));
        // the switch off: the next design releases its stage models
        CK(almpc_set_keep_stage_models(h, 0));
        CK(almpc_certificate_ltv(h, 31));   // (read by the next design only)
        CK(design(h, p, a, variant));
        CK(almpc_calculate(h, nullptr));
        REFUSED(almpc_certificate_ltv(h, ALMPC_CERT_COST), ALMPC_ERR_INVALID);
        if (!std::strstr(almpc_last_error(h), "almpc_set_keep_stage_models")) return 1;
        // ... and on again
        CK(almpc_set_keep_stage_models(h, 7));
        CK(design(h, p, a, variant));
        CK(almpc_calculate(h, nullptr));
        CK(almpc_certificate_ltv(h, 31));
        // a time-invariant design on the same handle
        CK(almpc_design_shared(h, p.A.data(), p.B.data(), p.Q.data(), p.R.data(), nullptr, nullptr, p.umin.data(), p.umax.data(), nullptr, nullptr, 0.1, 1e-6));
        std::vector<double> x0((size_t)batch * n, 0.25);
        CK(almpc_update_initialization(h, x0.data()));
        CK(almpc_calculate(h, nullptr));
        REFUSED(almpc_certificate_ltv(h, ALMPC_CERT_COST), ALMPC_ERR_UNSUPPORTED);
        if (!std::strstr(almpc_last_error(h), "almpc_certificate")) return 1;
        REFUSED(almpc_relin_fnn_certificate(h, ALMPC_CERT_COST), ALMPC_ERR_UNSUPPORTED);
        CK(almpc_certificate(h, 15));
        almpc_destroy(h); h = nullptr;
    }
    // ---- state rows: the cost and the states (keep on or off, the design keeps its stage models for the step; the switch decides)
    for (int variant = 0; variant < 2; ++variant) {   // state box | terminal equality
        CK(almpc_create(&h, n, m, N, batch, 0, 0));
        if (variant == 0) CK(almpc_set_state_box(h, p.xmin.data(), p.xmax.data()));
        else CK(almpc_set_terminal_equality(h, 1));
        CK(design(h, p, a, 0));
        CK(almpc_calculate(h, nullptr));
        REFUSED(almpc_certificate_ltv(h, ALMPC_CERT_COST), ALMPC_ERR_INVALID);   // the switch was off
        CK(almpc_set_keep_stage_models(h, 1));
        CK(design(h, p, a, 0));
        CK(almpc_calculate(h, nullptr));
        if (masks(h, n, m, N, batch, ALMPC_CERT_COST | ALMPC_CERT_STATES)) return 1;
        almpc_destroy(h); h = nullptr;
    }
    {   // beyond the shapes of an LTV step: n = 18
        const Plant w = chain(18, 1);
        const Ltv aw(w, 3, 4);
        CK(almpc_create(&h, 18, 1, 3, 4, 0, 0));
        CK(almpc_set_keep_stage_models(h, 1));
        CK(design(h, w, aw, 0));
        const int rc = almpc_calculate(h, nullptr);   // (the step itself refuses the shape: the certificate's refusal does not wait for it)
        if (rc != ALMPC_OK && rc != ALMPC_ERR_UNSUPPORTED) return 1;
        REFUSED(almpc_certificate_ltv(h, ALMPC_CERT_COST), ALMPC_ERR_UNSUPPORTED);
        almpc_destroy(h); h = nullptr;
    }
    // ---- the SQP loop stays without a certificate; the re-linearisation pipeline has its own
    const int Hn = 8, L = 2;
    std::vector<double> W_in((size_t)Hn * (n + m), 0.05), W_h((size_t)L * Hn * Hn, 0.02), b_h((size_t)L * Hn, 0.01), W_out((size_t)n * Hn, 0.1);
    std::vector<double> xr((size_t)n * (N + 1), 0.0), ur((size_t)m * N, 0.0), x0((size_t)batch * n, 0.1), si(1), di(1);
    std::vector<double> grad((size_t)batch * N * m, -1.0), lam((size_t)batch * (N + 1) * n, -1.0);
    {
        CK(almpc_create(&h, n, m, N, batch, 0, 0));
        CK(almpc_set_keep_stage_models(h, 1));
        CK(almpc_sqp_fnn_setup(h, Hn, L, 2, W_in.data(), W_h.data(), b_h.data(), W_out.data(), xr.data(), ur.data(), p.Q.data(), p.R.data(), nullptr,
                               p.P.data(), 0, p.umin.data(), p.umax.data(), 0.1, 1e-6));
        CK(almpc_sqp_fnn_start(h, x0.data(), nullptr));
        const int rc = almpc_sqp_fnn_iterate(h, 1, 1.0, nullptr, si.data(), di.data());
        if (rc != ALMPC_OK && rc != ALMPC_ERR_NUMERIC) { std::fprintf(stderr, "iterate -> %d (%s)\n", rc, almpc_last_error(h)); return 1; }
        REFUSED(almpc_certificate_ltv(h, ALMPC_CERT_COST), ALMPC_ERR_UNSUPPORTED);
        REFUSED(almpc_relin_fnn_certificate(h, ALMPC_CERT_COST), ALMPC_ERR_UNSUPPORTED);
        almpc_destroy(h); h = nullptr;
    }
    for (int variant = 0; variant < 6; ++variant) {   // condensed | structured, x (plain | S | one P per step)
        const bool structured = variant & 1;
        CK(almpc_create(&h, n, m, N, batch, 0, structured ? ALMPC_FLAG_STRUCTURED : 0));
        REFUSED(almpc_relin_fnn_certificate(h, ALMPC_CERT_COST), ALMPC_ERR_NOT_DESIGNED);
        if (variant >= 4) CK(almpc_set_terminal_weight(h, ALMPC_TERMINAL_DARE_DEVICE));
        CK(almpc_relin_fnn_setup(h, Hn, L, 2, W_in.data(), W_h.data(), b_h.data(), W_out.data(), xr.data(), ur.data(), p.Q.data(), p.R.data(),
                                 (variant & 2) ? p.S.data() : nullptr, p.P.data(), p.umin.data(), p.umax.data(), 0.1, 1e-6));
        CK(almpc_update_initialization(h, x0.data()));
        REFUSED(almpc_relin_fnn_certificate(h, ALMPC_CERT_COST), ALMPC_ERR_INVALID);   // set up, no step yet
        CK(almpc_relin_fnn_step(h, nullptr));
        REFUSED(almpc_relin_fnn_certificate(h, 0), ALMPC_ERR_INVALID);
        REFUSED(almpc_relin_fnn_certificate(h, 16), ALMPC_ERR_INVALID);
        REFUSED(almpc_certificate(h, ALMPC_CERT_COST), ALMPC_ERR_UNSUPPORTED);       // almpc_certificate keeps refusing the pipeline
        REFUSED(almpc_certificate_ltv(h, ALMPC_CERT_COST), ALMPC_ERR_UNSUPPORTED);
        for (uint32_t want = 1; want < 16; ++want) {
            CK(almpc_relin_fnn_certificate(h, want));
            for (uint32_t ask = 0; ask < 16; ++ask) {
                const int rc = almpc_get_certificate(h, (ask & 1) ? cost.data() : nullptr, (ask & 2) ? res.data() : nullptr, (ask & 4) ? grad.data() : nullptr,
                                                     (ask & 8) ? lam.data() : nullptr);
                if (rc != ((ask & ~want) ? ALMPC_ERR_INVALID : ALMPC_OK)) return 1;
            }
            CK(almpc_device_certificate(h, nullptr, nullptr, nullptr, nullptr));
        }
        CK(almpc_relin_fnn_advance(h));
        almpc_opts o;
        almpc_default_opts(&o);
        o.warm_start = 1;
        CK(almpc_relin_fnn_step(h, &o));
        REFUSED(almpc_get_certificate(h, cost.data(), nullptr, nullptr, nullptr), ALMPC_ERR_INVALID);   // a new step
        CK(almpc_relin_fnn_certificate(h, 15));
        CK(almpc_get_certificate(h, cost.data(), res.data(), grad.data(), lam.data()));
        // a new setup voids the uploaded weights
        CK(almpc_relin_fnn_setup(h, Hn, L, 2, W_in.data(), W_h.data(), b_h.data(), W_out.data(), xr.data(), ur.data(), p.Q.data(), p.R.data(), p.S.data(),
                                 p.P.data(), p.umin.data(), p.umax.data(), 0.1, 1e-6));
        REFUSED(almpc_relin_fnn_certificate(h, ALMPC_CERT_COST), ALMPC_ERR_INVALID);
        CK(almpc_update_initialization(h, x0.data()));
        CK(almpc_relin_fnn_step(h, nullptr));
        CK(almpc_relin_fnn_certificate(h, 15));
        almpc_destroy(h); h = nullptr;
    }
    {   // the pipeline with a state box: the cost alone
        CK(almpc_create(&h, n, m, N, batch, 0, 0));
        CK(almpc_set_state_box(h, p.xmin.data(), p.xmax.data()));
        CK(almpc_relin_fnn_setup(h, Hn, L, 2, W_in.data(), W_h.data(), b_h.data(), W_out.data(), xr.data(), ur.data(), p.Q.data(), p.R.data(), nullptr,
                                 p.P.data(), p.umin.data(), p.umax.data(), 0.1, 1e-6));
        CK(almpc_update_initialization(h, x0.data()));
        CK(almpc_relin_fnn_step(h, nullptr));
        for (uint32_t want = 2; want < 16; ++want) REFUSED(almpc_relin_fnn_certificate(h, want), ALMPC_ERR_UNSUPPORTED);
        CK(almpc_relin_fnn_certificate(h, ALMPC_CERT_COST));
        almpc_destroy(h); h = nullptr;
    }
    // ---- the pipeline, a plain design and the pipeline again on one handle (also m > n: the offsets in the one device copy of the
    // weights are not symmetric); then a time-varying design and a plain one: the getters of the form that did not fill the buffers
    for (int variant = 0; variant < 4; ++variant) {   // condensed | structured, x (5, 2, 9) | (2, 3, 4)
        const bool wide = variant & 2;
        const int n2 = wide ? 2 : n, m2 = wide ? 3 : m, N2 = wide ? 4 : N, b2 = wide ? 5 : batch;
        const Plant w = chain(n2, m2);
        Plant v = w;
        for (double& q : v.Q) q *= 3.0;
        for (double& q : v.S) q *= 0.5;
        std::vector<double> W2_in((size_t)Hn * (n2 + m2), 0.05), W2_out((size_t)n2 * Hn, 0.1), xr2((size_t)n2 * (N2 + 1), 0.0), ur2((size_t)m2 * N2, 0.0);
        std::vector<double> x2((size_t)b2 * n2, 0.1), lam2((size_t)b2 * (N2 + 1) * n2), grad2((size_t)b2 * N2 * m2);
        CK(almpc_create(&h, n2, m2, N2, b2, 0, (variant & 1) ? ALMPC_FLAG_STRUCTURED : 0));
        for (int pass = 0; pass < 2; ++pass) {
            const Plant& u = pass ? v : w;
            CK(almpc_relin_fnn_setup(h, Hn, L, 2, W2_in.data(), W_h.data(), b_h.data(), W2_out.data(), xr2.data(), ur2.data(), u.Q.data(), u.R.data(), u.S.data(),
                                     u.P.data(), u.umin.data(), u.umax.data(), 0.1, 1e-6));
            CK(almpc_update_initialization(h, x2.data()));
            CK(almpc_relin_fnn_step(h, nullptr));
            CK(almpc_relin_fnn_certificate(h, 15));
            CK(almpc_get_certificate(h, cost.data(), res.data(), grad2.data(), lam2.data()));
            REFUSED(almpc_get_certificate_ltv(h, cost.data(), nullptr, nullptr, nullptr, nullptr, nullptr), ALMPC_ERR_INVALID);
            CK(almpc_relin_fnn_step(h, nullptr));   // (a step's redesign: the weights go to the device again)
            CK(almpc_relin_fnn_certificate(h, 15));
            if (pass) break;
            CK(almpc_design_shared(h, w.A.data(), w.B.data(), v.Q.data(), w.R.data(), v.S.data(), w.P.data(), w.umin.data(), w.umax.data(), nullptr, nullptr, 0.1, 1e-6));
            CK(almpc_update_initialization(h, x2.data()));
            CK(almpc_calculate(h, nullptr));
            REFUSED(almpc_relin_fnn_certificate(h, 15), ALMPC_ERR_UNSUPPORTED);
            CK(almpc_certificate(h, 15));
            CK(almpc_get_certificate(h, cost.data(), res.data(), grad2.data(), lam2.data()));
        }
        almpc_destroy(h); h = nullptr;
    }
    {
        std::vector<double> x((size_t)batch * (N + 1) * n), xs((size_t)batch * n, 0.25);
        const double* d[6];
        CK(almpc_create(&h, n, m, N, batch, 0, 0));
        CK(almpc_set_keep_stage_models(h, 1));
        CK(design(h, p, a, 0));
        CK(almpc_calculate(h, nullptr));
        CK(almpc_certificate_ltv(h, 31));
        CK(almpc_get_certificate_ltv(h, cost.data(), res.data(), grad.data(), lam.data(), x.data(), nullptr));
        REFUSED(almpc_get_certificate(h, cost.data(), nullptr, nullptr, nullptr), ALMPC_ERR_INVALID);
        REFUSED(almpc_device_certificate(h, &d[0], &d[1], &d[2], &d[3]), ALMPC_ERR_INVALID);
        CK(almpc_design_shared(h, p.A.data(), p.B.data(), p.Q.data(), p.R.data(), p.S.data(), nullptr, p.umin.data(), p.umax.data(), nullptr, nullptr, 0.1, 1e-6));
        CK(almpc_update_initialization(h, xs.data()));
        CK(almpc_calculate(h, nullptr));
        CK(almpc_certificate(h, 15));
        CK(almpc_get_certificate(h, cost.data(), res.data(), grad.data(), lam.data()));
        REFUSED(almpc_get_certificate_ltv(h, cost.data(), nullptr, nullptr, nullptr, nullptr, nullptr), ALMPC_ERR_INVALID);
        REFUSED(almpc_device_certificate_ltv(h, &d[0], &d[1], &d[2], &d[3], &d[4], &d[5]), ALMPC_ERR_INVALID);
        CK(almpc_calculate(h, nullptr));   // a new step voids both
        REFUSED(almpc_get_certificate(h, cost.data(), nullptr, nullptr, nullptr), ALMPC_ERR_INVALID);
        REFUSED(almpc_get_certificate_ltv(h, cost.data(), nullptr, nullptr, nullptr, nullptr, nullptr), ALMPC_ERR_INVALID);
        almpc_destroy(h); h = nullptr;
    }
    // ---- a group of three handles, uneven shards: condensed, structured
    for (int variant = 0; variant < 2; ++variant) {
        almpc_group* g = nullptr;
        const int ids[3] = {0, 0, 0};
        std::fill(cost.begin(), cost.end(), -1.0); std::fill(res.begin(), res.end(), -1.0);
        CKG(almpc_group_create(&g, n, m, N, batch, 3, ids, variant == 1 ? ALMPC_FLAG_STRUCTURED : 0));
        if (almpc_group_relin_fnn_certificate(g, 15) != ALMPC_ERR_NOT_DESIGNED) return 1;
        CKG(almpc_group_relin_fnn_setup(g, Hn, L, 2, W_in.data(), W_h.data(), b_h.data(), W_out.data(), xr.data(), ur.data(), p.Q.data(), p.R.data(), p.S.data(),
                                        p.P.data(), p.umin.data(), p.umax.data(), 0.1, 1e-6));
        CKG(almpc_group_update_initialization(g, x0.data()));
        if (almpc_group_relin_fnn_certificate(g, 15) != ALMPC_ERR_INVALID) return 1;   // no step yet
        CKG(almpc_group_relin_fnn_step(g, nullptr));
        if (almpc_group_relin_fnn_certificate(g, 0) != ALMPC_ERR_INVALID || almpc_group_relin_fnn_certificate(g, 16) != ALMPC_ERR_INVALID) return 1;
        if (almpc_group_certificate(g, 15) != ALMPC_ERR_UNSUPPORTED) return 1;
        CKG(almpc_group_relin_fnn_certificate(g, 15));
        CKG(almpc_group_get_certificate(g, cost.data(), res.data(), grad.data(), lam.data()));
        for (const std::vector<double>* v : {&cost, &res, &grad, &lam})   // (no kernel ran: the zeroed buffers, every shard's slice written)
            for (double q : *v)
                if (q != 0.0) return 1;
        CKG(almpc_group_relin_fnn_certificate(g, ALMPC_CERT_RES));
        if (almpc_group_get_certificate(g, cost.data(), res.data(), nullptr, nullptr) != ALMPC_ERR_INVALID) return 1;
        CKG(almpc_group_get_certificate(g, nullptr, res.data(), nullptr, nullptr));
        almpc_group_destroy(g);
    }
    std::printf("cert ltv host logic ok: %ld launches\n", fake_hip_launch_count());
    return 0;
}
