// Driver of the CPU sanitizer build of the library's HOST half for the sensitivities of a step of a time-varying design
// (almpc_sensitivity_ltv, almpc_sensitivity_ltv_vjp): csrc/almpc_api.hip compiled host-only under AddressSanitizer +
// UndefinedBehaviorSanitizer and linked against tests/sanitize/fake_hip_runtime.cpp, as cert_ltv_driver.cpp is (device memory = calloc'd
// host memory, launches = no-ops, so every buffer the calls size, upload and read back is bounds-checked).  Walks both entry points,
// every `want` mask with every combination of null outputs of the getter, a NULL g_x and a NULL rows, every refusal, the keep switch on
// and off, a redesign, with and without defects, S, R and a P per instance, state rows, a shape beyond the served ones, the designs
// of other kinds (whose own sensitivity calls keep refusing a time-varying design and name the new call), the (12, 4) builds.
// Prints "sens ltv host logic ok: <launches> launches".
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
// ... and names something
#define NAMES(call, want, text)                                                                              \
    do {                                                                                                     \
        REFUSED(call, want);                                                                                 \
        if (!std::strstr(almpc_last_error(h), text)) { std::fprintf(stderr, "%s:%d \"%s\" does not name %s\n", __FILE__, __LINE__, almpc_last_error(h), text); return 1; } \
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
    for (int a = 0; a < m; ++a) { p.B[(size_t)a * n + (n - 1 - a % n)] = 0.5; p.R[(size_t)a * m + a] = 0.1; p.S[(size_t)a * m + a] = 2.0; }
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

// exactly sized outputs of both calls: an overrun of any of them is the sanitizer's to find
struct Out {
    std::vector<double> K0, dU, dX, g_u, g_x, g_x0;
    std::vector<int32_t> rows;
    Out(int n, int m, int N, int batch)
        : K0((size_t)batch * n * m), dU((size_t)batch * n * N * m), dX((size_t)batch * n * (N + 1) * n), g_u((size_t)batch * N * m, 0.5),
          g_x((size_t)batch * (N + 1) * n, -0.25), g_x0((size_t)batch * n), rows(batch) {}
};

// every mask on a stepped handle, the getter with every combination of null outputs, the device view, the VJP in its four forms
static int walk(almpc_handle* h, Out& o) {
    for (uint32_t want = 1; want < 8; ++want) {
        CK(almpc_sensitivity_ltv(h, want, want & 1 ? 0.0 : 1e-6));
        const uint32_t have = want | ((want & ALMPC_SENS_DX) ? ALMPC_SENS_DU : 0u);   // (the forward pass writes dU on its way to dX)
        for (uint32_t ask = 0; ask < 16; ++ask) {
            const int rc = almpc_get_sensitivity(h, (ask & 1) ? o.K0.data() : nullptr, (ask & 2) ? o.dU.data() : nullptr, (ask & 4) ? o.dX.data() : nullptr,
                                                 (ask & 8) ? o.rows.data() : nullptr);
            if (rc != (((ask & 7u) & ~have) ? ALMPC_ERR_INVALID : ALMPC_OK)) { std::fprintf(stderr, "get_sensitivity want %u ask %u -> %d\n", want, ask, rc); return 1; }
        }
        const double* d[3];
        const int32_t* dr = nullptr;
        CK(almpc_device_sensitivity(h, &d[0], &d[1], &d[2], &dr));
        for (int k = 0; k < 3; ++k)
            if (!!d[k] != !!(have & (1u << k))) return 1;
        if (!dr) return 1;
    }
    CK(almpc_sensitivity_ltv_vjp(h, o.g_u.data(), o.g_x.data(), 0.0, o.g_x0.data(), o.rows.data()));
    CK(almpc_sensitivity_ltv_vjp(h, o.g_u.data(), nullptr, 0.0, o.g_x0.data(), o.rows.data()));
    CK(almpc_sensitivity_ltv_vjp(h, o.g_u.data(), o.g_x.data(), 1e-6, o.g_x0.data(), nullptr));
    CK(almpc_sensitivity_ltv_vjp(h, o.g_u.data(), nullptr, -1.0, o.g_x0.data(), nullptr));
    for (double q : o.g_x0)   // (no kernel ran: the zeroed device buffer came back whole)
        if (q != 0.0) return 1;
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
    EXPECT(almpc_sensitivity_ltv(nullptr, 1, 0.0), ALMPC_ERR_INVALID);
    EXPECT(almpc_sensitivity_ltv_vjp(nullptr, nullptr, nullptr, 0.0, nullptr, nullptr), ALMPC_ERR_INVALID);
    const int n = 5, m = 2, N = 9, batch = 19;
    const Plant p = chain(n, m);
    const Ltv a(p, N, batch);
    Out o(n, m, N, batch);
    std::vector<double> R0 = p.R;
    R0[0] = 0.0;   // the branch rule drops R and S
    // ---- time-varying designs with the keep switch on: with S (k_sens_ltv<.., true, ..>) and without
    for (int variant = 0; variant < 16; ++variant) {
        CK(almpc_create(&h, n, m, N, batch, 0, 0));
        REFUSED(almpc_sensitivity_ltv(h, ALMPC_SENS_K0, 0.0), ALMPC_ERR_NOT_DESIGNED);
        REFUSED(almpc_sensitivity_ltv_vjp(h, o.g_u.data(), nullptr, 0.0, o.g_x0.data(), nullptr), ALMPC_ERR_NOT_DESIGNED);
        CK(almpc_set_keep_stage_models(h, 1));
        CK(design(h, p, a, variant, variant == 5 ? R0.data() : nullptr));
        REFUSED(almpc_sensitivity_ltv(h, ALMPC_SENS_K0, 0.0), ALMPC_ERR_INVALID);   // designed, no step yet
        REFUSED(almpc_sensitivity_ltv_vjp(h, o.g_u.data(), nullptr, 0.0, o.g_x0.data(), nullptr), ALMPC_ERR_INVALID);
        CK(almpc_calculate(h, nullptr));
        REFUSED(almpc_sensitivity_ltv(h, 0, 0.0), ALMPC_ERR_INVALID);
        REFUSED(almpc_sensitivity_ltv(h, 8, 0.0), ALMPC_ERR_INVALID);
        REFUSED(almpc_sensitivity_ltv(h, 0x80000001u, 0.0), ALMPC_ERR_INVALID);
        REFUSED(almpc_sensitivity_ltv_vjp(h, nullptr, o.g_x.data(), 0.0, o.g_x0.data(), o.rows.data()), ALMPC_ERR_INVALID);
        REFUSED(almpc_sensitivity_ltv_vjp(h, o.g_u.data(), o.g_x.data(), 0.0, nullptr, o.rows.data()), ALMPC_ERR_INVALID);
        REFUSED(almpc_get_sensitivity(h, o.K0.data(), nullptr, nullptr, nullptr), ALMPC_ERR_INVALID);   // nothing computed yet
        // the calls of the other designs keep refusing this one, and name the call that serves it
        NAMES(almpc_sensitivity(h, ALMPC_SENS_K0, 0.0), ALMPC_ERR_UNSUPPORTED, "almpc_sensitivity_ltv");
        NAMES(almpc_sensitivity_rows(h, ALMPC_SENS_K0, 0.0, 0.0), ALMPC_ERR_UNSUPPORTED, "almpc_sensitivity_ltv");
        NAMES(almpc_sensitivity_vjp(h, o.g_u.data(), nullptr, 0.0, o.g_x0.data(), nullptr), ALMPC_ERR_UNSUPPORTED, "almpc_sensitivity_ltv");
        NAMES(almpc_sensitivity_stagewise(h, ALMPC_SENS_K0, 0.0), ALMPC_ERR_UNSUPPORTED, "almpc_sensitivity_ltv");
        NAMES(almpc_sensitivity_stagewise_rate_vjp(h, o.g_u.data(), nullptr, 0.0, o.g_x0.data(), nullptr), ALMPC_ERR_UNSUPPORTED, "almpc_sensitivity_ltv");
        if (walk(h, o)) return 1;
        CK(almpc_certificate_ltv(h, 31));   // (the certificate of the same step beside them)
        CK(almpc_get_sensitivity(h, nullptr, nullptr, nullptr, o.rows.data()));
        CK(almpc_calculate(h, nullptr));   // a new step voids the sensitivities of the last one
        REFUSED(almpc_get_sensitivity(h, o.K0.data(), nullptr, nullptr, nullptr), ALMPC_ERR_INVALID);
        REFUSED(almpc_device_sensitivity(h, nullptr, nullptr, nullptr, nullptr), ALMPC_ERR_INVALID);
        CK(almpc_sensitivity_ltv(h, ALMPC_SENS_K0, 0.0));
        CK(almpc_get_sensitivity(h, o.K0.data(), nullptr, nullptr, o.rows.data()));
        // a redesign (the switch stays on), other arguments -- the other RATE build, another width of the gain scratch: no step of it yet
        CK(design(h, p, a, variant ^ 15));
        REFUSED(almpc_get_sensitivity(h, o.K0.data(), nullptr, nullptr, nullptr), ALMPC_ERR_INVALID);
        REFUSED(almpc_sensitivity_ltv(h, ALMPC_SENS_K0, 0.0), ALMPC_ERR_INVALID);
        CK(almpc_calculate(h, nullptr));
        if (walk(h, o)) return 1;
        // the switch off: the next design releases its stage models
        CK(almpc_set_keep_stage_models(h, 0));
        CK(almpc_sensitivity_ltv(h, 7, 0.0));   // (read by the next design only)
        CK(design(h, p, a, variant));
        CK(almpc_calculate(h, nullptr));
        NAMES(almpc_sensitivity_ltv(h, ALMPC_SENS_K0, 0.0), ALMPC_ERR_INVALID, "almpc_set_keep_stage_models");
        NAMES(almpc_sensitivity_ltv_vjp(h, o.g_u.data(), nullptr, 0.0, o.g_x0.data(), nullptr), ALMPC_ERR_INVALID, "almpc_set_keep_stage_models");
        // ... and on again
        CK(almpc_set_keep_stage_models(h, 7));
        CK(design(h, p, a, variant));
        CK(almpc_calculate(h, nullptr));
        CK(almpc_sensitivity_ltv(h, 7, 0.0));
        // a time-invariant design on the same handle: the message names the call that serves it
        CK(almpc_design_shared(h, p.A.data(), p.B.data(), p.Q.data(), p.R.data(), nullptr, nullptr, p.umin.data(), p.umax.data(), nullptr, nullptr, 0.1, 1e-6));
        std::vector<double> x0((size_t)batch * n, 0.25);
        CK(almpc_update_initialization(h, x0.data()));
        CK(almpc_calculate(h, nullptr));
        NAMES(almpc_sensitivity_ltv(h, ALMPC_SENS_K0, 0.0), ALMPC_ERR_UNSUPPORTED, "almpc_sensitivity");
        NAMES(almpc_sensitivity_ltv_vjp(h, o.g_u.data(), nullptr, 0.0, o.g_x0.data(), nullptr), ALMPC_ERR_UNSUPPORTED, "almpc_design_ltv");
        CK(almpc_sensitivity(h, 7, 0.0));
        almpc_destroy(h); h = nullptr;
    }
    // ---- state rows: refused, keep on or off
    for (int variant = 0; variant < 2; ++variant) {   // state box | terminal equality
        CK(almpc_create(&h, n, m, N, batch, 0, 0));
        if (variant == 0) CK(almpc_set_state_box(h, p.xmin.data(), p.xmax.data()));
        else CK(almpc_set_terminal_equality(h, 1));
        CK(almpc_set_keep_stage_models(h, 1));
        CK(design(h, p, a, 0));
        CK(almpc_calculate(h, nullptr));
        NAMES(almpc_sensitivity_ltv(h, ALMPC_SENS_K0, 0.0), ALMPC_ERR_UNSUPPORTED, "state rows");
        NAMES(almpc_sensitivity_ltv_vjp(h, o.g_u.data(), nullptr, 0.0, o.g_x0.data(), nullptr), ALMPC_ERR_UNSUPPORTED, "state rows");
        almpc_destroy(h); h = nullptr;
    }
    {   // beyond the shapes of an LTV step: n = 18
        const Plant w = chain(18, 1);
        const Ltv aw(w, 3, 4);
        Out ow(18, 1, 3, 4);
        CK(almpc_create(&h, 18, 1, 3, 4, 0, 0));
        CK(almpc_set_keep_stage_models(h, 1));
        CK(design(h, w, aw, 0));
        const int rc = almpc_calculate(h, nullptr);   // (the step itself refuses the shape: the refusal here does not wait for it)
        if (rc != ALMPC_OK && rc != ALMPC_ERR_UNSUPPORTED) return 1;
        NAMES(almpc_sensitivity_ltv(h, ALMPC_SENS_K0, 0.0), ALMPC_ERR_UNSUPPORTED, "n <= 16");
        NAMES(almpc_sensitivity_ltv_vjp(h, ow.g_u.data(), nullptr, 0.0, ow.g_x0.data(), nullptr), ALMPC_ERR_UNSUPPORTED, "n <= 16");
        almpc_destroy(h); h = nullptr;
    }
    // ---- the (12, 4) builds, the largest stage (16, 16, 31: two waves of the rate kernel per workgroup), N = 1
    for (int variant = 0; variant < 6; ++variant) {
        const int n2 = variant < 2 ? 12 : variant < 4 ? 16 : 3, m2 = variant < 2 ? 4 : variant < 4 ? 16 : 2, N2 = variant < 2 ? 7 : variant < 4 ? 8 : 1, b2 = 6;
        const Plant w = chain(n2, m2);
        const Ltv aw(w, N2, b2);
        Out ow(n2, m2, N2, b2);
        CK(almpc_create(&h, n2, m2, N2, b2, 0, 0));
        CK(almpc_set_keep_stage_models(h, 1));
        CK(design(h, w, aw, (variant & 1) ? 2 : 0));
        CK(almpc_calculate(h, nullptr));
        if (walk(h, ow)) return 1;
        almpc_destroy(h); h = nullptr;
    }
    // ---- structured handles, the SQP loop and the re-linearisation pipeline stay refused
    {
        CK(almpc_create(&h, n, m, N, batch, 0, ALMPC_FLAG_STRUCTURED));
        CK(almpc_set_keep_stage_models(h, 1));
        CK(almpc_design_shared(h, p.A.data(), p.B.data(), p.Q.data(), p.R.data(), p.S.data(), nullptr, p.umin.data(), p.umax.data(), nullptr, nullptr, 0.1, 1e-6));
        std::vector<double> x0((size_t)batch * n, 0.25);
        CK(almpc_update_initialization(h, x0.data()));
        CK(almpc_calculate(h, nullptr));
        NAMES(almpc_sensitivity_ltv(h, ALMPC_SENS_K0, 0.0), ALMPC_ERR_UNSUPPORTED, "almpc_sensitivity_stagewise_rate");
        CK(almpc_sensitivity_stagewise_rate(h, 7, 0.0));
        almpc_destroy(h); h = nullptr;
    }
    const int Hn = 8, L = 2;
    std::vector<double> W_in((size_t)Hn * (n + m), 0.05), W_h((size_t)L * Hn * Hn, 0.02), b_h((size_t)L * Hn, 0.01), W_out((size_t)n * Hn, 0.1);
    std::vector<double> xr((size_t)n * (N + 1), 0.0), ur((size_t)m * N, 0.0), x0((size_t)batch * n, 0.1), si(1), di(1);
    {
        CK(almpc_create(&h, n, m, N, batch, 0, 0));
        CK(almpc_set_keep_stage_models(h, 1));
        CK(almpc_sqp_fnn_setup(h, Hn, L, 2, W_in.data(), W_h.data(), b_h.data(), W_out.data(), xr.data(), ur.data(), p.Q.data(), p.R.data(), nullptr,
                               p.P.data(), 0, p.umin.data(), p.umax.data(), 0.1, 1e-6));
        CK(almpc_sqp_fnn_start(h, x0.data(), nullptr));
        const int rc = almpc_sqp_fnn_iterate(h, 1, 1.0, nullptr, si.data(), di.data());
        if (rc != ALMPC_OK && rc != ALMPC_ERR_NUMERIC) { std::fprintf(stderr, "iterate -> %d (%s)\n", rc, almpc_last_error(h)); return 1; }
        NAMES(almpc_sensitivity_ltv(h, ALMPC_SENS_K0, 0.0), ALMPC_ERR_UNSUPPORTED, "SQP");
        REFUSED(almpc_sensitivity_ltv_vjp(h, o.g_u.data(), nullptr, 0.0, o.g_x0.data(), nullptr), ALMPC_ERR_UNSUPPORTED);
        almpc_destroy(h); h = nullptr;
    }
    {
        CK(almpc_create(&h, n, m, N, batch, 0, 0));
        CK(almpc_set_keep_stage_models(h, 1));
        CK(almpc_relin_fnn_setup(h, Hn, L, 2, W_in.data(), W_h.data(), b_h.data(), W_out.data(), xr.data(), ur.data(), p.Q.data(), p.R.data(), nullptr, p.P.data(),
                                 p.umin.data(), p.umax.data(), 0.1, 1e-6));
        CK(almpc_update_initialization(h, x0.data()));
        CK(almpc_relin_fnn_step(h, nullptr));
        REFUSED(almpc_sensitivity_ltv(h, ALMPC_SENS_K0, 0.0), ALMPC_ERR_UNSUPPORTED);
        REFUSED(almpc_sensitivity_ltv_vjp(h, o.g_u.data(), nullptr, 0.0, o.g_x0.data(), nullptr), ALMPC_ERR_UNSUPPORTED);
        almpc_destroy(h); h = nullptr;
    }
    std::printf("sens ltv host logic ok: %ld launches\n", fake_hip_launch_count());
    return 0;
}
