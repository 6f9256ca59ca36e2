// Driver of the CPU sanitizer build of the library's HOST half for time-varying designs on the stage-wise solvers
// (almpc_design_ltv_stagewise, almpc_ltv_stagewise_update, almpc_get_ltv_stagewise_prepared): csrc/almpc_api.hip compiled host-only under
// AddressSanitizer + UndefinedBehaviorSanitizer and linked against tests/sanitize/fake_hip_runtime.cpp, as sens_ltv_driver.cpp is (device
// memory = calloc'd host memory, launches = no-ops, so every buffer the calls size, copy into and read back is bounds-checked; every
// array handed in is exactly sized, in the device form too, where the "device" arrays are host vectors the fake copies read).
// Walks both entry points in both forms on both routes (input box alone: k_riccati_t; S / state box / terminal equality: k_sgains +
// k_sdual), with and without defects, references, S, a P per instance; a step, the results, the certificate and the sensitivities
// behind each; updates in either form on either design; a redesign of another kind and back; and every refusal.
// Prints "ltv stagewise host logic ok: <launches> launches".
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
// a refusal carries its reason and names something
#define NAMES(call, want, text)                                                                              \
    do {                                                                                                     \
        EXPECT(call, want);                                                                                  \
        if (!almpc_last_error(h) || !std::strstr(almpc_last_error(h), text)) { std::fprintf(stderr, "%s:%d \"%s\" does not name %s\n", __FILE__, __LINE__, almpc_last_error(h), text); return 1; } \
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

// the trajectory arrays and references for `batch` copies of a plant, exactly sized
struct Ltv {
    std::vector<double> A, B, c, xbar, ubar, xref, uref, Pb;
    Ltv(const Plant& p, int N, int batch)
        : A(tiled(p.A, batch * N)), B(tiled(p.B, batch * N)), c((size_t)batch * N * p.n, 0.01), xbar((size_t)batch * (N + 1) * p.n, 0.2),
          ubar((size_t)batch * N * p.m, 0.1), xref((size_t)(N + 1) * p.n, 0.05), uref((size_t)N * p.m, 0.02), Pb(tiled(p.P, batch)) {}
};

// variant bits: 1 no defects, 2 no S, 4 a P per instance, 8 no references
static int design(almpc_handle* h, const Plant& p, const Ltv& a, int variant, int on_device, const double* R = nullptr) {
    return almpc_design_ltv_stagewise(h, a.A.data(), a.B.data(), (variant & 1) ? nullptr : a.c.data(), a.xbar.data(), a.ubar.data(),
                                      (variant & 8) ? nullptr : a.xref.data(), (variant & 8) ? nullptr : a.uref.data(), p.Q.data(),
                                      R ? R : p.R.data(), (variant & 2) ? nullptr : p.S.data(), (variant & 4) ? a.Pb.data() : p.P.data(),
                                      (variant & 4) ? 1 : 0, p.umin.data(), p.umax.data(), on_device);
}
static int update(almpc_handle* h, const Ltv& a, int variant, int on_device) {
    return almpc_ltv_stagewise_update(h, a.A.data(), a.B.data(), (variant & 1) ? nullptr : a.c.data(), a.xbar.data(), a.ubar.data(), on_device);
}

// exactly sized outputs
struct Out {
    std::vector<double> x, ex, u, eu, ebar, qadd, eqt, cost, K0;
    std::vector<int32_t> status, iters, piters;
    Out(int n, int m, int N, int batch)
        : x((size_t)batch * (N + 1) * n), ex(x.size()), u((size_t)batch * N * m), eu(u.size()), ebar((size_t)batch * N * n), qadd(u.size()), eqt(n),
          cost(batch), K0((size_t)batch * n * m), status(batch), iters(batch), piters(batch) {}
};

// a step on the current data, every result, the prepared vectors; rows: the design has state rows; eq: the terminal equality
static int step_and_read(almpc_handle* h, Out& o, bool rows, bool eq) {
    almpc_opts opts;
    almpc_default_opts(&opts);
    opts.warm_start = 1;   // (ignored by this design)
    CK(almpc_calculate(h, &opts));
    CK(almpc_calculate_async(h, nullptr));
    CK(almpc_synchronize(h));
    CK(almpc_get_results(h, o.x.data(), o.ex.data(), o.u.data(), o.eu.data(), o.status.data(), o.iters.data(), o.piters.data()));
    CK(almpc_get_ltv_stagewise_prepared(h, o.ebar.data(), o.qadd.data(), eq ? o.eqt.data() : nullptr));
    CK(almpc_get_ltv_stagewise_prepared(h, nullptr, nullptr, nullptr));
    if (!eq) EXPECT(almpc_get_ltv_stagewise_prepared(h, nullptr, nullptr, o.eqt.data()), ALMPC_ERR_INVALID);
    // the certificate and the sensitivities serve the design without almpc_set_keep_stage_models
    CK(almpc_certificate_ltv(h, ALMPC_CERT_COST | ALMPC_CERT_STATES));
    CK(almpc_get_certificate_ltv(h, o.cost.data(), nullptr, nullptr, nullptr, o.x.data(), o.ex.data()));
    if (rows) {
        NAMES(almpc_certificate_ltv(h, ALMPC_CERT_RES), ALMPC_ERR_UNSUPPORTED, "state rows");
        NAMES(almpc_sensitivity_ltv(h, ALMPC_SENS_K0, 0.0), ALMPC_ERR_UNSUPPORTED, "state rows");
    } else {
        CK(almpc_certificate_ltv(h, ALMPC_CERT_COST | ALMPC_CERT_RES | ALMPC_CERT_GRAD | ALMPC_CERT_COSTATE | ALMPC_CERT_STATES));
        CK(almpc_sensitivity_ltv(h, ALMPC_SENS_K0, 0.0));
        CK(almpc_get_sensitivity(h, o.K0.data(), nullptr, nullptr, o.status.data()));
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
    EXPECT(almpc_design_ltv_stagewise(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                                      nullptr, nullptr, 0), ALMPC_ERR_INVALID);
    EXPECT(almpc_ltv_stagewise_update(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0), ALMPC_ERR_INVALID);
    EXPECT(almpc_get_ltv_stagewise_prepared(nullptr, nullptr, nullptr, nullptr), ALMPC_ERR_INVALID);
    const int n = 5, m = 2, N = 9, batch = 7;
    const Plant p = chain(n, m);
    const Ltv a(p, N, batch);
    Ltv a2(p, N, batch);
    for (double& v : a2.xbar) v = -0.1;
    Out o(n, m, N, batch);
    std::vector<double> R0 = p.R;
    R0[0] = 0.0;   // the branch rule drops R and S: the Riccati route whatever S is
    // ---- every variant, both forms, four kinds of rows: none, state box, terminal equality, both
    for (int variant = 0; variant < 16; ++variant)
        for (int on_device = 0; on_device < 2; ++on_device)
            for (int rows = 0; rows < 4; ++rows) {
                CK(almpc_create(&h, n, m, N, batch, 0, ALMPC_FLAG_STRUCTURED));
                NAMES(update(h, a, variant, on_device), ALMPC_ERR_NOT_DESIGNED, "almpc_design_ltv_stagewise");
                NAMES(almpc_get_ltv_stagewise_prepared(h, o.ebar.data(), nullptr, nullptr), ALMPC_ERR_NOT_DESIGNED, "almpc_design_ltv_stagewise");
                CK(almpc_set_state_box(h, (rows & 1) ? p.xmin.data() : nullptr, (rows & 1) ? p.xmax.data() : nullptr));
                CK(almpc_set_terminal_equality(h, (rows & 2) ? 1 : 0));
                CK(design(h, p, a, variant, on_device));
                if (step_and_read(h, o, rows != 0, (rows & 2) != 0)) return 1;
                // the per-iteration call in either form, whatever form the design took; the c_all rule
                CK(update(h, a2, variant, 1 - on_device));
                if (step_and_read(h, o, rows != 0, (rows & 2) != 0)) return 1;
                CK(update(h, a, variant, on_device));
                NAMES(update(h, a, variant ^ 1, on_device), ALMPC_ERR_INVALID, "c_all");
                NAMES(almpc_ltv_stagewise_update(h, nullptr, a.B.data(), nullptr, a.xbar.data(), a.ubar.data(), on_device), ALMPC_ERR_INVALID, "null");
                NAMES(almpc_set_reference(h, a.xref.data(), a.uref.data(), 0), ALMPC_ERR_INVALID, "LTV");
                if (step_and_read(h, o, rows != 0, (rows & 2) != 0)) return 1;   // (the refused calls left the design alone)
                almpc_destroy(h);
                h = nullptr;
            }
    // ---- R[1,1] == 0; a redesign of another kind and back; almpc_design_ltv keeps refusing a structured handle with its old text
    CK(almpc_create(&h, n, m, N, batch, 0, ALMPC_FLAG_STRUCTURED));
    CK(design(h, p, a, 0, 0, R0.data()));
    if (step_and_read(h, o, false, false)) return 1;
    CK(almpc_design_batched(h, tiled(p.A, batch).data(), tiled(p.B, batch).data(), p.Q.data(), p.R.data(), nullptr, p.P.data(), 0, p.umin.data(),
                            p.umax.data(), 0.1, 1e-6));
    NAMES(update(h, a, 0, 0), ALMPC_ERR_NOT_DESIGNED, "almpc_design_ltv_stagewise");
    CK(almpc_calculate(h, nullptr));
    CK(design(h, p, a, 2, 1));
    if (step_and_read(h, o, false, false)) return 1;
    EXPECT(almpc_design_ltv(h, a.A.data(), a.B.data(), a.c.data(), a.xbar.data(), a.ubar.data(), a.xref.data(), a.uref.data(), p.Q.data(), p.R.data(),
                            p.S.data(), p.P.data(), 0, p.umin.data(), p.umax.data(), 0.1, 1e-6), ALMPC_ERR_UNSUPPORTED);
    if (std::strcmp(almpc_last_error(h), "structured solve: time-varying designs go through almpc_sqp_fnn_* (stage models on the device)")) return 1;
    // null arguments, umin > umax, continuous-time models
    NAMES(almpc_design_ltv_stagewise(h, a.A.data(), a.B.data(), nullptr, a.xbar.data(), a.ubar.data(), nullptr, nullptr, p.Q.data(), p.R.data(), nullptr,
                                     nullptr, 0, p.umin.data(), p.umax.data(), 0), ALMPC_ERR_INVALID, "P must be given");
    NAMES(almpc_design_ltv_stagewise(h, a.A.data(), a.B.data(), nullptr, a.xbar.data(), a.ubar.data(), nullptr, nullptr, p.Q.data(), p.R.data(), nullptr,
                                     p.P.data(), 0, p.umax.data(), p.umin.data(), 0), ALMPC_ERR_INVALID, "umin > umax");
    CK(almpc_set_model_time(h, ALMPC_MODEL_CONTINUOUS_ZOH, 0.1));
    NAMES(design(h, p, a, 0, 0), ALMPC_ERR_UNSUPPORTED, "continuous-time");
    CK(almpc_set_model_time(h, ALMPC_MODEL_DISCRETE, 0.0));
    almpc_destroy(h);
    h = nullptr;
    // ---- a condensed handle: almpc_design_ltv is its call
    CK(almpc_create(&h, n, m, N, batch, 0, 0));
    NAMES(design(h, p, a, 0, 0), ALMPC_ERR_UNSUPPORTED, "almpc_design_ltv");
    NAMES(update(h, a, 0, 0), ALMPC_ERR_NOT_DESIGNED, "almpc_design_ltv_stagewise");
    almpc_destroy(h);
    h = nullptr;
    // ---- (20, 9, 6): an input box alone is served (k_riccati_t); a state box, the terminal equality or S would need the table-less G = 1
    // builds of k_sdual and are refused before anything is launched or allocated
    {
        const int n2 = 20, m2 = 9, N2 = 6, b2 = 3;
        const Plant q = chain(n2, m2);
        const Ltv w(q, N2, b2);
        Out o2(n2, m2, N2, b2);
        CK(almpc_create(&h, n2, m2, N2, b2, 0, ALMPC_FLAG_STRUCTURED));
        const long before = fake_hip_launch_count();
        NAMES(design(h, q, w, 0, 0), ALMPC_ERR_UNSUPPORTED, "G = 1");                       // S: nt = 29
        CK(almpc_set_state_box(h, q.xmin.data(), q.xmax.data()));
        NAMES(design(h, q, w, 2, 1), ALMPC_ERR_UNSUPPORTED, "(32, 16)");                    // state box
        CK(almpc_set_state_box(h, nullptr, nullptr));
        CK(almpc_set_terminal_equality(h, 1));
        NAMES(design(h, q, w, 2, 0), ALMPC_ERR_UNSUPPORTED, "(48, 16)");                    // terminal equality
        CK(almpc_set_terminal_equality(h, 0));
        if (fake_hip_launch_count() != before) { std::fprintf(stderr, "a refused design launched something\n"); return 1; }
        NAMES(almpc_calculate(h, nullptr), ALMPC_ERR_NOT_DESIGNED, "design");
        CK(design(h, q, w, 2, 1));
        CK(almpc_calculate(h, nullptr));
        CK(almpc_get_results(h, o2.x.data(), o2.ex.data(), o2.u.data(), o2.eu.data(), o2.status.data(), nullptr, nullptr));
        NAMES(almpc_certificate_ltv(h, ALMPC_CERT_COST), ALMPC_ERR_UNSUPPORTED, "n <= 16");  // (the certificate's own shape limit)
        almpc_destroy(h);
        h = nullptr;
    }
    std::printf("ltv stagewise host logic ok: %ld launches\n", fake_hip_launch_count());
    return 0;
}
