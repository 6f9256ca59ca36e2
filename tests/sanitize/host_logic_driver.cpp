// Driver of the CPU sanitizer build of the library's HOST half (round-4 review, item 9): csrc/almpc_api.hip compiled host-only under
// AddressSanitizer + UndefinedBehaviorSanitizer and linked against tests/sanitize/fake_hip_runtime.cpp (device memory = calloc'd host
// memory, launches = no-ops).  What runs is exactly the code a GPU lease cannot instrument: argument checks, buffer sizing, staging
// copies, launch-parameter set-up and every host-side readback of the C ABI, for a shared, a state-row, a per-instance, a structured,
// a re-linearised and an SQP handle, single and as a group, synchronous and through tickets.  The "results" are zeros (no kernel
// ran): the point is that no call touches memory it does not own.  Prints "host logic ok: <launches> launches".
// With a path argument the fake runtime writes every launch there (stream ordinal, kernel, grid, block, LDS: the launch trace that
// tests/golden/host_launch_trace.txt pins); the handles below reach every kernel of the step path at least once.
// A second argument NAME=VALUE is one ALMPC_* switch (csrc/almpc_switches.h) the whole run is made under: its launch trace against the
// plain one is what tests/golden/host_launch_trace_switches.txt pins per switch.
// With a path argument the byte sizes of all device and pinned allocations of the run go to <path>.allocs at the end, sorted
// (tests/golden/host_alloc_sizes.txt).  With "alloc-failures" as the second argument nothing of the above runs: every entry point that
// allocates is called with its k-th allocation failing, k = 1, 2, ... until it gets through (alloc_failures below).
// With "setups" as the second argument the design and setup entry points are walked on the routes the plain run does not reach
// (setups below): every call's return line and, sorted, what it uploaded and set on the device go to stdout; with the launch trace and
// the allocation sizes they are what tests/golden/host_setups.txt pins.
// With "loops" as the second argument (and, if given, one switch NAME=VALUE as the third) the SQP loop and the re-linearised step are
// walked (loops below) with the fake runtime's ordered call trace on: return lines, trace and allocation sizes are what
// tests/golden/host_loops.txt pins.
#include "../../include/almpc.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

extern "C" long fake_hip_launch_count();
extern "C" int fake_hip_trace_to(const char* path);
extern "C" void fake_hip_trace_close();
extern "C" int fake_hip_fail_alloc_at(int k);
extern "C" int fake_hip_dump_allocs(const char* path);
extern "C" void fake_hip_record_uploads(int on);
extern "C" void fake_hip_trace_calls(int on);
extern "C" void fake_hip_print_uploads(FILE* f);
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

struct Plant {
    int n, m;
    std::vector<double> A, B, Q, R, S, umin, umax, xmin, xmax;
};

static Plant chain(int n, int m) {   // stable chain of integrators-with-leak, column-major
    Plant p;
    p.n = n; p.m = m;
    p.A.assign((size_t)n * n, 0.0); p.B.assign((size_t)n * m, 0.0); p.Q.assign((size_t)n * n, 0.0); p.R.assign((size_t)m * m, 0.0);
    p.S.assign((size_t)m * m, 0.0);
    for (int i = 0; i < n; ++i) {
        p.A[(size_t)i * n + i] = 0.9;
        if (i + 1 < n) p.A[(size_t)(i + 1) * n + i] = 0.1;
        p.Q[(size_t)i * n + i] = 100.0;
    }
    for (int a = 0; a < m; ++a) { p.B[(size_t)a * n + (n - 1 - a)] = 0.5; p.R[(size_t)a * m + a] = 0.1; p.S[(size_t)a * m + a] = 2.0; }
    p.umin.assign(m, -1.0); p.umax.assign(m, 1.0); p.xmin.assign(n, -3.0); p.xmax.assign(n, 3.0);
    return p;
}

static int step_and_read(almpc_handle* h, int n, int m, int N, int batch, bool tickets) {
    std::vector<double> x0((size_t)batch * n, 0.25), x((size_t)batch * n * (N + 1)), ex(x.size()), u((size_t)batch * m * N), eu(u.size()), u0((size_t)batch * m);
    std::vector<int32_t> st(batch), it(batch), pit(batch);
    almpc_opts o;
    almpc_default_opts(&o);
    CK(almpc_update_initialization(h, x0.data()));
    CK(almpc_calculate(h, &o));
    CK(almpc_get_results(h, x.data(), ex.data(), u.data(), eu.data(), st.data(), it.data(), pit.data()));
    CK(almpc_get_first_input(h, u0.data()));
    if (tickets) {
        double* slot = nullptr;
        CK(almpc_x0_staging(h, &slot));
        for (size_t i = 0; i < x0.size(); ++i) slot[i] = x0[i];
        CK(almpc_update_initialization_async(h, slot));
        CK(almpc_calculate_async(h, &o));
        const int t0 = almpc_get_results_async(h, ALMPC_WANT_FIRST_INPUT | ALMPC_WANT_STATUS);
        if (t0 < 0) return 1;
        CK(almpc_update_initialization_async(h, x0.data()));
        CK(almpc_calculate_async(h, &o));
        const int t1 = almpc_get_results_async(h, ALMPC_WANT_ALL);
        if (t1 < 0) return 1;
        CK(almpc_get_results_wait(h, t0, nullptr, nullptr, nullptr, nullptr, u0.data(), st.data(), nullptr, nullptr));
        CK(almpc_get_results_wait(h, t1, x.data(), ex.data(), u.data(), eu.data(), u0.data(), st.data(), it.data(), pit.data()));
        CK(almpc_synchronize(h));
    }
    return 0;
}

// `call` on a fresh handle (made by `prep` without failures) with the k-th allocation inside it failing, for k = 1, 2, ... until no
// allocation is left to fail.  Every call whose allocation failed must return ALMPC_ERR_HIP, and no call fails otherwise.  The
// redo of undecided instances (almpc_set_structured_fallback) is asked for (`fallback` 1: a stage-wise setup that fails is the
// call's error; at the default, 2, the design goes on without it) or off (0: its buffers are not made).  Every handle is destroyed:
// what a failed call leaves behind must be freed exactly once (ASan, LSan).
template <typename Prep, typename Call>
static int walk(const char* name, int n, int m, int N, int batch, uint32_t flags, int fallback, Prep prep, Call call) {
    for (int k = 1; k <= 200; ++k) {
        almpc_handle* h = nullptr;
        CK(almpc_create(&h, n, m, N, batch, 0, flags));
        CK(almpc_set_structured_fallback(h, fallback));
        CK(prep(h));
        fake_hip_fail_alloc_at(k);
        const int rc = call(h);
        const bool fired = fake_hip_fail_alloc_at(0) == 0;
        const std::string msg = almpc_last_error(h);
        almpc_destroy(h);
        if (rc != (fired ? ALMPC_ERR_HIP : ALMPC_OK)) {
            std::fprintf(stderr, "%s (fallback %d), allocation %d %s: -> %d (%s)\n", name, fallback, k, fired ? "failing" : "not reached", rc, msg.c_str());
            return 1;
        }
        if (!fired) { std::printf("%s (fallback %d): %d allocations\n", name, fallback, k - 1); return 0; }
    }
    std::fprintf(stderr, "%s: still allocating after 200 failures\n", name);
    return 1;
}

static int alloc_failures() {
    const int n = 4, m = 2, N = 12, batch = 7, Hn = 8, L = 2;
    const Plant p = chain(n, m);
    const auto nothing = [](almpc_handle*) { return (int)ALMPC_OK; };
    for (int k = 1;; ++k) {   // almpc_create, condensed and structured
        almpc_handle *h = nullptr, *hs = nullptr;
        fake_hip_fail_alloc_at(k);
        const int rc = almpc_create(&h, n, m, N, batch, 0, 0);
        const bool fired = fake_hip_fail_alloc_at(0) == 0;
        fake_hip_fail_alloc_at(k);
        const int rcs = almpc_create(&hs, n, m, N, batch, 0, ALMPC_FLAG_STRUCTURED);
        const bool fireds = fake_hip_fail_alloc_at(0) == 0;
        if ((rc == ALMPC_OK) != (h != nullptr) || (rcs == ALMPC_OK) != (hs != nullptr) || (rc == ALMPC_OK) == fired || (rcs == ALMPC_OK) == fireds || k > 200) {
            std::fprintf(stderr, "almpc_create, allocation %d failing: -> %d, %d\n", k, rc, rcs);
            return 1;
        }
        almpc_destroy(h); almpc_destroy(hs);
        if (!fired && !fireds) { std::printf("almpc_create: %d allocations\n", k - 1); break; }
    }
    std::vector<double> xr((size_t)n * (N + 1), 0.1), ur((size_t)m * N, 0.05), x0((size_t)batch * n, 0.25), P((size_t)n * n, 0.0);
    for (int k = 0; k < N; ++k) ur[(size_t)k * m] = 0.01 * k;
    for (int i = 0; i < n; ++i) P[(size_t)i * n + i] = 150.0;
    std::vector<double> Ab((size_t)batch * n * n), Bb((size_t)batch * n * m);
    for (int i = 0; i < batch; ++i) {
        for (size_t t = 0; t < p.A.size(); ++t) Ab[(size_t)i * n * n + t] = p.A[t];
        for (size_t t = 0; t < p.B.size(); ++t) Bb[(size_t)i * n * m + t] = p.B[t] * (1.0 + 0.01 * i);
    }
    for (const int fb : {1, 0}) {   // the redo of undecided instances asked for, then off
    const auto box_and_eq = [&](almpc_handle* h) { return almpc_set_terminal_equality(h, 1); };
    if (walk("almpc_design_shared", n, m, N, batch, 0, fb, box_and_eq, [&](almpc_handle* h) {   // state box + terminal equality: the projection's temporary
            return almpc_design_shared(h, p.A.data(), p.B.data(), p.Q.data(), p.R.data(), p.S.data(), nullptr, p.umin.data(), p.umax.data(), p.xmin.data(), p.xmax.data(), 0.1, 1e-6);
        })) return 1;
    if (walk("almpc_design_shared (structured)", n, m, N, batch, ALMPC_FLAG_STRUCTURED, fb, box_and_eq, [&](almpc_handle* h) {
            return almpc_design_shared(h, p.A.data(), p.B.data(), p.Q.data(), p.R.data(), p.S.data(), nullptr, p.umin.data(), p.umax.data(), p.xmin.data(), p.xmax.data(), 0.1, 1e-6);
        })) return 1;
    const auto design_batched = [&](almpc_handle* h) {
        return almpc_design_batched(h, Ab.data(), Bb.data(), p.Q.data(), p.R.data(), p.S.data(), nullptr, 0, p.umin.data(), p.umax.data(), 0.1, 1e-6);
    };
    const auto state_box = [&](almpc_handle* h) { return almpc_set_state_box(h, p.xmin.data(), p.xmax.data()); };
    if (walk("almpc_design_batched", n, m, N, batch, 0, fb, state_box, design_batched)) return 1;
    if (walk("almpc_design_batched (structured)", n, m, N, batch, ALMPC_FLAG_STRUCTURED, fb, state_box, design_batched)) return 1;
    {
        std::vector<double> Aall((size_t)batch * N * n * n), Ball((size_t)batch * N * n * m), call((size_t)batch * N * n, 0.01),
            xbar((size_t)batch * (N + 1) * n, 0.2), ubar((size_t)batch * N * m, 0.1);
        for (size_t i = 0; i < (size_t)batch * N; ++i) {
            for (size_t t = 0; t < p.A.size(); ++t) Aall[i * n * n + t] = p.A[t];
            for (size_t t = 0; t < p.B.size(); ++t) Ball[i * n * m + t] = p.B[t];
        }
        if (walk("almpc_design_ltv", n, m, N, batch, 0, fb, state_box, [&](almpc_handle* h) {   // state rows: the staging buffers are handed to the handle
                return almpc_design_ltv(h, Aall.data(), Ball.data(), call.data(), xbar.data(), ubar.data(), xr.data(), ur.data(), p.Q.data(), p.R.data(),
                                        p.S.data(), P.data(), 0, p.umin.data(), p.umax.data(), 0.1, 1e-6);
            })) return 1;
    }
    if (walk("almpc_set_reference", n, m, N, batch, 0, fb, design_batched, [&](almpc_handle* h) {   // per-instance models with S: the gradient's temporary
            return almpc_set_reference(h, xr.data(), ur.data(), 0);
        })) return 1;
    std::vector<double> W_in((size_t)Hn * (n + m), 0.05), W_h((size_t)L * Hn * Hn, 0.02), b_h((size_t)L * Hn, 0.01), W_out((size_t)n * Hn, 0.1);
    const auto relin = [&](almpc_handle* h) {
        return almpc_relin_fnn_setup(h, Hn, L, 0, W_in.data(), W_h.data(), b_h.data(), W_out.data(), xr.data(), ur.data(), p.Q.data(), p.R.data(), p.S.data(),
                                     P.data(), p.umin.data(), p.umax.data(), 0.1, 1e-6);
    };
    if (walk("almpc_relin_fnn_setup", n, m, N, batch, 0, fb, state_box, relin)) return 1;
    if (walk("almpc_relin_fnn_setup (structured)", n, m, N, batch, ALMPC_FLAG_STRUCTURED, fb, nothing, relin)) return 1;
    if (walk("almpc_sqp_fnn_setup", n, m, N, batch, 0, fb, relin, [&](almpc_handle* h) {   // on a handle that held the re-linearisation pipeline
            const int rc = almpc_set_state_box(h, p.xmin.data(), p.xmax.data());
            return rc != ALMPC_OK ? rc : almpc_sqp_fnn_setup(h, Hn, L, 1, W_in.data(), W_h.data(), b_h.data(), W_out.data(), xr.data(), ur.data(), p.Q.data(),
                                                             p.R.data(), nullptr, P.data(), 0, p.umin.data(), p.umax.data(), 0.1, 1e-6);
        })) return 1;
    if (walk("almpc_update_initialization_async", n, m, N, batch, 0, fb, nothing, [&](almpc_handle* h) { return almpc_update_initialization_async(h, x0.data()); }))
        return 1;
    }
    std::printf("alloc failures ok\n");
    return 0;
}

// One line per call, `what -> code (almpc_last_error)`, and behind a setup call what it copied to and set on the device, sorted (a step's
// own copies are dropped).  Whatever a path returns is its pin: nothing here stops at an error code.
static int show(almpc_handle* h, const char* what, int rc, bool uploads = true) {
    std::printf("%s -> %d (%s)\n", what, rc, rc != ALMPC_OK && h ? almpc_last_error(h) : "");
    fake_hip_print_uploads(uploads ? stdout : nullptr);
    return rc;
}

static int setups() {
    const int n = 4, m = 2, N = 12, batch = 13, Hn = 8, L = 2;
    const Plant p = chain(n, m);
    fake_hip_record_uploads(1);
    std::vector<double> xr((size_t)n * (N + 1), 0.1), ur((size_t)m * N, 0.05), x0((size_t)batch * n, 0.25);
    for (int k = 0; k < N; ++k) ur[(size_t)k * m] = 0.01 * k;
    std::vector<double> Ab((size_t)batch * n * n), Bb((size_t)batch * n * m), P((size_t)n * n, 0.0), Pb((size_t)batch * n * n, 0.0);
    for (int i = 0; i < batch; ++i) {
        for (size_t t = 0; t < p.A.size(); ++t) Ab[(size_t)i * n * n + t] = p.A[t];
        for (size_t t = 0; t < p.B.size(); ++t) Bb[(size_t)i * n * m + t] = p.B[t] * (1.0 + 0.01 * i);
        for (int j = 0; j < n; ++j) Pb[(size_t)i * n * n + (size_t)j * n + j] = 150.0 + i;
        Pb[(size_t)i * n * n + 1] = 3.0;   // (not symmetric: what a path does with that is part of its pin)
    }
    for (int j = 0; j < n; ++j) P[(size_t)j * n + j] = 150.0;
    P[1] = 3.0;
    Plant ps = p;   // weights that are not symmetric
    ps.Q[1] = 2.0; ps.R[1] = 0.02; ps.S[1] = 0.5;
    Plant pd = p;   // ... for the designs that take their terminal weight from a DARE, which wants Q and R symmetric: S only
    pd.S[1] = 0.5;
    std::vector<double> W_in((size_t)Hn * (n + m), 0.05), W_h((size_t)L * Hn * Hn, 0.02), b_h((size_t)L * Hn, 0.01), W_out((size_t)n * Hn, 0.1);
    std::vector<double> Wd_h((size_t)Hn * Hn * L * (L + 1) / 2, 0.02), Wd_out((size_t)n * Hn * (L + 1), 0.1);   // DenseNet: growing blocks
    for (size_t t = 0; t < W_in.size(); ++t) W_in[t] += 0.001 * t;
    std::vector<double> Aall((size_t)batch * N * n * n), Ball((size_t)batch * N * n * m), call((size_t)batch * N * n, 0.01),
        xbar((size_t)batch * (N + 1) * n, 0.2), ubar((size_t)batch * N * m, 0.1);
    for (size_t i = 0; i < (size_t)batch * N; ++i) {
        for (size_t t = 0; t < p.A.size(); ++t) Aall[i * n * n + t] = p.A[t];
        for (size_t t = 0; t < p.B.size(); ++t) Ball[i * n * m + t] = p.B[t];
    }
    almpc_opts cold, warm;
    almpc_default_opts(&cold);
    almpc_default_opts(&warm);
    warm.warm_start = 1;
    almpc_handle* h = nullptr;
    const auto open = [&](const char* title, uint32_t flags, bool box) {
        std::printf("---- %s\n", title);
        if (almpc_create(&h, n, m, N, batch, 0, flags) != ALMPC_OK) return 1;
        return box ? show(h, "set_state_box", almpc_set_state_box(h, p.xmin.data(), p.xmax.data())) : 0;
    };
    const auto close = [&] { almpc_destroy(h); h = nullptr; };
    const auto step = [&] {
        show(h, "  update_initialization", almpc_update_initialization(h, x0.data()), false);
        show(h, "  calculate", almpc_calculate(h, &cold), false);
    };
    const auto relin_steps = [&] {
        show(h, "  update_initialization", almpc_update_initialization(h, x0.data()), false);
        show(h, "  relin_fnn_step cold", almpc_relin_fnn_step(h, &cold), false);
        show(h, "  relin_fnn_step warm", almpc_relin_fnn_step(h, &warm), false);
    };
    const auto sqp_iterate = [&] {
        show(h, "  sqp_fnn_start", almpc_sqp_fnn_start(h, x0.data(), nullptr), false);
        double si = 0.0, di = 0.0;
        show(h, "  sqp_fnn_iterate", almpc_sqp_fnn_iterate(h, 1, 1.0, nullptr, &si, &di), false);
    };
    const auto batched = [&](const Plant& w_, const double* S, const double* Pw, int per) {
        const Plant& w = &w_ == &ps && !Pw ? pd : w_;
        return almpc_design_batched(h, Ab.data(), Bb.data(), w.Q.data(), w.R.data(), S, Pw, per, w.umin.data(), w.umax.data(), 0.1, 1e-6);
    };
    const auto shared = [&](const Plant& w_, const double* S, const double* Pw, const double* xmin, const double* xmax) {
        const Plant& w = &w_ == &ps && !Pw ? pd : w_;
        return almpc_design_shared(h, w.A.data(), w.B.data(), w.Q.data(), w.R.data(), S, Pw, w.umin.data(), w.umax.data(), xmin, xmax, 0.1, 1e-6);
    };
    const auto relin = [&](const Plant& w, int act) {
        return almpc_relin_fnn_setup(h, Hn, L, act, W_in.data(), W_h.data(), b_h.data(), W_out.data(), xr.data(), ur.data(), w.Q.data(), w.R.data(), w.S.data(),
                                     P.data(), w.umin.data(), w.umax.data(), 0.1, 1e-6);
    };
    const auto sqp = [&](const Plant& w, const double* S, int act) {
        return almpc_sqp_fnn_setup(h, Hn, L, act, W_in.data(), W_h.data(), b_h.data(), W_out.data(), xr.data(), ur.data(), w.Q.data(), w.R.data(), S, Pb.data(), 1,
                                   w.umin.data(), w.umax.data(), 0.1, 1e-6);
    };
    const auto ltv = [&](const Plant& w) {
        return almpc_design_ltv(h, Aall.data(), Ball.data(), call.data(), xbar.data(), ubar.data(), xr.data(), ur.data(), w.Q.data(), w.R.data(), w.S.data(), P.data(), 0,
                                w.umin.data(), w.umax.data(), 0.1, 1e-6);
    };
    // ---- the condensed designs the plain run walks, here for what they upload
    if (open("condensed: design_shared, input box; then state box + terminal equality + S", 0, false)) return 1;
    show(h, "design_shared", shared(ps, nullptr, nullptr, nullptr, nullptr)); step();
    show(h, "set_terminal_equality", almpc_set_terminal_equality(h, 1));
    show(h, "design_shared (box, eq, S, P)", shared(ps, ps.S.data(), P.data(), p.xmin.data(), p.xmax.data())); step();
    close();
    for (const bool box : {false, true}) {
        if (open(box ? "condensed: design_batched, state box + S" : "condensed: design_batched, input box", 0, box)) return 1;
        show(h, "design_batched P null", batched(ps, box ? ps.S.data() : nullptr, nullptr, 0)); step();
        show(h, "design_batched P shared", batched(ps, box ? ps.S.data() : nullptr, P.data(), 0)); step();
        show(h, "design_batched P per instance", batched(ps, box ? ps.S.data() : nullptr, Pb.data(), 1)); step();
        close();
    }
    for (const bool box : {false, true}) {
        if (open(box ? "condensed: relin_fnn_setup, state box" : "condensed: relin_fnn_setup", 0, box)) return 1;
        show(h, "relin_fnn_setup", relin(ps, 1)); relin_steps();
        show(h, "sqp_fnn_setup behind it", sqp(ps, ps.S.data(), 1)); sqp_iterate();
        close();
    }
    // ---- structured handle, almpc_design_batched
    for (const bool box : {false, true})
        for (int pk = 0; pk < 3; ++pk) {
            if (open(box ? "structured: design_batched, state box + S" : "structured: design_batched, input box", ALMPC_FLAG_STRUCTURED, box)) return 1;
            show(h, pk == 0 ? "design_batched P null" : (pk == 1 ? "design_batched P shared" : "design_batched P per instance"),
                 batched(ps, box ? ps.S.data() : nullptr, pk == 0 ? nullptr : (pk == 1 ? P.data() : Pb.data()), pk == 2));
            step();
            close();
        }
    // ---- structured handle, almpc_design_shared (state box + S), almpc_relin_fnn_setup
    if (open("structured: design_shared, state box + S", ALMPC_FLAG_STRUCTURED, false)) return 1;
    show(h, "design_shared", shared(ps, ps.S.data(), nullptr, p.xmin.data(), p.xmax.data())); step();
    close();
    for (const bool box : {false, true}) {
        if (open(box ? "structured: relin_fnn_setup, state box" : "structured: relin_fnn_setup", ALMPC_FLAG_STRUCTURED, box)) return 1;
        show(h, "relin_fnn_setup", relin(ps, ALMPC_NET_CODE(1, 2))); relin_steps();
        close();
    }
    // ---- SQP on the structured routes, P per instance
    if (open("condensed: sqp_fnn_set_structured(1), state box", 0, true)) return 1;
    show(h, "sqp_fnn_set_structured", almpc_sqp_fnn_set_structured(h, 1));
    show(h, "sqp_fnn_setup", sqp(ps, ps.S.data(), 1)); sqp_iterate();
    close();
    if (open("structured: sqp_fnn_setup", ALMPC_FLAG_STRUCTURED, false)) return 1;
    show(h, "sqp_fnn_setup", sqp(ps, nullptr, 1)); sqp_iterate();
    close();
    // ---- almpc_design_ltv
    if (open("condensed: design_ltv, state box", 0, true)) return 1;
    show(h, "design_ltv", ltv(ps)); step();
    close();
    if (open("condensed: design_ltv, input box", 0, false)) return 1;
    show(h, "design_ltv", ltv(ps)); step();
    close();
    // ---- DenseNet
    if (open("condensed: DenseNet", 0, false)) return 1;
    show(h, "relin_densenet_setup", almpc_relin_densenet_setup(h, Hn, L, 1, W_in.data(), Wd_h.data(), b_h.data(), Wd_out.data(), xr.data(), ur.data(), ps.Q.data(),
                                                               ps.R.data(), ps.S.data(), P.data(), p.umin.data(), p.umax.data(), 0.1, 1e-6));
    relin_steps();
    show(h, "sqp_densenet_setup", almpc_sqp_densenet_setup(h, Hn, L, 1, W_in.data(), Wd_h.data(), b_h.data(), Wd_out.data(), xr.data(), ur.data(), ps.Q.data(),
                                                           ps.R.data(), nullptr, Pb.data(), 1, p.umin.data(), p.umax.data(), 0.1, 1e-6));
    sqp_iterate();
    close();
    // ---- terminal weights and discretisation on the device
    for (const uint32_t flags : {0u, (uint32_t)ALMPC_FLAG_STRUCTURED}) {
        if (open(flags ? "structured: set_terminal_weight(DARE_DEVICE)" : "condensed: set_terminal_weight(DARE_DEVICE)", flags, false)) return 1;
        show(h, "set_terminal_weight", almpc_set_terminal_weight(h, ALMPC_TERMINAL_DARE_DEVICE));
        show(h, "design_batched P null", batched(ps, nullptr, nullptr, 0)); step();
        show(h, "relin_fnn_setup", relin(ps, 1)); relin_steps();
        close();
        if (open(flags ? "structured: set_model_time(1, 0.1)" : "condensed: set_model_time(1, 0.1)", flags, false)) return 1;
        show(h, "set_model_time", almpc_set_model_time(h, ALMPC_MODEL_CONTINUOUS_ZOH, 0.1));
        show(h, "design_shared", shared(ps, nullptr, nullptr, nullptr, nullptr)); step();
        show(h, "design_batched P null", batched(ps, nullptr, nullptr, 0)); step();
        show(h, "relin_fnn_setup", relin(ps, 1)); relin_steps();
        show(h, "sqp_fnn_setup", sqp(ps, nullptr, 1));
        show(h, "design_ltv", ltv(ps));
        close();
    }
    // ---- refusals: every entry point with one thing wrong at a time
    for (const uint32_t flags : {0u, (uint32_t)ALMPC_FLAG_STRUCTURED}) {
        if (open(flags ? "structured: refusals" : "condensed: refusals", flags, false)) return 1;
        Plant bad = p;
        bad.umin[1] = 2.0;   // umin > umax
        Plant xb = p;
        xb.xmin[2] = 4.0;    // xmin > xmax
        const int Hbig = 3000;   // 2 H (1 + n + m) doubles of Jacobian scratch: beyond 160 KB
        std::vector<double> Wb_in((size_t)Hbig * (n + m), 0.01), Wb_out((size_t)n * Hbig, 0.01);
        show(h, "design_shared, Q null", almpc_design_shared(h, p.A.data(), p.B.data(), nullptr, p.R.data(), nullptr, nullptr, p.umin.data(), p.umax.data(), nullptr, nullptr, 0.1, 1e-6));
        show(h, "design_shared, umin > umax", shared(bad, nullptr, nullptr, nullptr, nullptr));
        show(h, "design_shared, xmin without xmax", shared(p, nullptr, nullptr, p.xmin.data(), nullptr));
        show(h, "design_shared, xmin > xmax", shared(p, nullptr, nullptr, xb.xmin.data(), xb.xmax.data()));
        show(h, "design_shared, rho 0", almpc_design_shared(h, p.A.data(), p.B.data(), p.Q.data(), p.R.data(), nullptr, nullptr, p.umin.data(), p.umax.data(), nullptr, nullptr, 0.0, 1e-6));
        show(h, "design_batched, A null", almpc_design_batched(h, nullptr, Bb.data(), p.Q.data(), p.R.data(), nullptr, nullptr, 0, p.umin.data(), p.umax.data(), 0.1, 1e-6));
        show(h, "design_batched, umin > umax", batched(bad, nullptr, nullptr, 0));
        show(h, "design_batched, rho 0", almpc_design_batched(h, Ab.data(), Bb.data(), p.Q.data(), p.R.data(), nullptr, nullptr, 0, p.umin.data(), p.umax.data(), 0.0, 1e-6));
        show(h, "set_state_box, xmin without xmax", almpc_set_state_box(h, p.xmin.data(), nullptr));
        show(h, "set_state_box, xmin > xmax", almpc_set_state_box(h, xb.xmin.data(), xb.xmax.data()));
        show(h, "design_ltv", ltv(p));   // (a structured handle: time-varying designs are refused)
        show(h, "design_ltv, P null", almpc_design_ltv(h, Aall.data(), Ball.data(), call.data(), xbar.data(), ubar.data(), xr.data(), ur.data(), p.Q.data(), p.R.data(), nullptr,
                                                       nullptr, 0, p.umin.data(), p.umax.data(), 0.1, 1e-6));
        show(h, "design_ltv, umin > umax", ltv(bad));
        show(h, "design_ltv, rho 0", almpc_design_ltv(h, Aall.data(), Ball.data(), call.data(), xbar.data(), ubar.data(), xr.data(), ur.data(), p.Q.data(), p.R.data(), nullptr,
                                                      P.data(), 0, p.umin.data(), p.umax.data(), 0.0, 1e-6));
        for (const bool dense : {false, true}) {
            const auto rs = [&](int Hh, int Ll, int act, const double* Wi, const double* Wo, const double* Pw, const Plant& w, double rho) {
                return (dense ? almpc_relin_densenet_setup : almpc_relin_fnn_setup)(h, Hh, Ll, act, Wi, dense ? Wd_h.data() : W_h.data(), b_h.data(), Wo, xr.data(), ur.data(),
                                                                                    w.Q.data(), w.R.data(), w.S.data(), Pw, w.umin.data(), w.umax.data(), rho, 1e-6);
            };
            const auto ss = [&](int Hh, int Ll, int act, const double* Wi, const double* Wo, const double* Pw, const Plant& w, double rho) {
                return (dense ? almpc_sqp_densenet_setup : almpc_sqp_fnn_setup)(h, Hh, Ll, act, Wi, dense ? Wd_h.data() : W_h.data(), b_h.data(), Wo, xr.data(), ur.data(),
                                                                                w.Q.data(), w.R.data(), w.S.data(), Pw, 0, w.umin.data(), w.umax.data(), rho, 1e-6);
            };
            const double* Wo = dense ? Wd_out.data() : W_out.data();
            std::printf("-- %s\n", dense ? "DenseNet" : "Fnn");
            show(h, "relin setup, P null", rs(Hn, L, 1, W_in.data(), Wo, nullptr, p, 0.1));
            show(h, "relin setup, umin > umax", rs(Hn, L, 1, W_in.data(), Wo, P.data(), bad, 0.1));
            show(h, "relin setup, rho 0", rs(Hn, L, 1, W_in.data(), Wo, P.data(), p, 0.0));
            show(h, "relin setup, activation 9", rs(Hn, L, 9, W_in.data(), Wo, P.data(), p, 0.1));
            show(h, "relin setup, network beyond 160 KB", rs(Hbig, 0, 1, Wb_in.data(), Wb_out.data(), P.data(), p, 0.1));
            show(h, "sqp setup, P null", ss(Hn, L, 1, W_in.data(), Wo, nullptr, p, 0.1));
            show(h, "sqp setup, umin > umax", ss(Hn, L, 1, W_in.data(), Wo, P.data(), bad, 0.1));
            show(h, "sqp setup, rho 0", ss(Hn, L, 1, W_in.data(), Wo, P.data(), p, 0.0));
            show(h, "sqp setup, activation 9", ss(Hn, L, 9, W_in.data(), Wo, P.data(), p, 0.1));
            show(h, "sqp setup, network beyond 160 KB", ss(Hbig, 0, 1, Wb_in.data(), Wb_out.data(), P.data(), p, 0.1));
        }
        close();
    }
    {   // shapes: what almpc_create lets through decides which refusals of the setups can be reached at all
        std::printf("---- refusals by shape\n");
        std::printf("create n = 65 -> %d\n", almpc_create(&h, 65, 1, 4, 2, 0, 0));
        std::printf("create structured n = 40 (outside both stage-wise solvers) -> %d\n", almpc_create(&h, 40, 2, 4, 2, 0, ALMPC_FLAG_STRUCTURED));
        // n + m = 50 with an input-rate weight: outside the stage-wise dual solve, n = 40 outside the primal one
        const int n2 = 40, m2 = 10, N2 = 8, b2 = 3;
        const Plant w = chain(n2, m2);
        std::vector<double> A2((size_t)b2 * n2 * n2), B2((size_t)b2 * n2 * m2);
        for (int i = 0; i < b2; ++i) {
            std::copy(w.A.begin(), w.A.end(), A2.begin() + (size_t)i * n2 * n2);
            std::copy(w.B.begin(), w.B.end(), B2.begin() + (size_t)i * n2 * m2);
        }
        if (almpc_create(&h, n2, m2, N2, b2, 0, 0) != ALMPC_OK) return 1;
        show(h, "set_structured_fallback 1", almpc_set_structured_fallback(h, 1));
        show(h, "design_shared, S + state box, fallback 1", almpc_design_shared(h, w.A.data(), w.B.data(), w.Q.data(), w.R.data(), w.S.data(), nullptr, w.umin.data(),
                                                                               w.umax.data(), w.xmin.data(), w.xmax.data(), 0.1, 1e-6));
        show(h, "design_shared, S, fallback 1", almpc_design_shared(h, w.A.data(), w.B.data(), w.Q.data(), w.R.data(), w.S.data(), nullptr, w.umin.data(), w.umax.data(),
                                                                   nullptr, nullptr, 0.1, 1e-6));
        show(h, "design_batched, S, fallback 1", almpc_design_batched(h, A2.data(), B2.data(), w.Q.data(), w.R.data(), w.S.data(), nullptr, 0, w.umin.data(), w.umax.data(), 0.1, 1e-6));
        close();
        if (almpc_create(&h, n2, m2, N2, b2, 0, 0) != ALMPC_OK) return 1;   // (the default: the redo wherever the solvers cover the design)
        show(h, "design_shared, S + state box", almpc_design_shared(h, w.A.data(), w.B.data(), w.Q.data(), w.R.data(), w.S.data(), nullptr, w.umin.data(), w.umax.data(),
                                                                   w.xmin.data(), w.xmax.data(), 0.1, 1e-6));
        close();
    }
    fake_hip_record_uploads(0);
    std::printf("setups ok\n");
    return 0;
}

// The SQP loop (start, iterate, solve on every QP route, both Hessian modes, row multipliers, every refusal) and the re-linearised
// step (cold, warm, timing, advance; terminal weights and discretisation on the device) with the ordered call trace on.
static int loops() {
    const int n = 4, m = 2, N = 12, batch = 5, Hn = 8, L = 2, TANH = 2;
    const Plant p = chain(n, m);
    fake_hip_record_uploads(1);
    fake_hip_trace_calls(1);
    std::vector<double> xr((size_t)n * (N + 1), 0.1), ur((size_t)m * N, 0.05), x0((size_t)batch * n, 0.25), P((size_t)n * n, 0.0);
    for (int k = 0; k < N; ++k) ur[(size_t)k * m] = 0.01 * k;
    for (int j = 0; j < n; ++j) P[(size_t)j * n + j] = 150.0;
    std::vector<double> W_in((size_t)Hn * (n + m), 0.05), W_h((size_t)L * Hn * Hn, 0.02), b_h((size_t)L * Hn, 0.01), W_out((size_t)n * Hn, 0.1);
    std::vector<double> Wd_h((size_t)Hn * Hn * L * (L + 1) / 2, 0.02), Wd_out((size_t)n * Hn * (L + 1), 0.1);   // DenseNet: growing blocks
    for (size_t t = 0; t < W_in.size(); ++t) W_in[t] += 0.001 * t;
    std::vector<double> ug((size_t)batch * m * N);   // a start that leaves the input box on both sides
    for (size_t t = 0; t < ug.size(); ++t) ug[t] = 0.4 * (double)(t % 9) - 1.6;
    std::vector<double> si(8), di(8), kkt(batch), mu((size_t)batch * N * n);
    std::vector<int32_t> st(batch), its(batch), sk(batch);
    almpc_opts cold, warm;
    almpc_default_opts(&cold);
    almpc_default_opts(&warm);
    warm.warm_start = 1;
    almpc_handle* h = nullptr;
    const auto open = [&](const char* title, uint32_t flags, bool box, int horizon = 0) {
        std::printf("---- %s\n", title);
        if (almpc_create(&h, n, m, horizon ? horizon : N, batch, 0, flags) != ALMPC_OK) return 1;
        return box ? show(h, "set_state_box", almpc_set_state_box(h, p.xmin.data(), p.xmax.data())) : 0;
    };
    const auto close = [&] { almpc_destroy(h); h = nullptr; };
    const auto sqp = [&](const Plant& w, const double* S, int act, bool dense = false) {
        return show(h, dense ? "sqp_densenet_setup" : "sqp_fnn_setup",
                    (dense ? almpc_sqp_densenet_setup : almpc_sqp_fnn_setup)(h, Hn, L, act, W_in.data(), dense ? Wd_h.data() : W_h.data(), b_h.data(),
                                                                             dense ? Wd_out.data() : W_out.data(), xr.data(), ur.data(), w.Q.data(), w.R.data(), S,
                                                                             P.data(), 0, w.umin.data(), w.umax.data(), 0.1, 1e-6));
    };
    const auto start = [&](const double* guess) { return show(h, guess ? "  sqp_fnn_start (guess outside the box)" : "  sqp_fnn_start", almpc_sqp_fnn_start(h, x0.data(), guess)); };
    const auto iterate = [&](int k, double scale = 1.0) {
        std::printf("  iterate %d %g:", k, scale);
        return show(h, "", almpc_sqp_fnn_iterate(h, k, scale, nullptr, si.data(), di.data()));
    };
    const auto solve = [&](int k, double tol = 1e-6) {
        std::printf("  solve %d %g:", k, tol);
        return show(h, "", almpc_sqp_fnn_solve(h, k, tol, nullptr, st.data(), its.data(), kkt.data()));
    };
    const auto hessian = [&](int mode) { return show(h, mode ? "  set_hessian exact" : "  set_hessian gauss-newton", almpc_sqp_fnn_set_hessian(h, mode)); };
    const auto rows_on = [&] { return show(h, "  set_row_multipliers 1", almpc_sqp_fnn_set_row_multipliers(h, 1)); };
    // ---- 1. condensed, input box only
    if (open("sqp 1: condensed, input box", 0, false)) return 1;
    sqp(p, nullptr, TANH); start(nullptr);
    iterate(3); iterate(2, 0.5);
    show(h, "  set_step_rule 1", almpc_sqp_fnn_set_step_rule(h, 1));
    solve(4);
    hessian(1); start(ug.data());
    iterate(2); solve(3);
    close();
    // ---- 2. condensed, state box, the default fallback
    if (open("sqp 2: condensed, state box", 0, true)) return 1;
    sqp(p, nullptr, TANH); start(nullptr);
    iterate(2); rows_on(); iterate(2); solve(3);
    hessian(1); solve(3);
    show(h, "  state_multipliers", almpc_sqp_fnn_state_multipliers(h, mu.data()));
    show(h, "  skipped", almpc_sqp_fnn_skipped(h, sk.data()));
    close();
    // ---- 3. condensed, input box with S: the flagged redo is k_sgains + k_sdual
    if (open("sqp 3: condensed, input box, S", 0, false)) return 1;
    sqp(p, p.S.data(), TANH); start(nullptr);
    iterate(2);
    close();
    // ---- 4. no redo
    if (open("sqp 4: condensed, input box, fallback off", 0, false)) return 1;
    show(h, "set_structured_fallback 0", almpc_set_structured_fallback(h, 0));
    sqp(p, nullptr, TANH); start(nullptr);
    iterate(2); solve(2);
    close();
    // ---- 5. every QP stage-wise on a condensed handle, state box
    if (open("sqp 5: sqp_fnn_set_structured(1), state box", 0, true)) return 1;
    show(h, "sqp_fnn_set_structured", almpc_sqp_fnn_set_structured(h, 1));
    sqp(p, nullptr, TANH); start(nullptr);
    iterate(2); solve(3);
    rows_on(); iterate(1);
    close();
    // ---- 6. structured handle, input box: k_riccati
    if (open("sqp 6: structured, input box", ALMPC_FLAG_STRUCTURED, false)) return 1;
    sqp(p, nullptr, TANH); start(nullptr);
    iterate(2); solve(3);
    close();
    // ---- 7. DenseNet
    if (open("sqp 7: DenseNet", 0, false)) return 1;
    sqp(p, nullptr, TANH, true); start(nullptr);
    iterate(2); hessian(1); solve(2);
    close();
    // ---- 8. nz = 140 on a condensed handle: almpc_create lets m N <= 128 through, so nz > 128 never reaches this loop.  Its branches
    // without the scaling in the design kernel's tail (k_sqp_prepare, flag memset, k_fs_scale, k_neg_gm by launches of their own) are
    // walked by the exact-Hessian cases above and by the whole mode under ALMPC_DBG_SPLIT_SCALE=1 and ALMPC_LTV_LDS=1
    std::printf("---- sqp 8: condensed, nz 140\ncreate n 4, m 2, N 70 -> %d\n", almpc_create(&h, n, m, 70, batch, 0, 0));
    // ... and the plain run's nz = 80 (N = 40): from the second iteration on the guess builds the inverse of its working set
    // (k_guess_iterate_ws), with an input box and with state rows
    for (const bool box : {false, true}) {
        const int N80 = 40;
        std::vector<double> xr80((size_t)n * (N80 + 1), 0.1), ur80((size_t)m * N80, 0.05);
        if (open(box ? "sqp 8: condensed, state box, nz 80" : "sqp 8: condensed, input box, nz 80", 0, box, N80)) return 1;
        show(h, "sqp_fnn_setup", almpc_sqp_fnn_setup(h, Hn, L, TANH, W_in.data(), W_h.data(), b_h.data(), W_out.data(), xr80.data(), ur80.data(), p.Q.data(), p.R.data(),
                                                     nullptr, P.data(), 0, p.umin.data(), p.umax.data(), 0.1, 1e-6));
        start(nullptr);
        iterate(2);
        close();
    }
    // ---- 9. refusals, one at a time
    if (open("sqp 9: refusals", 0, false)) return 1;
    show(h, "start before setup", almpc_sqp_fnn_start(h, x0.data(), nullptr));
    show(h, "iterate before setup", almpc_sqp_fnn_iterate(h, 1, 1.0, nullptr, nullptr, nullptr));
    show(h, "solve before setup", almpc_sqp_fnn_solve(h, 1, 1e-6, nullptr, nullptr, nullptr, nullptr));
    show(h, "state_multipliers before setup", almpc_sqp_fnn_state_multipliers(h, mu.data()));
    show(h, "skipped before setup", almpc_sqp_fnn_skipped(h, sk.data()));
    show(h, "set_hessian 2", almpc_sqp_fnn_set_hessian(h, 2));
    show(h, "set_step_rule 2", almpc_sqp_fnn_set_step_rule(h, 2));
    sqp(p, nullptr, TANH);
    show(h, "iterate before start", almpc_sqp_fnn_iterate(h, 1, 1.0, nullptr, nullptr, nullptr));
    show(h, "solve before start", almpc_sqp_fnn_solve(h, 1, 1e-6, nullptr, nullptr, nullptr, nullptr));
    show(h, "start, x0 null", almpc_sqp_fnn_start(h, nullptr, nullptr));
    start(nullptr);
    show(h, "iterate, iters 0", almpc_sqp_fnn_iterate(h, 0, 1.0, nullptr, nullptr, nullptr));
    show(h, "iterate, step_scale 0", almpc_sqp_fnn_iterate(h, 1, 0.0, nullptr, nullptr, nullptr));
    show(h, "iterate, step_scale 1.5", almpc_sqp_fnn_iterate(h, 1, 1.5, nullptr, nullptr, nullptr));
    show(h, "solve, max_iters 0", almpc_sqp_fnn_solve(h, 0, 1e-6, nullptr, nullptr, nullptr, nullptr));
    show(h, "solve, tol 0", almpc_sqp_fnn_solve(h, 1, 0.0, nullptr, nullptr, nullptr, nullptr));
    {
        Plant r0 = p;
        r0.R[0] = 0.0;
        sqp(r0, nullptr, TANH); start(nullptr);
        show(h, "solve, R[0,0] = 0", almpc_sqp_fnn_solve(h, 1, 1e-6, nullptr, nullptr, nullptr, nullptr));
        iterate(1);
    }
    sqp(p, nullptr, 1);   // relu
    show(h, "set_hessian exact, relu", almpc_sqp_fnn_set_hessian(h, 1));
    close();
    if (open("sqp 9: exact asked for before a relu setup", 0, false)) return 1;
    hessian(1);
    sqp(p, nullptr, 1); start(nullptr);
    iterate(1); solve(1);
    close();
    if (open("sqp 9: exact with state rows", 0, true)) return 1;
    sqp(p, nullptr, TANH);
    show(h, "set_hessian exact, no row multipliers", almpc_sqp_fnn_set_hessian(h, 1));
    close();
    if (open("sqp 9: exact with state rows and their multipliers, fallback off", 0, true)) return 1;
    show(h, "set_structured_fallback 0", almpc_set_structured_fallback(h, 0));
    sqp(p, nullptr, TANH); rows_on();
    show(h, "set_hessian exact, no fallback", almpc_sqp_fnn_set_hessian(h, 1));
    close();
    if (open("sqp 9: exact on the stage-wise route", ALMPC_FLAG_STRUCTURED, false)) return 1;
    sqp(p, nullptr, TANH);
    show(h, "set_hessian exact, structured", almpc_sqp_fnn_set_hessian(h, 1));
    close();
    // ---- 10 - 14. the re-linearised step: as set up, with every instance's own terminal weight, with a continuous-time network
    const auto relin_walk = [&] {
        show(h, "relin_fnn_setup", almpc_relin_fnn_setup(h, Hn, L, TANH, W_in.data(), W_h.data(), b_h.data(), W_out.data(), xr.data(), ur.data(), p.Q.data(), p.R.data(),
                                                         p.S.data(), P.data(), p.umin.data(), p.umax.data(), 0.1, 1e-6));
        float a = 0, b = 0, c = 0;
        show(h, "  update_initialization", almpc_update_initialization(h, x0.data()));
        show(h, "  relin_fnn_step cold", almpc_relin_fnn_step(h, &cold));
        show(h, "  update_initialization", almpc_update_initialization(h, x0.data()));
        show(h, "  relin_fnn_step warm", almpc_relin_fnn_step(h, &warm));
        show(h, "  relin_fnn_timing", almpc_relin_fnn_timing(h, &a, &b, &c));
        show(h, "  relin_fnn_advance", almpc_relin_fnn_advance(h));
        show(h, "  update_initialization", almpc_update_initialization(h, x0.data()));
        show(h, "  relin_fnn_step warm", almpc_relin_fnn_step(h, &warm));
    };
    for (int variant = 0; variant < 3; ++variant)
        for (int kind = 0; kind < 3; ++kind) {
            const char* const titles[3][3] = {{"relin 10: condensed, timing", "relin 11: condensed, state box", "relin 12: structured, timing"},
                                              {"relin 13: condensed, timing, DARE on the device", "relin 13: condensed, state box, DARE on the device", "relin 13: structured, timing, DARE on the device"},
                                              {"relin 14: condensed, timing, continuous time", "relin 14: condensed, state box, continuous time", "relin 14: structured, timing, continuous time"}};
            if (open(titles[variant][kind], kind == 2 ? ALMPC_FLAG_STRUCTURED | ALMPC_FLAG_TIMING : (kind == 0 ? ALMPC_FLAG_TIMING : 0u), kind == 1)) return 1;
            if (variant == 1) show(h, "set_terminal_weight", almpc_set_terminal_weight(h, ALMPC_TERMINAL_DARE_DEVICE));
            if (variant == 2) show(h, "set_model_time", almpc_set_model_time(h, ALMPC_MODEL_CONTINUOUS_ZOH, 0.1));
            relin_walk();
            close();
        }
    // ---- 15. the `warm` predicate without a polish; calls out of order
    if (open("relin 15: no polish, calls out of order", 0, false)) return 1;
    show(h, "relin_fnn_step before setup", almpc_relin_fnn_step(h, &cold));
    show(h, "relin_fnn_advance before setup", almpc_relin_fnn_advance(h));
    show(h, "relin_fnn_setup", almpc_relin_fnn_setup(h, Hn, L, TANH, W_in.data(), W_h.data(), b_h.data(), W_out.data(), xr.data(), ur.data(), p.Q.data(), p.R.data(),
                                                     p.S.data(), P.data(), p.umin.data(), p.umax.data(), 0.1, 1e-6));
    show(h, "relin_fnn_advance before a step", almpc_relin_fnn_advance(h));
    show(h, "  update_initialization", almpc_update_initialization(h, x0.data()));
    show(h, "  relin_fnn_step cold", almpc_relin_fnn_step(h, &cold));
    almpc_opts rough = warm;
    rough.polish = 0;
    show(h, "  update_initialization", almpc_update_initialization(h, x0.data()));
    show(h, "  relin_fnn_step warm_start 1, polish 0", almpc_relin_fnn_step(h, &rough));
    show(h, "  relin_fnn_step, opts null", almpc_relin_fnn_step(h, nullptr));
    close();
    fake_hip_record_uploads(0);
    std::printf("loops ok\n");
    return 0;
}

int main(int argc, char** argv) {
    {   // every almpc_create below reads the switches: none may come in from the caller's environment
        std::vector<std::string> inherited;
        for (char** e = environ; *e; ++e)
            if (std::strncmp(*e, "ALMPC_", 6) == 0) inherited.emplace_back(*e, std::strchr(*e, '=') - *e);
        for (const std::string& name : inherited) unsetenv(name.c_str());
    }
    if (argc > 1 && fake_hip_trace_to(argv[1])) { std::fprintf(stderr, "cannot write %s\n", argv[1]); return 1; }
    if (argc > 2 && std::strcmp(argv[2], "alloc-failures") == 0) return alloc_failures();
    if (argc > 2 && std::strcmp(argv[2], "setups") == 0) {
        if (setups()) return 1;
        fake_hip_trace_close();
        return fake_hip_dump_allocs((std::string(argv[1]) + ".allocs").c_str());
    }
    if (argc > 2 && std::strcmp(argv[2], "loops") == 0) {
        const char* const sw = argc > 3 ? std::strchr(argv[3], '=') : nullptr;
        if (argc > 3 && (!sw || setenv(std::string(argv[3], sw - argv[3]).c_str(), sw + 1, 1))) { std::fprintf(stderr, "not NAME=VALUE: %s\n", argv[3]); return 1; }
        if (loops()) return 1;
        fake_hip_trace_close();
        return fake_hip_dump_allocs((std::string(argv[1]) + ".allocs").c_str());
    }
    const char* const eq = argc > 2 ? std::strchr(argv[2], '=') : nullptr;
    if (argc > 2 && (!eq || setenv(std::string(argv[2], eq - argv[2]).c_str(), eq + 1, 1))) { std::fprintf(stderr, "not NAME=VALUE: %s\n", argv[2]); return 1; }
    almpc_handle* h = nullptr;
    // ---- shared model, input box; then state box + terminal equality + S on the same handle; closed loop on the device
    {
        const int n = 4, m = 2, N = 12, batch = 37;
        const Plant p = chain(n, m);
        CK(almpc_create(&h, n, m, N, batch, 0, ALMPC_FLAG_TIMING));
        CK(almpc_set_rho_profile(h, 1));
        CK(almpc_design_shared(h, p.A.data(), p.B.data(), p.Q.data(), p.R.data(), nullptr, nullptr, p.umin.data(), p.umax.data(), nullptr, nullptr, 30.0, 1e-6));
        std::vector<double> xr((size_t)n * (N + 1), 0.1), ur((size_t)m * N, 0.05);
        for (int k = 0; k < N; ++k) ur[(size_t)k * m] = 0.01 * k;   // horizon-varying input reference
        CK(almpc_set_reference(h, xr.data(), ur.data(), 0));
        almpc_opts o;
        almpc_default_opts(&o);
        o.rho = 30.0;
        std::vector<double> x0((size_t)batch * n, 0.25);
        CK(almpc_update_initialization(h, x0.data()));
        CK(almpc_calculate(h, &o));
        CK(almpc_advance_plant(h));
        o.warm_start = 1;
        CK(almpc_calculate(h, &o));
        std::vector<double> H((size_t)m * N * m * N), F((size_t)m * N * n), P((size_t)n * n), d((size_t)m * N);
        CK(almpc_get_design(h, H.data(), F.data(), P.data(), d.data()));
        CK(almpc_set_terminal_equality(h, 1));
        CK(almpc_design_shared(h, p.A.data(), p.B.data(), p.Q.data(), p.R.data(), p.S.data(), nullptr, p.umin.data(), p.umax.data(), p.xmin.data(), p.xmax.data(), 0.1, 1e-6));
        std::vector<double> xrb((size_t)batch * n * (N + 1), 0.0), urb((size_t)batch * m * N, 0.0);
        CK(almpc_set_reference(h, xrb.data(), urb.data(), 1));   // per-instance references
        if (step_and_read(h, n, m, N, batch, true)) return 1;
        almpc_destroy(h); h = nullptr;
    }
    // ---- the benchmark shape (fused one-kernel step, nz = 120) and the per-instance-model path on it
    {
        const int n = 12, m = 4, N = 30, batch = 48;
        const Plant p = chain(n, m);
        CK(almpc_create(&h, n, m, N, batch, 0, 0));
        CK(almpc_design_shared(h, p.A.data(), p.B.data(), p.Q.data(), p.R.data(), nullptr, nullptr, p.umin.data(), p.umax.data(), nullptr, nullptr, 0.1, 1e-6));
        std::vector<double> xz((size_t)n * (N + 1), 0.0), uz((size_t)m * N, 0.0);
        CK(almpc_set_reference(h, xz.data(), uz.data(), 0));
        if (step_and_read(h, n, m, N, batch, true)) return 1;
        almpc_opts o;
        almpc_default_opts(&o);
        CK(almpc_set_step_fusion(h, 0));   // two launches: ADMM, then k_polish<true>
        CK(almpc_calculate(h, &o));
        o.polish = 0;                      // no polish: ADMM + k_rollout<4>
        CK(almpc_calculate(h, &o));
        CK(almpc_set_step_fusion(h, 1));
        std::vector<double> Ab((size_t)batch * n * n), Bb((size_t)batch * n * m);
        for (int i = 0; i < batch; ++i) {
            for (size_t t = 0; t < p.A.size(); ++t) Ab[(size_t)i * n * n + t] = p.A[t];
            for (size_t t = 0; t < p.B.size(); ++t) Bb[(size_t)i * n * m + t] = p.B[t] * (1.0 + 0.01 * i);
        }
        CK(almpc_set_state_box(h, p.xmin.data(), p.xmax.data()));
        CK(almpc_design_batched(h, Ab.data(), Bb.data(), p.Q.data(), p.R.data(), nullptr, nullptr, 0, p.umin.data(), p.umax.data(), 0.1, 1e-6));
        CK(almpc_set_reference(h, xz.data(), uz.data(), 0));
        if (step_and_read(h, n, m, N, batch, false)) return 1;
        std::vector<double> Hi((size_t)m * N * m * N), Fi((size_t)m * N * n), di((size_t)m * N);
        CK(almpc_get_design_instance(h, batch - 1, Hi.data(), Fi.data(), di.data()));
        almpc_destroy(h); h = nullptr;
    }
    // ---- structured handle beyond the condensed horizon (m N = 200), state box + S
    {
        const int n = 12, m = 4, N = 50, batch = 21;
        const Plant p = chain(n, m);
        CK(almpc_create(&h, n, m, N, batch, 0, ALMPC_FLAG_STRUCTURED));
        CK(almpc_design_shared(h, p.A.data(), p.B.data(), p.Q.data(), p.R.data(), p.S.data(), nullptr, p.umin.data(), p.umax.data(), p.xmin.data(), p.xmax.data(), 0.1, 1e-6));
        std::vector<double> xz((size_t)n * (N + 1), 0.0), uz((size_t)m * N, 0.0);
        CK(almpc_set_reference(h, xz.data(), uz.data(), 0));
        if (step_and_read(h, n, m, N, batch, true)) return 1;
        almpc_opts o;
        almpc_default_opts(&o);
        o.warm_start = 1;   // receding-horizon start from the previous inputs (k_guess_from_inputs)
        CK(almpc_calculate(h, &o));
        almpc_destroy(h); h = nullptr;
    }
    // ---- shared model, nz = 80, G through L2 (k_polish<false>), redo enqueued behind the step (ALMPC_EAGER_REDO)
    {
        const int n = 4, m = 2, N = 40, batch = 20;
        const Plant p = chain(n, m);
        setenv("ALMPC_POLISH_NO_GLDS", "1", 1);   // (a handle's switches are what almpc_create finds)
        setenv("ALMPC_EAGER_REDO", "1", 1);
        CK(almpc_create(&h, n, m, N, batch, 0, 0));
        CK(almpc_design_shared(h, p.A.data(), p.B.data(), p.Q.data(), p.R.data(), nullptr, nullptr, p.umin.data(), p.umax.data(), nullptr, nullptr, 0.1, 1e-6));
        std::vector<double> xz((size_t)n * (N + 1), 0.0), uz((size_t)m * N, 0.0);
        CK(almpc_set_reference(h, xz.data(), uz.data(), 0));
        if (step_and_read(h, n, m, N, batch, false)) return 1;
        almpc_destroy(h); h = nullptr;
        unsetenv("ALMPC_POLISH_NO_GLDS");
        unsetenv("ALMPC_EAGER_REDO");
    }
    // ---- per-instance models, nz = 40, no polish: k_admm_inst with the full inverse, then k_rollout<1>
    {
        const int n = 4, m = 2, N = 20, batch = 9;
        const Plant p = chain(n, m);
        CK(almpc_create(&h, n, m, N, batch, 0, 0));
        std::vector<double> Ab((size_t)batch * n * n), Bb((size_t)batch * n * m);
        for (int i = 0; i < batch; ++i) {
            for (size_t t = 0; t < p.A.size(); ++t) Ab[(size_t)i * n * n + t] = p.A[t];
            for (size_t t = 0; t < p.B.size(); ++t) Bb[(size_t)i * n * m + t] = p.B[t] * (1.0 + 0.01 * i);
        }
        CK(almpc_design_batched(h, Ab.data(), Bb.data(), p.Q.data(), p.R.data(), nullptr, nullptr, 0, p.umin.data(), p.umax.data(), 0.1, 1e-6));
        std::vector<double> xz((size_t)n * (N + 1), 0.0), uz((size_t)m * N, 0.0), x0((size_t)batch * n, 0.25);
        CK(almpc_set_reference(h, xz.data(), uz.data(), 0));
        CK(almpc_update_initialization(h, x0.data()));
        almpc_opts o;
        almpc_default_opts(&o);
        o.polish = 0;
        CK(almpc_calculate(h, &o));
        almpc_destroy(h); h = nullptr;
    }
    // ---- re-linearisation pipeline and SQP loop on a small network
    {
        const int n = 4, m = 2, N = 20, batch = 19, Hn = 8, L = 2;
        const Plant p = chain(n, m);
        std::vector<double> W_in((size_t)Hn * (n + m), 0.05), W_h((size_t)L * Hn * Hn, 0.02), b_h((size_t)L * Hn, 0.01), W_out((size_t)n * Hn, 0.1);
        std::vector<double> P((size_t)n * n, 0.0), xr((size_t)n * (N + 1), 0.0), ur((size_t)m * N, 0.0);
        for (int i = 0; i < n; ++i) P[(size_t)i * n + i] = 150.0;
        for (int k = 0; k < N; ++k) ur[(size_t)k * m + 1] = 0.02 * k;
        CK(almpc_create(&h, n, m, N, batch, 0, ALMPC_FLAG_TIMING));
        CK(almpc_relin_fnn_setup(h, Hn, L, 0, W_in.data(), W_h.data(), b_h.data(), W_out.data(), xr.data(), ur.data(), p.Q.data(), p.R.data(), p.S.data(),
                                 P.data(), p.umin.data(), p.umax.data(), 0.1, 1e-6));
        std::vector<double> x0((size_t)batch * n, 0.1);
        CK(almpc_update_initialization(h, x0.data()));
        almpc_opts o;
        almpc_default_opts(&o);
        CK(almpc_relin_fnn_step(h, &o));
        CK(almpc_relin_fnn_advance(h));
        o.warm_start = 1;
        CK(almpc_relin_fnn_step(h, &o));
        float a, b, c;
        CK(almpc_relin_fnn_timing(h, &a, &b, &c));
        CK(almpc_sqp_fnn_setup(h, Hn, L, 1, W_in.data(), W_h.data(), b_h.data(), W_out.data(), xr.data(), ur.data(), p.Q.data(), p.R.data(), nullptr,
                               P.data(), 0, p.umin.data(), p.umax.data(), 0.1, 1e-6));
        CK(almpc_sqp_fnn_start(h, x0.data(), nullptr));
        std::vector<double> si(3), di(3);
        const int rc = almpc_sqp_fnn_iterate(h, 3, 1.0, nullptr, si.data(), di.data());
        if (rc != ALMPC_OK && rc != ALMPC_ERR_NUMERIC) { std::fprintf(stderr, "sqp iterate -> %d (%s)\n", rc, almpc_last_error(h)); return 1; }
        std::vector<int32_t> sk(batch);
        CK(almpc_sqp_fnn_skipped(h, sk.data()));
        almpc_destroy(h); h = nullptr;
    }
    // ---- SQP loop with nz = 80: the first iteration's ADMM + k_polish_sgl<0>, then k_guess_iterate_ws + k_polish_sgl<1>
    {
        const int n = 4, m = 2, N = 40, batch = 11, Hn = 8, L = 2;
        const Plant p = chain(n, m);
        std::vector<double> W_in((size_t)Hn * (n + m), 0.05), W_h((size_t)L * Hn * Hn, 0.02), b_h((size_t)L * Hn, 0.01), W_out((size_t)n * Hn, 0.1);
        std::vector<double> P((size_t)n * n, 0.0), xr((size_t)n * (N + 1), 0.0), ur((size_t)m * N, 0.0), x0((size_t)batch * n, 0.1);
        for (int i = 0; i < n; ++i) P[(size_t)i * n + i] = 150.0;
        CK(almpc_create(&h, n, m, N, batch, 0, 0));
        CK(almpc_sqp_fnn_setup(h, Hn, L, 1, W_in.data(), W_h.data(), b_h.data(), W_out.data(), xr.data(), ur.data(), p.Q.data(), p.R.data(), nullptr,
                               P.data(), 0, p.umin.data(), p.umax.data(), 0.1, 1e-6));
        CK(almpc_sqp_fnn_start(h, x0.data(), nullptr));
        std::vector<double> si(3), di(3);
        const int rc = almpc_sqp_fnn_iterate(h, 3, 1.0, nullptr, si.data(), di.data());
        if (rc != ALMPC_OK && rc != ALMPC_ERR_NUMERIC) { std::fprintf(stderr, "sqp iterate -> %d (%s)\n", rc, almpc_last_error(h)); return 1; }
        almpc_destroy(h); h = nullptr;
    }
    // ---- a group of three handles (all on the one fake device): uneven shards, tickets
    {
        almpc_group* g = nullptr;
        const int n = 4, m = 2, N = 10, batch = 50, ids[3] = {0, 0, 0};
        const Plant p = chain(n, m);
        CKG(almpc_group_create(&g, n, m, N, batch, 3, ids, 0));
        CKG(almpc_group_design_shared(g, p.A.data(), p.B.data(), p.Q.data(), p.R.data(), nullptr, nullptr, p.umin.data(), p.umax.data(), nullptr, nullptr, 0.1, 1e-6));
        std::vector<double> xz((size_t)n * (N + 1), 0.0), uz((size_t)m * N, 0.0);
        CKG(almpc_group_set_reference(g, xz.data(), uz.data(), 0));
        std::vector<double> x0((size_t)batch * n, 0.2), x((size_t)batch * n * (N + 1)), u((size_t)batch * m * N), u0((size_t)batch * m);
        std::vector<int32_t> st(batch);
        CKG(almpc_group_update_initialization(g, x0.data()));
        CKG(almpc_group_calculate(g, nullptr));
        CKG(almpc_group_get_results(g, x.data(), nullptr, u.data(), nullptr, u0.data(), st.data(), nullptr, nullptr));
        CKG(almpc_group_calculate_async(g, nullptr));
        const int t = almpc_group_get_results_async(g, ALMPC_WANT_FIRST_INPUT | ALMPC_WANT_STATUS | ALMPC_WANT_X);
        if (t < 0) return 1;
        CKG(almpc_group_get_results_wait(g, t, x.data(), nullptr, nullptr, nullptr, u0.data(), st.data(), nullptr, nullptr));
        CKG(almpc_group_advance_plant(g));
        almpc_group_destroy(g);
    }
    // ---- small shared problems, nz = 10: more than two instances per CU (the fake device has 256) take the two-launch path, unless
    // ALMPC_SHARED_WAVE_MAX_BATCH moves the limit
    {
        const int n = 4, m = 2, N = 5, batch = 600;
        const Plant p = chain(n, m);
        CK(almpc_create(&h, n, m, N, batch, 0, 0));
        CK(almpc_design_shared(h, p.A.data(), p.B.data(), p.Q.data(), p.R.data(), nullptr, nullptr, p.umin.data(), p.umax.data(), nullptr, nullptr, 0.1, 1e-6));
        if (step_and_read(h, n, m, N, batch, false)) return 1;
        almpc_destroy(h); h = nullptr;
    }
    // ---- a switch belongs to the handle, fixed when almpc_create returns: set behind it, ALMPC_NO_SHARED_WAVE does not move the first
    // handle off k_step_inst_wave; a handle created while it is set takes the two-launch path.  (Without a switch argument only: the
    // runs under one switch keep the environment still while a handle lives.)
    if (argc <= 2) {
        const int n = 4, m = 2, N = 5, batch = 8;
        const Plant p = chain(n, m);
        almpc_handle* h2 = nullptr;
        CK(almpc_create(&h, n, m, N, batch, 0, 0));
        CK(almpc_design_shared(h, p.A.data(), p.B.data(), p.Q.data(), p.R.data(), nullptr, nullptr, p.umin.data(), p.umax.data(), nullptr, nullptr, 0.1, 1e-6));
        setenv("ALMPC_NO_SHARED_WAVE", "1", 1);
        if (step_and_read(h, n, m, N, batch, false)) return 1;
        if (almpc_create(&h2, n, m, N, batch, 0, 0) != ALMPC_OK) return 1;
        unsetenv("ALMPC_NO_SHARED_WAVE");
        almpc_destroy(h); h = h2;
        CK(almpc_design_shared(h, p.A.data(), p.B.data(), p.Q.data(), p.R.data(), nullptr, nullptr, p.umin.data(), p.umax.data(), nullptr, nullptr, 0.1, 1e-6));
        if (step_and_read(h, n, m, N, batch, false)) return 1;
        almpc_destroy(h); h = nullptr;
    }
    fake_hip_trace_close();
    if (argc > 1 && fake_hip_dump_allocs((std::string(argv[1]) + ".allocs").c_str())) { std::fprintf(stderr, "cannot write %s.allocs\n", argv[1]); return 1; }
    std::printf("host logic ok: %ld launches\n", fake_hip_launch_count());
    return 0;
}
