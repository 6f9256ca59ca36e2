// Driver of the CPU sanitizer build of the library's HOST half for the state-row multipliers of the SQP loop
// (almpc_sqp_fnn_set_row_multipliers, almpc_sqp_fnn_state_multipliers and their group forms): csrc/almpc_api.hip compiled host-only under
// AddressSanitizer + UndefinedBehaviorSanitizer and linked against tests/sanitize/fake_hip_runtime.cpp, as host_logic_driver.cpp is (device
// memory = calloc'd host memory, launches = no-ops, so every buffer the switch sizes, zeroes and reads back is bounds-checked).  Walks the
// switch on a state-box handle (iterate, solve, both Hessians, read-back before and after), its refusals, a handle without state rows,
// the terminal equality alone, and a group of three.  Prints "rows host logic ok: <launches> launches".
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

struct Net {
    int n, m, N, Hn, L;
    std::vector<double> W_in, W_h, b_h, W_out, Q, R, P, xr, ur, umin, umax, xmin, xmax;
};

static Net net(int n, int m, int N) {
    Net t;
    t.n = n; t.m = m; t.N = N; t.Hn = 8; t.L = 2;
    t.W_in.assign((size_t)t.Hn * (n + m), 0.05); t.W_h.assign((size_t)t.L * t.Hn * t.Hn, 0.02); t.b_h.assign((size_t)t.L * t.Hn, 0.01);
    t.W_out.assign((size_t)n * t.Hn, 0.1);
    t.Q.assign((size_t)n * n, 0.0); t.R.assign((size_t)m * m, 0.0); t.P.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) { t.Q[(size_t)i * n + i] = 100.0; t.P[(size_t)i * n + i] = 150.0; }
    for (int a = 0; a < m; ++a) t.R[(size_t)a * m + a] = 0.1;
    t.xr.assign((size_t)n * (N + 1), 0.0); t.ur.assign((size_t)m * N, 0.0);
    t.umin.assign(m, -1.0); t.umax.assign(m, 1.0); t.xmin.assign(n, -3.0); t.xmax.assign(n, 3.0);
    return t;
}

static int setup(almpc_handle* h, const Net& t) {
    return almpc_sqp_fnn_setup(h, t.Hn, t.L, 2, t.W_in.data(), t.W_h.data(), t.b_h.data(), t.W_out.data(), t.xr.data(), t.ur.data(), t.Q.data(),
                               t.R.data(), nullptr, t.P.data(), 0, t.umin.data(), t.umax.data(), 0.1, 1e-6);
}

static bool all_zero(const std::vector<double>& v) {
    for (double a : v)
        if (a != 0.0) return false;
    return true;
}

int main() {
    {   // every almpc_create below reads the switches: none may come in from the caller's environment
        std::vector<std::string> inherited;
        for (char** e = environ; *e; ++e)
            if (std::strncmp(*e, "ALMPC_", 6) == 0) inherited.emplace_back(*e, std::strchr(*e, '=') - *e);
        for (const std::string& name : inherited) unsetenv(name.c_str());
    }
    almpc_handle* h = nullptr;
    EXPECT(almpc_sqp_fnn_set_row_multipliers(nullptr, 1), ALMPC_ERR_INVALID);
    EXPECT(almpc_sqp_fnn_state_multipliers(nullptr, nullptr), ALMPC_ERR_INVALID);
    EXPECT(almpc_group_sqp_fnn_set_row_multipliers(nullptr, 1), ALMPC_ERR_INVALID);
    EXPECT(almpc_group_sqp_fnn_state_multipliers(nullptr, nullptr), ALMPC_ERR_INVALID);
    // ---- state box: the switch before the setup, read-backs, iterate, solve, both Hessians
    {
        const int n = 4, m = 2, N = 20, batch = 19;
        const Net t = net(n, m, N);
        std::vector<double> x0((size_t)batch * n, 0.1), mu((size_t)batch * N * n, 1.0), kkt(batch);
        std::vector<int32_t> st(batch), it(batch);
        CK(almpc_create(&h, n, m, N, batch, 0, 0));
        EXPECT(almpc_sqp_fnn_state_multipliers(h, mu.data()), ALMPC_ERR_NOT_DESIGNED);
        CK(almpc_set_state_box(h, t.xmin.data(), t.xmax.data()));
        CK(almpc_sqp_fnn_set_row_multipliers(h, 1));
        CK(setup(h, t));
        EXPECT(almpc_sqp_fnn_state_multipliers(h, nullptr), ALMPC_ERR_INVALID);
        CK(almpc_sqp_fnn_state_multipliers(h, mu.data()));   // before the start: zeros, no buffer yet
        if (!all_zero(mu)) return 1;
        CK(almpc_sqp_fnn_start(h, x0.data(), nullptr));
        mu.assign(mu.size(), 1.0);
        CK(almpc_sqp_fnn_state_multipliers(h, mu.data()));   // before the first QP: the zeroed buffer
        if (!all_zero(mu)) return 1;
        std::vector<double> si(2), di(2);
        const int rc = almpc_sqp_fnn_iterate(h, 2, 1.0, nullptr, si.data(), di.data());
        if (rc != ALMPC_OK && rc != ALMPC_ERR_NUMERIC) { std::fprintf(stderr, "iterate -> %d (%s)\n", rc, almpc_last_error(h)); return 1; }
        CK(almpc_sqp_fnn_state_multipliers(h, mu.data()));
        CK(almpc_sqp_fnn_set_step_rule(h, 1));
        CK(almpc_sqp_fnn_solve(h, 3, 1e-6, nullptr, st.data(), it.data(), kkt.data()));
        CK(almpc_sqp_fnn_set_hessian(h, ALMPC_SQP_HESSIAN_EXACT));   // state rows with their multipliers: accepted
        CK(almpc_sqp_fnn_start(h, x0.data(), nullptr));
        CK(almpc_sqp_fnn_solve(h, 3, 1e-6, nullptr, st.data(), it.data(), kkt.data()));
        const int rc2 = almpc_sqp_fnn_iterate(h, 2, 1.0, nullptr, si.data(), di.data());
        if (rc2 != ALMPC_OK && rc2 != ALMPC_ERR_NUMERIC) { std::fprintf(stderr, "iterate -> %d (%s)\n", rc2, almpc_last_error(h)); return 1; }
        CK(almpc_sqp_fnn_state_multipliers(h, mu.data()));
        // a new setup keeps the switch; switched off, the exact mode is refused at the next solve and at set_hessian
        CK(setup(h, t));
        CK(almpc_sqp_fnn_start(h, x0.data(), nullptr));
        CK(almpc_sqp_fnn_solve(h, 2, 1e-6, nullptr, st.data(), it.data(), kkt.data()));
        CK(almpc_sqp_fnn_set_row_multipliers(h, 0));
        EXPECT(almpc_sqp_fnn_solve(h, 2, 1e-6, nullptr, st.data(), it.data(), kkt.data()), ALMPC_ERR_UNSUPPORTED);
        CK(almpc_sqp_fnn_set_hessian(h, ALMPC_SQP_HESSIAN_GAUSS_NEWTON));
        EXPECT(almpc_sqp_fnn_set_hessian(h, ALMPC_SQP_HESSIAN_EXACT), ALMPC_ERR_UNSUPPORTED);
        CK(almpc_sqp_fnn_solve(h, 2, 1e-6, nullptr, st.data(), it.data(), kkt.data()));
        // switched on AFTER setup and start: the buffer appears with the next loop
        CK(almpc_sqp_fnn_set_row_multipliers(h, 1));
        CK(almpc_sqp_fnn_solve(h, 2, 1e-6, nullptr, st.data(), it.data(), kkt.data()));
        CK(almpc_sqp_fnn_state_multipliers(h, mu.data()));
        // without the stage-wise fallback the exact mode with state rows has nowhere to send an indefinite iteration
        CK(almpc_set_structured_fallback(h, 0));
        CK(setup(h, t));
        EXPECT(almpc_sqp_fnn_set_hessian(h, ALMPC_SQP_HESSIAN_EXACT), ALMPC_ERR_UNSUPPORTED);
        // the stage-wise QP route does not hand the multipliers out
        CK(almpc_set_structured_fallback(h, 1));
        CK(almpc_sqp_fnn_set_structured(h, 1));
        CK(setup(h, t));
        CK(almpc_sqp_fnn_start(h, x0.data(), nullptr));
        EXPECT(almpc_sqp_fnn_solve(h, 2, 1e-6, nullptr, st.data(), it.data(), kkt.data()), ALMPC_ERR_UNSUPPORTED);
        CK(almpc_sqp_fnn_set_row_multipliers(h, 0));
        CK(almpc_sqp_fnn_solve(h, 2, 1e-6, nullptr, st.data(), it.data(), kkt.data()));
        almpc_destroy(h); h = nullptr;
    }
    // ---- the terminal equality alone (n rows), and a handle without state rows (the switch changes nothing)
    {
        const int n = 4, m = 2, N = 8, batch = 5;
        const Net t = net(n, m, N);
        std::vector<double> x0((size_t)batch * n, 0.1), mu((size_t)batch * N * n, 1.0), kkt(batch);
        std::vector<int32_t> st(batch), it(batch);
        CK(almpc_create(&h, n, m, N, batch, 0, 0));
        CK(almpc_set_terminal_equality(h, 1));
        CK(setup(h, t));
        CK(almpc_sqp_fnn_set_row_multipliers(h, 1));
        CK(almpc_sqp_fnn_set_hessian(h, ALMPC_SQP_HESSIAN_EXACT));
        CK(almpc_sqp_fnn_start(h, x0.data(), nullptr));
        CK(almpc_sqp_fnn_solve(h, 3, 1e-6, nullptr, st.data(), it.data(), kkt.data()));
        CK(almpc_sqp_fnn_state_multipliers(h, mu.data()));
        CK(almpc_set_terminal_equality(h, 0));
        CK(setup(h, t));
        CK(almpc_sqp_fnn_start(h, x0.data(), nullptr));
        CK(almpc_sqp_fnn_solve(h, 3, 1e-6, nullptr, st.data(), it.data(), kkt.data()));
        mu.assign(mu.size(), 1.0);
        CK(almpc_sqp_fnn_state_multipliers(h, mu.data()));
        if (!all_zero(mu)) return 1;
        almpc_destroy(h); h = nullptr;
    }
    // ---- a group of three handles, uneven shards
    {
        almpc_group* g = nullptr;
        const int n = 4, m = 2, N = 10, batch = 50, ids[3] = {0, 0, 0};
        const Net t = net(n, m, N);
        std::vector<double> x0((size_t)batch * n, 0.1), mu((size_t)batch * N * n, 1.0), kkt(batch);
        std::vector<int32_t> st(batch), it(batch);
        CKG(almpc_group_create(&g, n, m, N, batch, 3, ids, 0));
        CKG(almpc_group_set_state_box(g, t.xmin.data(), t.xmax.data()));
        CKG(almpc_group_sqp_fnn_set_row_multipliers(g, 1));
        CKG(almpc_group_sqp_fnn_setup(g, t.Hn, t.L, 2, t.W_in.data(), t.W_h.data(), t.b_h.data(), t.W_out.data(), t.xr.data(), t.ur.data(),
                                      t.Q.data(), t.R.data(), nullptr, t.P.data(), 0, t.umin.data(), t.umax.data(), 0.1, 1e-6));
        CKG(almpc_group_sqp_fnn_set_hessian(g, ALMPC_SQP_HESSIAN_EXACT));
        CKG(almpc_group_sqp_fnn_start(g, x0.data(), nullptr));
        CKG(almpc_group_sqp_fnn_set_step_rule(g, 1));
        CKG(almpc_group_sqp_fnn_solve(g, 3, 1e-6, nullptr, st.data(), it.data(), kkt.data()));
        EXPECT(almpc_group_sqp_fnn_state_multipliers(g, nullptr), ALMPC_ERR_INVALID);
        CKG(almpc_group_sqp_fnn_state_multipliers(g, mu.data()));
        if (!all_zero(mu)) return 1;   // (no kernel ran: the zeroed buffers, every shard's slice written)
        almpc_group_destroy(g);
    }
    std::printf("rows host logic ok: %ld launches\n", fake_hip_launch_count());
    return 0;
}
