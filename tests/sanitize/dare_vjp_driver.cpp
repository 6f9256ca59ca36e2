// Sanitizer driver for the adjoint of the DARE in the library's design-time host math (csrc/almpc_host_math.h: hm::dare_vjp): compiled by
// tests/test_dare_vjp_host.py with -fsanitize=address,undefined; reads n, m, A, B, Q, R, P, gP and prints the status, then gA, gB, gQ, gR.
// Test infrastructure only.
#include "../../automationlabsmodelpredictivecontrol.jl_amd/csrc/almpc_host_math.h"

#include <cstdio>
#include <cstdlib>
using namespace almpc::hm;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int n, m;
    if (std::fscanf(f, "%d %d", &n, &m) != 2) return 2;
    auto rd = [&](size_t cnt) { mat v(cnt); for (auto& x : v) if (std::fscanf(f, "%lf", &x) != 1) std::exit(2); return v; };
    mat A = rd((size_t)n * n), B = rd((size_t)n * m), Q = rd((size_t)n * n), R = rd((size_t)m * m), P = rd((size_t)n * n), gP = rd((size_t)n * n);
    std::fclose(f);
    mat gA, gB, gQ, gR;
    const int st = dare_vjp(A, B, Q, R, P, gP, n, m, &gA, &gB, &gQ, &gR);
    std::printf("%d\n", st);
    if (st == 0)
        for (const mat* g : {&gA, &gB, &gQ, &gR})
            for (double v : *g) std::printf("%.17g\n", v);
    return dare_vjp(A, B, Q, R, P, gP, n, m, nullptr, nullptr, nullptr, nullptr) == st ? 0 : 3;   // (null outputs are skipped)
}
