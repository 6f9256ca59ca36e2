// c2d_driver.cpp -- hm::c2d (csrc/almpc_host_math.h) under AddressSanitizer / UndefinedBehaviorSanitizer: a stand-alone program that
// discretises random continuous-time models of every shape of tests/test_c2d_host.py at three sample times, checks the double
// integrator (exact) and the three refusals, and prints "c2d host math ok: <models>".  Built and run by tests/test_sanitizers_c2d.py.
#include <cmath>
#include <cstdio>
#include <limits>

#include "../../automationlabsmodelpredictivecontrol.jl_amd/csrc/almpc_host_math.h"

using almpc::hm::mat;

static unsigned long long state = 0x5EED0C2DULL;
static double uniform() {   // splitmix64 -> [-1, 1)
    unsigned long long z = (state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    z ^= z >> 31;
    return (double)(z >> 11) / 4503599627370496.0 - 1.0;
}

int main() {
    const int shapes[9][2] = {{1, 1}, {2, 1}, {4, 2}, {12, 4}, {16, 16}, {17, 3}, {32, 8}, {33, 3}, {64, 16}};
    const double times[3] = {0.05, 1.0, 5.0};
    int done = 0;
    for (const auto& sh : shapes) {
        const int n = sh[0], m = sh[1];
        for (double Ts : times)
            for (int rep = 0; rep < 3; ++rep) {
                mat A((size_t)n * n), B((size_t)n * m), Ad, Bd;
                const double scale = (1.65 + 1.35 * uniform()) / std::sqrt((double)n), shift = 1.0 + uniform();
                for (double& v : A) v = scale * 1.7 * uniform();
                for (int i = 0; i < n; ++i) A[(size_t)i * n + i] -= shift;
                for (double& v : B) v = 1.7 * uniform();
                if (almpc::hm::c2d(A, B, Ts, n, m, Ad, Bd) != 0) { std::printf("c2d failed at n %d m %d Ts %g\n", n, m, Ts); return 1; }
                if (Ad.size() != A.size() || Bd.size() != B.size()) return 2;
                for (double v : Ad) if (!std::isfinite(v)) return 3;
                for (double v : Bd) if (!std::isfinite(v)) return 3;
                ++done;
            }
    }
    {   // the double integrator: a singular A, every operation exact
        mat A = {0.0, 0.0, 1.0, 0.0}, B = {0.0, 1.0}, Ad, Bd;
        if (almpc::hm::c2d(A, B, 1.0, 2, 1, Ad, Bd) != 0) return 4;
        if (Ad[0] != 1.0 || Ad[1] != 0.0 || Ad[2] != 1.0 || Ad[3] != 1.0 || Bd[0] != 0.5 || Bd[1] != 1.0) return 5;
        // refusals leave the outputs alone: a NaN entry, a norm beyond 2^59, an overflow in the doublings
        mat keepA = {7.0}, keepB = {7.0};
        mat An = A; An[1] = std::numeric_limits<double>::quiet_NaN();
        if (almpc::hm::c2d(An, B, 1.0, 2, 1, keepA, keepB) != 1) return 6;
        mat Ah = A; for (double& v : Ah) v *= 1e300;
        if (almpc::hm::c2d(Ah, B, 1.0, 2, 1, keepA, keepB) != 1) return 7;
        mat Au = {1000.0}, Bu = {1.0};
        if (almpc::hm::c2d(Au, Bu, 1.0, 1, 1, keepA, keepB) != 1) return 8;   // exp(1000) is not a double
        if (keepA.size() != 1 || keepA[0] != 7.0 || keepB.size() != 1 || keepB[0] != 7.0) return 9;
    }
    std::printf("c2d host math ok: %d\n", done);
    return 0;
}
