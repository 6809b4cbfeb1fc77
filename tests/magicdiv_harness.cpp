// magicdiv_harness.cpp - host check of the division by a launch-invariant divisor (csrc/hjbdp_walk.h: magic_div, magic_quot) that
// the evaluation kernel's 32-bit form takes a state index and a label apart with; compiled as plain C++ by
// tests/test_evaluate_abi.py.  Prints one line and returns the number of (n, d) pairs whose quotient is wrong.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "hjbdp_walk.h"

int main() {
    std::vector<uint32_t> ds;
    for (uint32_t d = 1; d <= 5000; ++d) ds.push_back(d);                       // every axis size a test or a reference grid has
    for (int k = 12; k <= 31; ++k)
        for (int64_t e = -2; e <= 2; ++e) ds.push_back((uint32_t)(((int64_t)1 << k) + e));
    ds.push_back(0x7fffffffu);
    ds.push_back(0xffffffffu);
    ds.push_back(1000003u);
    ds.push_back(207360000u);
    uint64_t seed = 0x9e3779b97f4a7c15ull;
    long long bad = 0, checked = 0;
    for (uint32_t d : ds) {
        const hjb::MagicDiv k = hjb::magic_div(d);
        std::vector<uint32_t> ns = {0u, 1u, d - 1, d, d + 1, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
        for (uint64_t q = 1; q * d <= 0xffffffffull && ns.size() < 200; q = q * 3 + 1) {   // around multiples of d: where a quotient steps
            ns.push_back((uint32_t)(q * d - 1));
            ns.push_back((uint32_t)(q * d));
            if (q * d + 1 <= 0xffffffffull) ns.push_back((uint32_t)(q * d + 1));
        }
        const uint32_t top = (uint32_t)(0xffffffffull / d * d);                    // the largest multiple of d
        ns.push_back(top);
        ns.push_back(top - 1);
        for (int i = 0; i < 300; ++i) {
            seed = seed * 6364136223846793005ull + 1442695040888963407ull;
            ns.push_back((uint32_t)(seed >> 32));
        }
        for (uint32_t n : ns) {
            ++checked;
            if (hjb::magic_quot(n, k) != n / d) {
                if (bad < 5) std::printf("WRONG: %u / %u = %u, got %u\n", n, d, n / d, hjb::magic_quot(n, k));
                ++bad;
            }
        }
    }
    std::printf("magic division: %lld pairs checked, %lld wrong\n", checked, bad);
    return bad ? 1 : 0;
}
