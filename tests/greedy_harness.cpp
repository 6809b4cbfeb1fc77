// greedy_harness.cpp - csrc/hjbdp_greedy.h compiled as plain C++ (tests/test_rollout_greedy_abi.py): the header the K26 kernel and
// the host twin include, without HIP.  Runs greedy_rollout_host on ONE fixed case - D = 2, a non-uniform and a uniform axis,
// 3 labels of 2 controls with the last row a duplicate of the first, float and double planes, the planes (1, 0, -1), four starts
// (inside, on a node, on the last node, outside) - and prints the bits, one line per output and value type:
//   "<f32|f64> <name> <hex words...>"   name in X_final, cost, X_path, U_path, L_path, V_path
// The test rebuilds the case from the same formulas and holds the lines to tests/greedy_rollout_refs.py.
#include <cstdio>
#include <cstring>
#include <vector>

#include "hjbdp_greedy.h"

using namespace hjb;

static void line(const char *ty, const char *name, const std::vector<double> &v) {
    printf("%s %s", ty, name);
    for (double d : v) {
        uint64_t w;
        std::memcpy(&w, &d, sizeof w);
        printf(" %016llx", (unsigned long long)w);
    }
    printf("\n");
}

template <typename TV>
static void run(const char *ty) {
    const int32_t n[2] = {4, 3};
    const double knots[7] = {-1.0, -0.25, 0.5, 1.0, -1.0, 0.0, 1.0};
    const double ut[6] = {0.5, -0.75, 0.5, /* control 1 */ -0.125, 0.25, -0.125};     // [3, 2] column-major; row 2 == row 0
    GreedyModel M{};
    double rdx[7];
    greedy_grid(2, n, knots, M, rdx);
    M.n_u = 2;
    M.n_labels = 3;
    M.has_c = 1;
    const double A[4] = {0.875, -0.125, 0.25, 0.75}, B[4] = {0.5, 0.125, -0.25, 0.375};   // column-major
    std::memcpy(M.A, A, sizeof A);
    std::memcpy(M.B, B, sizeof B);
    M.c[0] = 0.0625;
    M.c[1] = -0.03125;
    M.q[0] = 0.75;
    M.q[1] = 0.3;
    M.r[0] = 0.1;
    M.r[1] = 0.7;
    std::vector<TV> values(24);
    for (int i = 0; i < 24; ++i) values[i] = (TV)(((i * 37 + 11) % 17) / 16.0 + (i % 3) * 0.1);
    const int32_t planes[3] = {1, 0, -1};
    const double X0[8] = {0.3, -0.4, /**/ -0.25, 0.0, /**/ 1.0, 1.0, /**/ 1.15, -1.2};
    const int64_t nt = 4;
    std::vector<double> Xf(2 * nt), cost(nt), Xp(nt * 2 * 4), Up(nt * 2 * 3), Lp(nt * 3), Vp(nt * 3);
    greedy_rollout_host<2, TV>(M, knots, rdx, ut, values.data(), 3, planes, nt, X0, Xf.data(), cost.data(), Xp.data(), Up.data(),
                               Lp.data(), Vp.data());
    line(ty, "X_final", Xf);
    line(ty, "cost", cost);
    line(ty, "X_path", Xp);
    line(ty, "U_path", Up);
    line(ty, "L_path", Lp);
    line(ty, "V_path", Vp);
}

int main() {
    run<float>("f32");
    run<double>("f64");
    return 0;
}
