// ctrl_lookahead_harness.cpp - csrc/hjbdp_ctrl_lookahead.h compiled as plain C++ with the address and undefined-behaviour
// sanitizers (tests/test_control_lookahead_refs.py): the header the K35 / K36 kernels and the host twin include, without HIP, in a
// program of its own.  Runs ctrl_lookahead_rollout_host on ONE fixed case - lookahead_harness.cpp's grid, table, model, planes and
// starts; a per-control set of 3 nodes on axis 1 alone (axis 0 is outside the mask) with label 2's nodes all zero, weights
// (1/4, 1/2, 1/4) in the expect mode and none in the worst mode; the actuator plant flown under given nodes of a 2-node set whose
// input 1 is dead and whose base lies on axis 0 alone - and prints the bits, one line per output, mode and value type:
//   "<f32|f64> <expect|worst> <name> <hex words...>"   name in X_final, cost, X_path, U_path, L_path, V_path
// The test rebuilds the case from the same formulas and holds the lines to tests/control_lookahead_rollout_refs.py.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "hjbdp_ctrl_lookahead.h"

using namespace hjb;

static void line(const char *ty, const char *mode, const char *name, const std::vector<double> &v) {
    printf("%s %s %s", ty, mode, name);
    for (double d : v) {
        uint64_t w;
        std::memcpy(&w, &d, sizeof w);
        printf(" %016llx", (unsigned long long)w);
    }
    printf("\n");
}

template <typename TV>
static void run(const char *ty, int mode) {
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
    // [2, 3, 3] column-major: axis 1 alone; label 0, label 1, label 2 (all zero, one of them -0.0)
    const double offsets[18] = {0.0, -0.3, 0.0, 0.0, -0.0, 0.45, /**/ 0.0, 0.2, 0.0, -0.35, 0.0, 0.05, /**/ 0.0, 0.0, 0.0, -0.0, 0.0, 0.0};
    const double weights[3] = {0.25, 0.5, 0.25};
    CtrlLookSet L{};
    L.mode = mode;
    double scratch[3 * (1 + 2 * 3)];
    const int64_t n_tab = ctrl_look_table(2, 3, 3, offsets, mode == HJB_DIST_EXPECT ? weights : nullptr, L, scratch);
    std::unique_ptr<double[]> tab(new double[n_tab]);         // an allocation of exactly the block: a read past it is the sanitizer's to find
    std::memcpy(tab.get(), scratch, sizeof(double) * n_tab);
    L.tab = tab.get();
    const double eps[4] = {0.5, 0.0, /**/ -0.25, -0.0};       // [n_u = 2, 2 nodes] column-major: input 1 is dead
    const double base[4] = {0.125, 0.0, /**/ -0.0625, -0.0};  // [2, 2 nodes] column-major: axis 0 alone
    CtrlLookPlant plant{};
    ctrl_look_plant(2, 2, 2, eps, base, M.B, plant);
    const int32_t nodes[12] = {0, 1, 1, 0, /**/ 1, 1, 0, 0, /**/ 0, 1, 0, 1};           // [nt, 3], trajectory fastest
    std::vector<double> Xf(2 * nt), cost(nt), Xp(nt * 2 * 4), Up(nt * 2 * 3), Lp(nt * 3), Vp(nt * 3);
    ctrl_lookahead_rollout_host<2, TV>(M, L, knots, rdx, ut, values.data(), 3, planes, nt, X0, nodes, plant, Xf.data(), cost.data(),
                                       Xp.data(), Up.data(), Lp.data(), Vp.data());
    const char *mname = mode == HJB_DIST_EXPECT ? "expect" : "worst";
    line(ty, mname, "X_final", Xf);
    line(ty, mname, "cost", cost);
    line(ty, mname, "X_path", Xp);
    line(ty, mname, "U_path", Up);
    line(ty, mname, "L_path", Lp);
    line(ty, mname, "V_path", Vp);
}

int main() {
    run<float>("f32", HJB_DIST_EXPECT);
    run<float>("f32", HJB_DIST_WORST);
    run<double>("f64", HJB_DIST_EXPECT);
    run<double>("f64", HJB_DIST_WORST);
    return 0;
}
