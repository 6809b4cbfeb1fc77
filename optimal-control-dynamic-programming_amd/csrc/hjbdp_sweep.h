// hjbdp_sweep.h - what the backward-sweep drivers (hjb_solve, hjb_solve_batch, hjb_solve_multi, hjb_rank_sweep) decide without a
// device: the early-stop monitor's rule, its schedule, and how a block of stages divides into graph replays and eager launches.
// The one statement of each.  No HIP dependency: tests/sweep_harness.cpp compiles it as plain C++ and walks every schedule.
#pragma once
#include <cmath>

namespace hjb {

constexpr int kGraphStages = 32;   // stages per graph replay; even: a replay starts and ends in buffer 0

// The early-stop monitor (Solver_pos_att.m:273-285): fsum50 = sum(F.Values(:)), idsum50 = sum(U_Optimal_id(:)), e and e2 their
// differences from the previous monitor point (0 before the first).  :276-282: with a single fsum50, `e = fsum50 - fsum50_prev`
// is a single-precision subtraction and `abs(e) < tol` compares in single (MATLAB casts the double tol); otherwise all is double.
struct MonitorDiff {
    double fprev = 0, iprev = 0, e = 0, e2 = 0;
    bool step(double sumJ, double sumI, bool single, double tol) {      // -> the sweep stops here
        e = single ? (double)((float)sumJ - (float)fprev) : sumJ - fprev;
        e2 = sumI - iprev;
        fprev = sumJ;
        iprev = sumI;
        return single ? std::fabs((float)e) < (float)tol : std::fabs(e) < tol;
    }
};

// the stage with reference index `stage` (n_stages down to 1) is a monitor point
inline bool monitor_due(int stage, int period) { return period > 0 && stage % period == 0; }

// The stages from k_s down to and including `stop`, the next monitor point (1 without one), in launch order: eager_first (0 or 1)
// stage that brings the sweep back to buffer 0, `replays` graph replays of kGraphStages stages each, `tail` eager stages.
// graph: the driver replays at all; parity: the buffer that holds the current cost-to-go.
struct SweepBlock { int stop, eager_first, replays, tail; };
inline SweepBlock sweep_block(int k_s, int period, bool graph, int parity) {
    SweepBlock b{1, 0, 0, 0};
    if (period > 0 && k_s / period >= 1) b.stop = (k_s / period) * period;
    int run = k_s - b.stop + 1;
    if (graph && run >= kGraphStages) {
        b.eager_first = parity != 0;
        b.replays = (run - b.eager_first) / kGraphStages;
    }
    b.tail = run - b.eager_first - b.replays * kGraphStages;
    return b;
}

}  // namespace hjb
