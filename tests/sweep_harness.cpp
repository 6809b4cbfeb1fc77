// sweep_harness.cpp - host check of what the backward-sweep drivers decide without a device (csrc/hjbdp_sweep.h), compiled as plain
// C++ by tests/test_sweep_arithmetic.py.  The schedule: every n_stages in 1 .. 200, every monitor period in 0 .. n_stages + 1, graph
// replay on and off, walked block by block from the first stage to k_s == 0.  The monitor's rule: a fixed list of sums against a
// literal transcription of the reference's two branches.  Prints one line and returns the number of checks that failed.
//   sweep_harness             the library's own rules
//   sweep_harness --mutants   the same checks on deliberately wrong copies: every one of them must be REJECTED (the line says so)
#include <cmath>
#include <cstdio>
#include <cstring>

#include "hjbdp_sweep.h"

using namespace hjb;

struct Rules {
    SweepBlock (*block)(int, int, bool, int);
    bool (*step)(MonitorDiff &, double, double, bool, double);
};

static char g_where[256];
static const char *at(const char *what, int n_stages, int period, int graph, int k_s) {
    snprintf(g_where, sizeof g_where, "%s (n_stages = %d, period = %d, graph = %d, k_s = %d)", what, n_stages, period, graph, k_s);
    return g_where;
}

// -> nullptr: every walk holds; else the first violation
static const char *check_schedule(const Rules &R) {
    for (int n = 1; n <= 200; ++n)
        for (int period = 0; period <= n + 1; ++period)
            for (int graph = 0; graph <= 1; ++graph) {
                int k_s = n, parity = 0, blocks = 0;
                int due = period > 0 ? (n / period) * period : 0;      // the next monitor point the walk must visit (0: none left)
                while (k_s >= 1) {
                    const SweepBlock b = R.block(k_s, period, graph != 0, parity);
                    ++blocks;
                    if (b.stop < 1 || b.stop > k_s) return at("a block's last stage is outside [1, k_s]", n, period, graph, k_s);
                    if (b.eager_first < 0 || b.eager_first > 1 || b.replays < 0 || b.tail < 0) return at("a negative count, or more than one eager-first stage", n, period, graph, k_s);
                    const int run = k_s - b.stop + 1;
                    if (b.eager_first + b.replays * kGraphStages + b.tail != run) return at("the launches do not add up to the block's stages", n, period, graph, k_s);
                    const bool replaying = graph && run >= kGraphStages;       // the drivers' condition for leaving the eager loop
                    if (!replaying && (b.eager_first || b.replays)) return at("a replay or an eager-first stage in a block that is not replayed", n, period, graph, k_s);
                    if (replaying && b.tail >= kGraphStages) return at("a tail that a replay would have covered", n, period, graph, k_s);
                    parity ^= b.eager_first;
                    if (b.replays && parity != 0) return at("a replay starts outside buffer 0", n, period, graph, k_s);
                    parity ^= b.tail & 1;
                    if (monitor_due(b.stop, period)) {
                        if (b.stop != due) return at("a monitor point that is not the next multiple of the period", n, period, graph, k_s);
                        due -= period;
                    }
                    k_s = b.stop - 1;
                }
                if (due != 0) return at("a multiple of the period was not visited", n, period, graph, 0);
                if (period == 0 && blocks != 1) return at("more than one block without a monitor", n, period, graph, 0);
                if (parity != (n & 1)) return at("the parity after the walk is not n_stages & 1", n, period, graph, 0);
            }
    return nullptr;
}

// ---- the monitor's rule: pos-att/Solver_pos_att.m:276-282, transcribed once per class of fsum50 --------------------------------------
//   e = fsum50 - fsum50_prev;  e2 = idsum50 - idsum50_prev;  fsum50_prev = fsum50;  idsum50_prev = idsum50;  if (abs(e) < tol) break
// single fsum50 (F_gI.Values single): the subtraction is single, and in abs(e) < tol MATLAB casts the double tol to single
struct RefSingle {
    float fsum50_prev = 0;
    double idsum50_prev = 0, e = 0, e2 = 0;
    bool step(double sumJ, double sumI, double tol) {
        const float fsum50 = (float)sumJ;
        const float es = fsum50 - fsum50_prev;
        e = (double)es;
        e2 = sumI - idsum50_prev;
        fsum50_prev = fsum50;
        idsum50_prev = sumI;
        return fabsf(es) < (float)tol;
    }
};
// double fsum50: everything is double
struct RefDouble {
    double fsum50_prev = 0, idsum50_prev = 0, e = 0, e2 = 0;
    bool step(double sumJ, double sumI, double tol) {
        e = sumJ - fsum50_prev;
        e2 = sumI - idsum50_prev;
        fsum50_prev = sumJ;
        idsum50_prev = sumI;
        return fabs(e) < tol;
    }
};

struct Series { double tol; int n; double sumJ[4], sumI[4]; };
static const Series kSeries[] = {
    // a first call (fprev = 0), then an ordinary descent to a stop
    {1e-2, 4, {5.0, 4.0, 3.9999, 3.9999}, {700.0, 650.0, 650.0, 649.0}},
    // the double difference is below tol, the single one is not: 2^24 + 1 rounds to 2^24, 2^24 + 1.009 to 2^24 + 2
    {1e-2, 2, {16777217.0, 16777217.009}, {10.0, 10.0}},
    // the reverse: 0.5 in double, 0 in single (2^24 + 0.5 rounds to 2^24)
    {1e-2, 2, {16777216.0, 16777216.5}, {3.0, 4.0}},
    // tol = 0.01 rounds DOWN in float: e = (float)0.01 is below the double tol and not below the single one
    {1e-2, 1, {(double)0.01f}, {0.0}},
    {1e-2, 2, {1.0, 1.0 - (double)0.01f}, {1.0, 1.0}},
    // tol = 0.1 rounds UP in float: e equal to the tolerance of its class stops neither, the float below it stops both
    {0.1, 1, {0.1}, {0.0}},
    {0.1, 1, {(double)nextafterf(0.1f, 0.0f)}, {0.0}},
    // negative differences, a zero tolerance (never stops), a zero difference under a positive one
    {0.0, 3, {2.0, 2.0, 1.0}, {5.0, 5.0, 5.0}},
    {1e-6, 3, {-3.0, -3.0000001, -3.0000001}, {9.0, 8.0, 8.0}},
};

static const char *check_monitor(const Rules &R) {
    for (const Series &s : kSeries)
        for (int single = 0; single <= 1; ++single) {
            MonitorDiff m;
            RefSingle rs;
            RefDouble rd;
            for (int i = 0; i < s.n; ++i) {
                const bool got = R.step(m, s.sumJ[i], s.sumI[i], single != 0, s.tol);
                const bool want = single ? rs.step(s.sumJ[i], s.sumI[i], s.tol) : rd.step(s.sumJ[i], s.sumI[i], s.tol);
                const double we = single ? rs.e : rd.e, we2 = single ? rs.e2 : rd.e2;
                if (got != want || m.e != we || m.e2 != we2) {
                    snprintf(g_where, sizeof g_where, "the monitor's rule (series %d, call %d, %s): stop %d e %.17g e2 %.17g, the reference's %d %.17g %.17g",
                             (int)(&s - kSeries), i, single ? "single" : "double", (int)got, m.e, m.e2, (int)want, we, we2);
                    return g_where;
                }
            }
        }
    return nullptr;
}

static const char *check(const Rules &R) {
    const char *why = check_schedule(R);
    return why ? why : check_monitor(R);
}

static bool lib_step(MonitorDiff &m, double sumJ, double sumI, bool single, double tol) { return m.step(sumJ, sumI, single, tol); }

// ---- the wrong copies ----------------------------------------------------------------------------------------------------------------
static bool step_compares_in_double(MonitorDiff &m, double sumJ, double sumI, bool single, double tol) {      // under `single` too
    m.step(sumJ, sumI, single, tol);
    return std::fabs(m.e) < tol;
}
// sweep_block restated with one rule wrong: 1 `stop` without the max(1, ...), 2 the eager-first stage at parity 0 instead of 1,
// 3 a tail of run % kGraphStages taken before the eager-first stage (which then comes out of a replay)
template <int WRONG>
static SweepBlock wrong_block(int k_s, int period, bool graph, int parity) {
    SweepBlock b{1, 0, 0, 0};
    if (period > 0) b.stop = (k_s / period) * period;
    if (WRONG != 1 && b.stop < 1) b.stop = 1;
    int run = k_s - b.stop + 1;
    if (graph && run >= kGraphStages) {
        if (WRONG == 3) { b.tail = run % kGraphStages; run -= b.tail; }
        b.eager_first = WRONG == 2 ? parity == 0 : parity != 0;
        b.replays = (run - b.eager_first) / kGraphStages;
        if (WRONG != 3) b.tail = run - b.eager_first - b.replays * kGraphStages;
    } else b.tail = run;
    return b;
}

int main(int argc, char **argv) {
    const Rules lib = {sweep_block, lib_step};
    if (argc > 1 && !strcmp(argv[1], "--mutants")) {
        int failed = 0;
        Rules m[4] = {lib, lib, lib, lib};
        const char *names[4] = {"single_compares_in_double", "stop_without_max", "eager_first_at_parity_0", "tail_before_eager_first"};
        m[0].step = step_compares_in_double;
        m[1].block = wrong_block<1>;
        m[2].block = wrong_block<2>;
        m[3].block = wrong_block<3>;
        for (int i = 0; i < 4; ++i) {
            const char *why = check(m[i]);
            printf("%s: %s\n", names[i], why ? "REJECTED" : "accepted");
            if (why) printf("  %s\n", why);
            failed += why ? 0 : 1;
        }
        return failed;
    }
    const char *why = check(lib);
    printf("sweep arithmetic: %s\n", why ? "FAILED" : "ok");
    if (why) printf("  %s\n", why);
    return why ? 1 : 0;
}
