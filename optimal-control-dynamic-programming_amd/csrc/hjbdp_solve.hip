// hjbdp_solve.hip - hjb_solve (include/hjbdp.h): one handle's backward sweep, the reference's stage loop (pos-att/Solver_pos_att.m:270-286),
// as four steps: the scratch of the per-stage outputs and the probe block, the choice of graph replay / K9, the block loop, the read-back.
// hjbdp_sweep.h states the monitor's rule, its schedule and how a block of stages divides into replays and eager launches.
// gfx950 (MI355X) only; no CPU fallback - without a HIP device every compute entry point returns HJB_E_DEVICE.
#include "hjbdp_host.h"

using namespace hjbhost;

namespace {

struct Solve {
    Handle *h;
    const hjb_solve_opts *o;
    SharedHold &lk;               // the call's shared hold of g_capture_mu (allocation, synchronous copies, device sync): released while
    SweepScratch &sc;             // the sweep only launches on and waits for the handle's own stream
    size_t jb, ib, pb = 0;        // bytes of one plane of J, of labels, of one probe output
    char *dJst = nullptr, *dIst = nullptr, *dPg = nullptr, *dPx = nullptr, *dPj = nullptr;
    DProbe pr{};
    bool every_stage = false, graph_ok = false, tiled = false;
    const void *cur = nullptr;    // the last stage's J and labels
    const char *cur_idx = nullptr;
    int done = 0, early = 0;
    MonitorDiff mon;
    float ms = 0;
};

// Optional per-stage capture (the kernels write straight into the stage planes) and the optional probe block (the reference's debug
// taps): one plane of each requested output per stage.  Zero-filled: planes of stages an early stop never runs come back as zeros.
int stage_scratch(Solve &s) {
    Handle *h = s.h;
    const hjb_solve_opts *o = s.o;
    const int n = o->n_stages;
    int st = HJB_OK;
    if (o->J_stages && (st = s.sc.alloc(s.jb * n, true, &s.dJst, "cannot hold %d J stages on the device", n))) return st;
    if (o->idx_stages && (st = s.sc.alloc(s.ib * n, true, &s.dIst, "cannot hold %d idx stages on the device", n))) return st;
    if (!o->probe) return HJB_OK;
    if ((st = make_probe(h, o->probe, &s.pr))) return st;
    s.pb = (size_t)s.pr.B * (h->dtype == HJB_F64 ? 8 : 4);
    if ((o->probe->g && s.sc.alloc(s.pb * n, true, &s.dPg, "probe buffers")) || (o->probe->x_next && s.sc.alloc(s.pb * h->hp.D * n, true, &s.dPx, "probe buffers")) ||
        (o->probe->j_interp && s.sc.alloc(s.pb * n, true, &s.dPj, "probe buffers")))
        return fail(h, HJB_E_NOMEM, "probe buffers");
    return HJB_OK;
}

// Launch-bound sweeps replay kGraphStages ping-pong launches per hipGraphLaunch; K9 runs several stages per launch for local 2-D
// problems (no per-stage outputs, no monitor read-backs).  The handle's graph exec is captured here when it is wanted and missing;
// the shared hold is released first, and whoever called cleans up after a failure.
int choose_replay(Solve &s) {
    Handle *h = s.h;
    const hjb_solve_opts *o = s.o;
    const bool plain = !s.dJst && !s.dIst && !o->probe && !s.every_stage;
    s.graph_ok = h->use_graph && plain && o->n_stages >= 2 * kGraphStages;
    if (h->use_temporal && !h->cost64 && plain && o->monitor_period <= 0 && o->n_stages >= 2 * kTileK && h->forced_variant < 0 && h->dist_nodes == 0) {
        if (h->tile2d < 0) {
            const int tst = examine_tile2d(h);
            if (tst) return tst;
        }
        s.tiled = h->tile2d == 1;
    }
    if (h->use_temporal == 2 && !s.tiled)
        return fail(h, HJB_E_UNSUPPORTED, "option temporal=2: several stages per launch do not apply (needs D=2, whole grid, "
                    "every query within one cell of its state, no per-stage outputs or monitor, no disturbance, >= %d stages)", 2 * kTileK);
    if (h->gexec && h->gexec_tiled != s.tiled) { (void)hipGraphExecDestroy(h->gexec); h->gexec = nullptr; }
    s.lk.unlock();
    if (!s.graph_ok || h->gexec) return HJB_OK;
    static_assert(kGraphStages % (2 * kTileK) == 0, "a graph must hold an even number of tile launches");
    h->gexec_tiled = s.tiled;
    return capture_stage_loop(h, h->stream, [&]() {      // from dJ[0] back into dJ[0]; tiled: 4 launches of kTileK stages
        int cst = HJB_OK;
        for (int i = 0; i < kGraphStages / (s.tiled ? kTileK : 1) && cst == HJB_OK; ++i)
            cst = s.tiled ? launch_tile2d(h, h->dJ[i & 1], h->dJ[(i + 1) & 1], h->d_idx, kTileK, h->stream)
                          : launch_stage(h, h->dJ[i & 1], h->dJ[(i + 1) & 1], h->d_idx, h->stream);
        return cst;
    }, &h->gexec);
}

// The stage loop on the handle's own stream, in blocks that end at a monitor point (sweep_block); timed by the scratch's events.
int run_blocks(Solve &s) {
    Handle *h = s.h;
    const hjb_solve_opts *o = s.o;
    hipStream_t stream = h->stream;
    HIP_TRY(h, hipEventCreate(&s.sc.ev0));
    HIP_TRY(h, hipEventCreate(&s.sc.ev1));
    HIP_TRY(h, hipEventRecord(s.sc.ev0, stream));
    auto seconds = [&]() {            // since the loop began (waits for the stream)
        float ms = 0;
        (void)hipEventRecord(s.sc.ev1, stream);
        (void)hipEventSynchronize(s.sc.ev1);
        (void)hipEventElapsedTime(&ms, s.sc.ev0, s.sc.ev1);
        return ms * 1e-3;
    };
    s.cur = h->dJ[0];
    s.cur_idx = h->d_idx;
    int pp = 1, st = HJB_OK;          // pp: the next ping-pong target
    for (int k_s = o->n_stages; k_s >= 1;) {
        const SweepBlock b = sweep_block(k_s, o->monitor_period, s.graph_ok, pp ^ 1);
        if (b.eager_first) {          // make dJ[0] the current buffer
            if ((st = launch_stage(h, s.cur, h->dJ[pp], h->d_idx, stream))) return st;
            s.cur = h->dJ[pp]; pp ^= 1; ++s.done; --k_s;
        }
        for (int r = 0; r < b.replays; ++r, s.done += kGraphStages, k_s -= kGraphStages) HIP_TRY(h, hipGraphLaunch(h->gexec, stream));
        int run = b.tail;
        while (s.tiled && run > 0) {                           // K9: up to kTileK stages per launch
            const int K = std::min(run, kTileK);
            if ((st = launch_tile2d(h, s.cur, h->dJ[pp], h->d_idx, K, stream))) return st;
            s.cur = h->dJ[pp];
            s.cur_idx = h->d_idx;
            pp ^= 1;
            s.done += K; run -= K; k_s -= K;
        }
        for (; run > 0; --run, --k_s) {
            void *outJ = s.dJst ? (void *)(s.dJst + (size_t)(k_s - 1) * s.jb) : h->dJ[pp];
            char *outI = s.dIst ? s.dIst + (size_t)(k_s - 1) * s.ib : h->d_idx;
            if (o->probe) {                              // taps of stage k_s: tables at the block, J_{k+1} = cur
                s.pr.g = s.dPg ? s.dPg + (size_t)(k_s - 1) * s.pb : nullptr;
                s.pr.x_next = s.dPx ? s.dPx + (size_t)(k_s - 1) * s.pb * h->hp.D : nullptr;
                s.pr.j_interp = s.dPj ? s.dPj + (size_t)(k_s - 1) * s.pb : nullptr;
                if ((st = launch_probe(h, s.pr, s.cur, stream))) return st;
            }
            if ((st = launch_stage(h, s.cur, outJ, outI, stream))) return st;
            if (s.every_stage && !(o->monitor_period > 0 && k_s == b.stop))      // Dynamic_Solver.m:101: one line per stage
                o->progress(o->progress_user, k_s, 0.0, 0.0, seconds());
            s.cur = outJ;
            s.cur_idx = outI;
            if (!s.dJst) pp ^= 1;
            ++s.done;
        }
        // here k_s == b.stop - 1; the stage just computed has reference index b.stop
        if (monitor_due(b.stop, o->monitor_period)) {
            const bool single = o->monitor_single != 0 || h->monitor_single;
            if (launch_monitor_sums(h->dtype, single, s.cur, s.cur_idx, h->idx_bytes, h->n_owned, h->d_partials, h->d_sums, stream) != HJB_OK)
                return fail(h, HJB_E_DEVICE, "monitor reduction launch failed");
            double sums[2];
            s.lk.lock();
            HIP_TRY(h, hipMemcpyAsync(sums, h->d_sums, sizeof sums, hipMemcpyDeviceToHost, stream));
            HIP_TRY(h, hipStreamSynchronize(stream));
            s.lk.unlock();
            const bool stop = s.mon.step(sums[0], sums[1], single && h->dtype != HJB_F64, o->monitor_tol);
            if (o->progress) o->progress(o->progress_user, b.stop, s.mon.e, s.mon.e2, seconds());
            if (stop) { s.early = 1; break; }
        }
    }
    HIP_TRY(h, hipEventRecord(s.sc.ev1, stream));
    HIP_TRY(h, hipEventSynchronize(s.sc.ev1));
    HIP_TRY(h, hipEventElapsedTime(&s.ms, s.sc.ev0, s.sc.ev1));
    return HJB_OK;
}

int read_back(Solve &s) {
    Handle *h = s.h;
    const hjb_solve_opts *o = s.o;
    const size_t n = (size_t)o->n_stages;
    s.lk.lock();
    const int st = check_status(h, h->stream);
    if (st) return st;
    if (o->J_final) HIP_TRY(h, hipMemcpy(o->J_final, s.cur, s.jb, hipMemcpyDeviceToHost));
    if (o->idx_final) HIP_TRY(h, hipMemcpy(o->idx_final, s.cur_idx, s.ib, hipMemcpyDeviceToHost));
    if (s.dPg) HIP_TRY(h, hipMemcpy(o->probe->g, s.dPg, s.pb * n, hipMemcpyDeviceToHost));
    if (s.dPx) HIP_TRY(h, hipMemcpy(o->probe->x_next, s.dPx, s.pb * h->hp.D * n, hipMemcpyDeviceToHost));
    if (s.dPj) HIP_TRY(h, hipMemcpy(o->probe->j_interp, s.dPj, s.pb * n, hipMemcpyDeviceToHost));
    if (o->J_stages) HIP_TRY(h, hipMemcpy(o->J_stages, s.dJst, s.jb * n, hipMemcpyDeviceToHost));
    if (o->idx_stages) HIP_TRY(h, hipMemcpy(o->idx_stages, s.dIst, s.ib * n, hipMemcpyDeviceToHost));
    return HJB_OK;
}

}  // namespace

extern "C" int32_t hjb_solve(hjb_handle hh, const hjb_solve_opts *o, hjb_result *res) {
    Handle *h = (Handle *)hh;
    if (!h || !o) return fail(h, HJB_E_INVALID, "null argument");
    if (o->n_stages < 1) return fail(h, HJB_E_INVALID, "n_stages=%d", o->n_stages);
    if (h->j_elems != h->n_owned)
        return fail(h, HJB_E_UNSUPPORTED, "hjb_solve runs whole grids; drive slabs with hjb_backup_stage_device + a halo exchange");
    if (o->probe && h->dist_nodes > 0)
        return fail(h, HJB_E_UNSUPPORTED, "the probe block taps the nominal next state: not available while a disturbance is set (hjb_set_disturbance)");
    HIP_TRY(h, hipSetDevice(h->device));
    SharedHold lk(g_capture_mu);
    int st = ensure_work(h);
    if (st) return st;
    if (!h->stream) HIP_TRY(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    SweepScratch sc(h, lk);
    Solve s{h, o, lk, sc, (size_t)h->n_owned * h->esz, (size_t)h->n_owned * h->idx_bytes};
    s.every_stage = o->progress && o->progress_every_stage;
    if ((st = stage_scratch(s))) return st;
    if (o->terminal) HIP_TRY(h, hipMemcpy(h->dJ[0], o->terminal, s.jb, hipMemcpyHostToDevice));
    else HIP_TRY(h, hipMemset(h->dJ[0], 0, s.jb));
    HIP_TRY(h, sync_setup());            // the sweep runs on the handle's own stream from here (other handles' sweeps are not waited for)
    if ((st = choose_replay(s)) || (st = run_blocks(s)) || (st = read_back(s))) return st;
    if (res) *res = hjb_result{s.done, s.early, s.ms, s.mon.e, s.mon.e2};
    return HJB_OK;
}
