// hjbdp_batch.hip - hjb_solve_batch: several independent sweeps of ONE kernel shape side by side, ONE launch per stage for all of them
// (the column-sweep kernel, kernels_colsweep.h, or the table kernel's 32-bit form, kernels_tabled.h).
// gfx950 (MI355X) only; no CPU fallback - without a HIP device every compute entry point returns HJB_E_DEVICE.
//
// Solver_pos_att.simplified_run (pos-att/Solver_pos_att.m:197-242) sweeps four independent channels - x, y, z and the thruster-failure
// variant of x - of 2.7e5 states each.  A stage kernel of one channel is a launch boundary plus one wave's chain of round trips
// (~10 - 14 us whatever the grid), and of four such chains on four streams the device runs two at full rate (profiles/r05_pos_att_run.log):
// the four sweeps took two rounds.  Here the channels are the y dimension of one launch of the column-sweep kernel (kernels_colsweep.h:
// k_backup_colsweep_batch), the stage loop is one chain, the early-stop monitor (:268-285) keeps its own sums, difference and stop
// decision per channel, and a stopped channel drops out of the launches that follow.  Results per channel are those of hjb_solve, bit
// for bit (the same kernel body on the same buffers).
#include "hjbdp_host.h"

using namespace hjbhost;

extern "C" {

int32_t hjb_solve_batch(int32_t n, const hjb_handle *hs, const hjb_solve_opts *const *opts, hjb_result *const *res) {
    if (n < 1 || !hs || !opts) return fail(nullptr, HJB_E_INVALID, "hjb_solve_batch: bad argument");
    if (n > kCsBatchMax) return fail(nullptr, HJB_E_UNSUPPORTED, "hjb_solve_batch: at most %d problems", kCsBatchMax);
    Handle *H[kCsBatchMax];
    for (int i = 0; i < n; ++i) {
        H[i] = (Handle *)hs[i];
        if (!H[i] || !opts[i]) return fail(nullptr, HJB_E_INVALID, "hjb_solve_batch: problem %d is null", i);
    }
    // ---- what can run as one launch: one kernel shape and one loop --------------------------------------------------------------------
    //   the column-sweep kernel (variant 7) in its usual form, one group axis and cost typing: Solver_pos_att's channels;
    //   the table kernel (variant 5) in its 32-bit form, one (dtype, D <= 4): Solver_attitude.simplified_run's channels, Solver_pos_att's
    //   channels in the reference's own axis order
    const hjb_solve_opts &o0 = *opts[0];
    if (o0.n_stages < 1) return fail(H[0], HJB_E_INVALID, "n_stages=%d", o0.n_stages);
    const bool tabled = H[0]->L.variant == 5;
    int ng = 0;
    for (int i = 0; i < n; ++i) {
        Handle *h = H[i];
        const hjb_solve_opts &o = *opts[i];
        const Launch &L = h->L;
        if (h->dist_nodes > 0)
            return fail(h, HJB_E_UNSUPPORTED, "hjb_solve_batch: problem %d has a disturbance set (kernel variant 8 is not batched); sweep it with hjb_solve", i);
        if (tabled) {
            if (L.variant != 5 || !L.idx32 || h->j_elems != h->n_owned || h->hp.D > 4)
                return fail(h, HJB_E_UNSUPPORTED, "hjb_solve_batch: problem %d does not run on the table kernel's 32-bit form (variant %d); "
                            "sweep the problems side by side with hjb_solve on threads of their own", i, L.variant);
            if (h->device != H[0]->device || h->dtype != H[0]->dtype || h->hp.D != H[0]->hp.D || L.block != H[0]->L.block)
                return fail(h, HJB_E_UNSUPPORTED, "hjb_solve_batch: problem %d has another device, dtype, dimension or block size than problem 0", i);
        } else {
            if (L.variant != 7 || h->dtype != HJB_F32 || h->j_elems != h->n_owned || !L.dpp || L.cost_form == 0 || L.coop_grid > 0)
                return fail(h, HJB_E_UNSUPPORTED, "hjb_solve_batch: problem %d does not run on the column-sweep kernel in its usual form (variant %d); "
                            "sweep the problems side by side with hjb_solve on threads of their own", i, L.variant);
            if (h->device != H[0]->device || h->hcs.gax != H[0]->hcs.gax || h->cost64 != H[0]->cost64)
                return fail(h, HJB_E_UNSUPPORTED, "hjb_solve_batch: problem %d has another device, group axis or cost typing than problem 0", i);
            ng = std::max(ng, (int)h->hcs.ng);
        }
        if (o.n_stages != o0.n_stages || o.monitor_period != o0.monitor_period)
            return fail(h, HJB_E_UNSUPPORTED, "hjb_solve_batch: one stage count and one monitor period for all problems");
        if (o.J_stages || o.idx_stages || o.probe || (o.progress && o.progress_every_stage))
            return fail(h, HJB_E_UNSUPPORTED, "hjb_solve_batch: no per-stage outputs, probe or per-stage progress (use hjb_solve)");
    }
    Handle *h0 = H[0];
    HIP_TRY(h0, hipSetDevice(h0->device));
    SharedHold unsafe_lk(g_capture_mu);
    for (int i = 0; i < n; ++i) {
        const int st = ensure_work(H[i]);
        if (st) return st;
    }
    struct Resplit {                          // every handle gets its own parts back, on every way out (declared before the call's
        const SharedHold &held;               // scratch: it runs after the frees), with nothing of this batch in flight
        Handle **H;
        int n, old_split[kCsBatchMax];
        ~Resplit() {
            HoldUnlessHeld hold(held);
            if (H[0]->stream) (void)hipStreamSynchronize(H[0]->stream);
            for (int i = 0; i < n; ++i) {
                Handle *h = H[i];
                if (h->cs_split == old_split[i]) continue;
                h->cs_split = old_split[i];
                (void)colsweep_options(h, false);
                choose_launch(h);
            }
        }
    } resplit{unsafe_lk, H, n, {}};
    for (int i = 0; i < n; ++i) resplit.old_split[i] = H[i]->cs_split;
    // Parts per column.  A handle's own choice (colsweep_split) is made for a launch that is ALONE on the device: as many parts as
    // fill the wave slots, because such a launch is one wave's chain of round trips.  Every part primes its rows again, so that
    // choice does up to twice the work per column - the right price for latency, the wrong one for a batch, whose launches hold n
    // problems' columns: here the parts are what lets ALL the batch's columns fill about one round of the wave slots
    // (profiles/r06_batch_split.log: the reference's channels, 4 x 450 columns of 20 steps, 10 parts each when alone - 2 to 4 here).
    if (!tabled) {
        int64_t columns = 0;
        for (int i = 0; i < n; ++i) {
            const DParams &P = H[i]->hp;
            columns += (int64_t)((P.n[0] + kCsDppLanes - 1) / kCsDppLanes) * P.n[2] * P.n[3];
        }
        const int64_t slots = (int64_t)(h0->cost64 ? 5 : 6) * 4 * 256;                   // waves per SIMD of the form that runs (82 / 80 registers) x SIMDs
        const int s_batch = (int)std::max<int64_t>(1, slots / std::max<int64_t>(columns, 1));
        for (int i = 0; i < n; ++i) {
            Handle *h = H[i];
            if (h->cs_split == 0 && s_batch < (int)h->hcs.split) {      // (an explicit option "cs_split" stands)
                h->cs_split = s_batch;
                const int ust = colsweep_options(h, false);
                if (ust) return ust;
                choose_launch(h);
            }
        }
    }
    if (!h0->stream) HIP_TRY(h0, hipStreamCreateWithFlags(&h0->stream, hipStreamNonBlocking));
    hipStream_t stream = h0->stream;
    DCsBatch hb;
    memset(&hb, 0, sizeof hb);
    unsigned gmax = 1;
    for (int i = 0; i < n; ++i) {
        Handle *h = H[i];
        hb.P[i] = h->dp; hb.TB[i] = h->dtb; hb.CS[i] = h->dcs;
        hb.J[i][0] = h->dJ[0]; hb.J[i][1] = h->dJ[1];
        hb.idx[i] = h->d_idx;
        hb.grid[i] = (uint32_t)h->L.grid;
        gmax = std::max(gmax, (unsigned)h->L.grid);
        const size_t jb = (size_t)h->n_owned * h->esz;
        const hipError_t te = opts[i]->terminal ? hipMemcpy(h->dJ[0], opts[i]->terminal, jb, hipMemcpyHostToDevice) : hipMemset(h->dJ[0], 0, jb);
        if (te != hipSuccess) return fail(h, HJB_E_DEVICE, "terminal cost of problem %d: %s", i, hipGetErrorString(te));
    }
    SweepScratch sc(h0, unsafe_lk);
    DCsBatch *dB = nullptr;
    if (sc.alloc(sizeof hb, false, &dB, "batch record")) return fail(h0, HJB_E_DEVICE, "hipMalloc of the batch record failed");
    HIP_TRY(h0, hipMemcpy(dB, &hb, sizeof hb, hipMemcpyHostToDevice));
    HIP_TRY(h0, sync_setup());
    StageArgs a;
    a.grid = gmax;
    a.block = tabled ? (unsigned)h0->L.block : 256u;
    a.st = stream;
    a.dtype = tabled ? h0->dtype : HJB_F32;
    a.D = h0->hp.D;
    const int gax = h0->hcs.gax;
    const bool c64 = h0->cost64;
    auto launch = [&](uint32_t mask, int parity) -> int {
        if (tabled) {
            if (stage_tabled_batch(a, n, hb, mask, parity)) return fail(h0, HJB_E_DEVICE, "hjb_solve_batch: no batched instantiation (D = %d)", a.D);
            return HJB_OK;
        }
        if (stage_colsweep_batch(a, n, dB, mask, parity, gax, ng, c64)) return fail(h0, HJB_E_DEVICE, "hjb_solve_batch: no batched instantiation (%d groups)", ng);
        return HJB_OK;
    };
    uint32_t mask = n >= 32 ? 0xffffffffu : ((1u << n) - 1u), gmask = 0;
    const bool want_graph = h0->use_graph && o0.n_stages >= 2 * kGraphStages;
    unsafe_lk.unlock();
    // kGraphStages ping-pong launches for the problems of `mask`, starting and ending in buffer 0; re-captured when a problem stops
    auto capture = [&]() -> int {
        sc.drop_graph();
        const int cst = capture_stage_loop(h0, stream, [&]() {
            int lst = HJB_OK;
            for (int i = 0; i < kGraphStages && lst == HJB_OK; ++i) lst = launch(mask, i & 1);
            return lst;
        }, &sc.gexec);
        if (!cst) gmask = mask;
        return cst;
    };
    HIP_TRY(h0, hipEventCreate(&sc.ev0));
    HIP_TRY(h0, hipEventCreate(&sc.ev1));
    HIP_TRY(h0, hipEventRecord(sc.ev0, stream));
    int parity = 0;                         // the buffer that holds the current cost-to-go of every problem still running
    int done[kCsBatchMax] = {0}, early[kCsBatchMax] = {0}, final_parity[kCsBatchMax] = {0};
    MonitorDiff mon[kCsBatchMax];
    int st = HJB_OK;
    int k_s = o0.n_stages;
    auto count = [&](int stages) { for (int i = 0; i < n; ++i) if ((mask >> i) & 1u) done[i] += stages; };
    auto eager = [&](int stages) -> int {
        for (; stages > 0; --stages, --k_s, parity ^= 1, count(1))
            if (const int lst = launch(mask, parity)) return lst;
        return HJB_OK;
    };
    while (k_s >= 1 && mask) {
        const SweepBlock b = sweep_block(k_s, o0.monitor_period, want_graph, parity);
        if ((st = eager(b.eager_first))) return st;                      // a replay starts in buffer 0
        if (b.replays && (!sc.gexec || gmask != mask) && (st = capture())) return st;
        for (int g = 0; g < b.replays; ++g, count(kGraphStages), k_s -= kGraphStages) HIP_TRY(h0, hipGraphLaunch(sc.gexec, stream));
        if ((st = eager(b.tail))) return st;
        // here k_s == b.stop - 1: the stage just computed has reference index b.stop (Solver_pos_att.m:273-285, per problem)
        if (monitor_due(b.stop, o0.monitor_period)) {
            double sums[kCsBatchMax][2];
            for (int i = 0; i < n; ++i) {
                if (!((mask >> i) & 1u)) continue;
                Handle *h = H[i];
                if (launch_monitor_sums(h->dtype, opts[i]->monitor_single != 0 || h->monitor_single, h->dJ[parity], h->d_idx, h->idx_bytes, h->n_owned,
                                        h->d_partials, h->d_sums, stream) != HJB_OK) return fail(h, HJB_E_DEVICE, "monitor reduction launch failed");
            }
            unsafe_lk.lock();
            for (int i = 0; i < n; ++i)
                if ((mask >> i) & 1u) HIP_TRY(h0, hipMemcpyAsync(sums[i], H[i]->d_sums, 2 * sizeof(double), hipMemcpyDeviceToHost, stream));
            HIP_TRY(h0, hipStreamSynchronize(stream));
            float ms = 0;
            bool timed = false;
            unsafe_lk.unlock();
            for (int i = 0; i < n; ++i) {
                if (!((mask >> i) & 1u)) continue;
                const hjb_solve_opts &o = *opts[i];
                const bool stops = mon[i].step(sums[i][0], sums[i][1], (o.monitor_single != 0 || H[i]->monitor_single) && H[i]->dtype != HJB_F64, o.monitor_tol);
                if (o.progress) {
                    if (!timed) {
                        (void)hipEventRecord(sc.ev1, stream);
                        (void)hipEventSynchronize(sc.ev1);
                        (void)hipEventElapsedTime(&ms, sc.ev0, sc.ev1);
                        timed = true;
                    }
                    o.progress(o.progress_user, b.stop, mon[i].e, mon[i].e2, ms * 1e-3);
                }
                if (stops) {
                    early[i] = 1;
                    final_parity[i] = parity;
                    mask &= ~(1u << i);           // this problem's sweep ends here: its result stays in the buffer it was just written to
                }
            }
        }
    }
    for (int i = 0; i < n; ++i)
        if (!early[i]) final_parity[i] = parity;
    HIP_TRY(h0, hipEventRecord(sc.ev1, stream));
    HIP_TRY(h0, hipEventSynchronize(sc.ev1));
    float ms = 0;
    HIP_TRY(h0, hipEventElapsedTime(&ms, sc.ev0, sc.ev1));
    unsafe_lk.lock();
    for (int i = 0; i < n; ++i) {
        Handle *h = H[i];
        if ((st = check_status(h, stream))) return st;
        const size_t jb = (size_t)h->n_owned * h->esz, ib = (size_t)h->n_owned * h->idx_bytes;
        if (opts[i]->J_final) HIP_TRY(h0, hipMemcpy(opts[i]->J_final, h->dJ[final_parity[i]], jb, hipMemcpyDeviceToHost));
        if (opts[i]->idx_final) HIP_TRY(h0, hipMemcpy(opts[i]->idx_final, h->d_idx, ib, hipMemcpyDeviceToHost));
        if (res && res[i]) *res[i] = hjb_result{done[i], early[i], ms, mon[i].e, mon[i].e2};
    }
    return HJB_OK;
}

}  // extern "C"
