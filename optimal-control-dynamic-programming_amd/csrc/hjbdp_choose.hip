// hjbdp_choose.hip - libhjbdp host side: which kernel variant serves a handle, in which form, with which grid, block and LDS
// (variant_status, choose_launch -> Handle::L), and the stage launch that dispatches on it.
#include "hjbdp_host.h"
#include "hjbdp_walk.h"
#include "kernels_evaluate.h"      // EvalDiv

namespace hjbhost {

// What kernel variant v needs of the handle - the one statement of it: HJB_OK, or the status and (*why) the reason it cannot serve.
// Once the typing and the structure admit v, the tables or plan it reads are built here (never inside a launch: launches may be under
// graph capture); a failed build gives the build's status.
int variant_status(Handle *h, int v, const char **why) {
    auto no = [&](const char *reason) { *why = reason; return (int)HJB_E_UNSUPPORTED; };
    if (h->dist_nodes > 0) return v == 8 ? (int)HJB_OK : no("a handle with a disturbance runs on variant 8 only");
    if (v == 8) return no("variant 8 serves a handle with a disturbance (hjb_set_disturbance)");
    if (h->hp.model && v != 4) return no("a problem with a state model runs on variant 4 only");
    if (h->tab64 && v < 5)
        return no("it evaluates the next-state terms in the kernel, in float32; a problem with table_dtype HJB_TAB_F64 runs on the "
                  "table-driven kernels (5, 6, 7)");
    if (h->cost64 && v != 5 && v != 7)
        return no("it sums the stage cost in float32; a problem with cost_dtype HJB_COST_F64 runs on the tabled kernel (5) or the column sweep (7)");
    if (h->dtype == HJB_F16S && v >= 1 && v <= 3) return no("it does not support float16 J storage (use 0, 4, 5, 6 or 7)");
    if (h->dtype == HJB_F64 && (v == 2 || v == 4 || v == 7)) return no("it is float32 arithmetic only");
    int st = HJB_OK;
    switch (v) {
        case 1:
            if (!h->nested_ok) return no("variant 1 (control-nested) needs: only the last state axis depends on the innermost control dim");
            break;
        case 2:
            if (h->packed_mode != 1) return no("variant 2 (packed) needs the canonical spacecraft structure (see kernels_packed.h)");
            st = ensure_axis0_table(h);          // variant 2 reads every axis from its table
            break;
        case 4:
            if (!h->packed_mode) return no("variant 4 (packed, control pairs) needs the canonical spacecraft structure");
            break;
        case 5:
            if (!h->tabled_ok) return no("variant 5 (tabled) needs per-axis tables that fit");
            st = ensure_tabled(h);
            break;
        case 6:
            if (!h->row_ok)
                return no("variant 6 (one wave per grid row) needs D >= 2, per-axis tables that fit, and no axis other than axis 0 depending "
                          "on state dim 0");
            st = ensure_tabled(h);
            break;
        case 7:
            if ((st = ensure_colsweep(h)) != HJB_OK) break;
            if (h->cs_state != 1)
                return no("variant 7 (column sweep) needs D = 4, one control dim, axes 0/1 independent of the control (and of each other's "
                          "state dim), axes 2/3 depending on state dims 2, 3 and the control only, control terms of the cost involving the "
                          "control only, and at most kCsGMax groups of corner rows per (i2, i3)");
            if (h->cost64 && !(colsweep_usual_cost(h) && !h->hcs.coop))
                return no("it sums float64 cost terms in its usual cost shape only (state terms + one control term), not in the cooperative form");
            break;
        default:
            break;
    }
    if (st) *why = h->err.c_str();       // the build's own message
    return st;
}

// The automatic choice: the first of variants 4, 1, 3 that applies by structure and serves, else 7, 6, 5, 0.  Variant 7 wants what 6
// wants - long axis-0 rows on a large grid - plus its own structure; its plan is examined only where 4, 1 and 3 do not apply by structure.
static int auto_variant(Handle *h) {
    const char *why = nullptr;
    // few states x many controls (Kirk): one wave per state, controls across lanes (too many controls for variant 7)
    const bool want_split = h->nU >= 64 && h->n_owned < 512 * 1024;
    const int first = h->packed_mode ? 4 : (h->nested_ok ? 1 : (want_split ? 3 : -1));
    if (first >= 0 && variant_status(h, first, &why) == HJB_OK) return first;
    if (first < 0 && h->row_auto && variant_status(h, 7, &why) == HJB_OK) return 7;
    return h->row_auto ? 6 : (h->tabled_ok ? 5 : 0);
}

// Handle::L: the variant in effect (8 while a disturbance is set, the model's 4, the forced one, or the automatic choice), its form, grid, block and LDS.  A variant
// that does not serve falls to the tabled kernel (float64 cost terms in a shape or form variant 7 does not sum them in), and one whose
// tables could not be built to the generic kernel - where that serves: a float64-typed handle keeps its variant and the build's status
// instead, and hjb_create refuses it.
void choose_launch(Handle *h) {
    const char *why = nullptr;
    int v = h->dist_nodes > 0 ? 8 : h->hp.model ? 4 : (h->forced_variant >= 0 ? h->forced_variant : auto_variant(h));
    int st = variant_status(h, v, &why);
    if (st == HJB_E_UNSUPPORTED) st = variant_status(h, v = 5, &why);
    if (st != HJB_OK && variant_status(h, 0, &why) == HJB_OK) { v = 0; st = HJB_OK; }
    const DParams &P = h->hp;
    Launch L;
    L.variant = v;
    L.status = st;
    switch (v) {
        case 1:
            L.fast = h->nested_fast;
            L.lds = h->nested_lds;
            break;
        case 2:
            L.lds = h->packed_lds;
            break;
        case 3:
            // J staged in LDS: eight waves share one copy of J (Kirk: 40 KB), so four workgroups fill a CU's 32 wave slots instead of half
            // of them (Kirk's default problem 16.1 -> 13.4 ms per 199 stages: profiles/r06_xcd_shares_and_spans.log)
            L.j_in_lds = (size_t)h->j_elems * h->esz <= 64 * 1024;
            if (L.j_in_lds) { L.block = 512; L.lds = (size_t)h->j_elems * h->esz; }
            break;
        case 4:
            L.mode = uniwin_active(h) ? h->packed_pre + 2 : h->packed_pre;      // 7 / 8: K15
            if (L.mode >= 7) L.block = h->huw.block;
            L.lds = (L.mode >= 7 ? h->uw_lds : h->packed2_lds) + h->lds_pad;
            break;
        case 6: {
            L.lean = h->row_lean && h->row_lean_ok && !h->htb.ax[0].has_ctrl;
            const size_t tsz = h->dtype != HJB_F64 ? 4 : 8;
            const size_t lean_wave = (((size_t)h->nU * 4 + 15) & ~(size_t)15) + (((size_t)h->nU * (P.D - 1 + kLeanMaxCu) * tsz + 15) & ~(size_t)15);
            if (L.lean) L.lds = 4 * lean_wave + (size_t)h->nU * 12;
            break;
        }
        case 7:
            L.cost_form = h->cost64 ? 2 : (colsweep_usual_cost(h) ? 1 : 0);
            L.dpp = h->hcs.dpp != 0;
            break;
        default:
            break;
    }
    const int per_block = v == 2 ? 512 : (v == 3 ? L.block / 64 : 256);   // states per workgroup pass (variant 4: 256)
    const int64_t blocks = (h->n_owned + per_block - 1) / per_block;
    // A launch smaller than the work walks it in equally long, grid-sized spans (hjbdp_walk.h, launch_spans)
    // (the control-split kernel keeps its 1024 workgroups: one wave per state and few states - Kirk's 2500 blocks as 3 x 840 ran 19.3 ms
    // per 199 stages against 16.3 with a short last span that overlaps the tail of the one before)
    // The table kernel takes its whole grid as ONE span where its 32-bit form allows (XCD x then sweeps one contiguous eighth of the
    // grid: 13M states 0.671 -> 0.630 ms, Solver_attitude.run in the reference's order 13.7 -> 12.9 ms per 19 stages; 2e8 states: equal)
    const int64_t cap = v == 5 ? kTab32MaxThreads / 256 : 256 * 16;
    L.grid = v == 3 ? (int)std::min<int64_t>(blocks, L.block == 512 ? 2048 : 1024) : (int)hjb::launch_spans(blocks, cap);
    if (v == 6) {       // one wave per (64-state chunk of a) grid row, four waves per workgroup
        const int64_t items = (h->n_owned / P.n[0]) * ((P.n[0] + 63) / 64);
        L.grid = (int)hjb::launch_spans((items + 3) / 4, 1 << 20);        // (one span where it can: C4 in the reference's order 6.49 -> 6.15 ms per stage)
    }
    if (v == 7) {       // one wave per (chunk of axis 0, i2, i3) column; workgroup b serves XCD b % 8
        const DColSweep &CS = h->hcs;
        const int lanes = CS.dpp ? kCsDppLanes : 64;
        const int64_t chunks = (P.n[0] + lanes - 1) / lanes;
        const int64_t nwax = P.n[5 - CS.gax];
        int64_t most = 0;
        const int64_t nfull = CS.xcd_win ? P.n[CS.gax] : nwax;      // the axis every XCD walks in full
        for (int x = 0; x < 8; ++x) most = std::max<int64_t>(most, (int64_t)CS.xcd_cnt[x] * chunks * nfull * CS.split);
        L.grid = (int)(8 * ((most + 3) / 4));
        if (CS.coop && !CS.xcd_win) {       // cooperative form: one workgroup of kCcW waves per (group-axis index, 64-state chunk, kCcW columns)
            const int64_t c64 = (P.n[0] + 63) / 64, nblk = (nwax + kCcW - 1) / kCcW;
            int64_t mostc = 0;
            for (int x = 0; x < 8; ++x) mostc = std::max<int64_t>(mostc, (int64_t)CS.xcd_cnt[x] * c64 * nblk);
            L.coop_grid = (int)(8 * mostc);
        }
    }
    if (L.mode >= 7) {  // K15: as many workgroups as the device holds at once (a persistent walk: a second generation would run alone)
        const DUniwin &U = h->huw;
        int occ = stage_uniwin_occupancy(h->dtype, P.D, P.model != 0, U.block, L.lds);
        if (occ < 1) occ = U.block == 64 ? 16 : 4;
        hipDeviceProp_t prop;
        int cus = 256;
        if (hipGetDeviceProperties(&prop, h->device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
        const int64_t g = std::min<int64_t>((int64_t)occ * cus, (int64_t)((U.n_v + 7) / 8) * 8);
        L.grid = (int)std::max<int64_t>(8, g - (g & 7));
    }
    if (L.grid < 1) L.grid = 1;
    h->L = L;
    launch_changed(h);
}

// After every change to Handle::L (choose_launch, options "grid", "block", "tabled_i32"): the fields that depend on the final grid, and
// the captured stage loop - it holds the old launches - is dropped.
void launch_changed(Handle *h) {
    Launch &L = h->L;
    L.idx32 = L.variant == 5 && h->tabled_i32 && h->tabled_i32_on && (int64_t)L.grid * L.block <= kTab32MaxThreads;
    if (h->gexec) { (void)hipGraphExecDestroy(h->gexec); h->gexec = nullptr; }
}

// One stage: the launch Handle::L on (dJn -> dJo, didx).  The kernels live in translation units of their own (stage_*.hip behind
// hjbdp_launch.h); this is the only place that knows which family serves which variant.
int launch_stage(Handle *h, const void *dJn, void *dJo, void *didx, hipStream_t st) {
    const Launch &L = h->L;
    if (L.status != HJB_OK) return fail(h, L.status, "kernel variant %d cannot run on this handle (status %d)", L.variant, L.status);
    StageArgs a = stage_args(h, dJn, dJo, didx, st);
    a.grid = (unsigned)L.grid;
    a.block = (unsigned)L.block;
    a.lds = L.lds;
    a.idx32 = L.idx32;
    int miss = 0;
    switch (L.variant) {
        case 7:
            // cooperative form: its staging loads are 16 bytes wide (a J pointer handed in unaligned runs the other form)
            if (L.coop_grid > 0 && ((uintptr_t)dJn & 15u) == 0) {
                a.grid = (unsigned)L.coop_grid;
                miss = stage_colcoop(a, h->hcs.gax, h->hcs.ng, L.cost_form == 1);
            } else {
                miss = stage_colsweep(a, h->hcs.gax, h->hcs.ng, L.cost_form, L.dpp);
            }
            if (miss) return fail(h, HJB_E_DEVICE, "variant 7: %d groups", h->hcs.ng);
            break;
        case 6: miss = stage_rowwise(a, L.lean); break;
        case 5: miss = stage_tabled(a); break;
        case 4:
            if (L.mode >= 7) {                       // K15 (kernels_uniwin.h)
                // the claim counters are per stream: two launches in flight on different streams never share (and re-zero) a set.
                // A stream is given a set on its first launch (host bookkeeping only: nothing is allocated, also under capture)
                int set = 0;
                while (set < h->uw_nstreams && h->uw_streams[set] != st) ++set;
                if (set == h->uw_nstreams && set < kUwSets) h->uw_streams[h->uw_nstreams++] = st;
                a.duw = h->duw + set;                // (set kUwSets: the static walk)
                if (h->uw_claim && set < kUwSets)    // (a memset node under capture)
                    HIP_TRY(h, hipMemsetAsync(h->huw.counters + (size_t)kUwSetWords * set, 0, kUwSetWords * sizeof(uint32_t), st));
                miss = stage_uniwin(a, h->hp.model != 0);
            } else {
                miss = stage_packed2(a, L.mode);
            }
            break;
        case 3: miss = stage_ctrlsplit(a, L.j_in_lds); break;
        case 2: miss = stage_packed(a); break;
        case 1: miss = stage_nested(a, L.fast); break;
        case 0: miss = stage_generic(a); break;
        case 8:
            a.idx32 = dist_runs_i32(h);
            miss = h->dist_ctrl ? stage_ctrldist(a, h->tab64, h->tab64 ? h->dp64 : h->dp, h->d_dist, h->d_dist_tab, nullptr, nullptr)
                                : stage_disturb(a, h->tab64, h->tab64 ? h->dp64 : h->dp, h->d_dist, nullptr, nullptr);
            break;
        default:    // never fall through to the generic kernel silently
            return fail(h, HJB_E_DEVICE, "internal: kernel variant %d was not dispatched", L.variant);
    }
    if (miss) return fail(h, HJB_E_UNSUPPORTED, "variant %d has no kernel for D=%d, dtype %d", L.variant, a.D, h->dtype);
    HIP_TRY(h, hipGetLastError());
    return HJB_OK;
}

// The fixed-label stage (kernels_evaluate.h) - the one place its launch is decided.  Source of cells and weights: the handle's
// stage-invariant (cell, t) tables where it can hold them (a HJB_TAB_F64 handle always does: its float32 terms are copies for the
// host's analysis), else the terms summed on the fly; option "eval_tables" forces either where both exist (same bits).
int prepare_evaluate(Handle *h, bool *tabled) {
    if (h->hp.model)
        return fail(h, HJB_E_UNSUPPORTED, "the fixed-label stage does not evaluate a state model (HJB_MODEL_QUAT_EULER321): its next states are formed in variant 4 only");
    *tabled = h->eval_tables < 0 ? h->tabled_ok : h->eval_tables == 1;
    if (h->dist_nodes > 0) { *tabled = false; return HJB_OK; }      // variant 8's fixed-label form: an offset query has no table entry, nothing is built
    if (!*tabled && h->tab64) return fail(h, HJB_E_UNSUPPORTED, "table_dtype HJB_TAB_F64 is evaluated from the (cell, weight) tables only");
    return *tabled ? ensure_tabled(h) : HJB_OK;
}

int launch_evaluate(Handle *h, const void *dJn, const void *dlabels, void *dJo, hipStream_t st) {
    bool tabled = false;
    const int pst = prepare_evaluate(h, &tabled);
    if (pst) return pst;
    StageArgs a = stage_args(h, dJn, dJo, nullptr, st);
    a.grid = (unsigned)eval_grid_of(h);
    a.block = 256;
    a.idx32 = eval_runs_i32(h);
    if (h->dist_nodes > 0) {                               // the same kernel as the disturbed backup, one candidate per state
        a.idx32 = dist_runs_i32(h);
        if (h->dist_ctrl ? stage_ctrldist(a, h->tab64, h->tab64 ? h->dp64 : h->dp, h->d_dist, h->d_dist_tab, dlabels, h->d_status + 1)
                         : stage_disturb(a, h->tab64, h->tab64 ? h->dp64 : h->dp, h->d_dist, dlabels, h->d_status + 1))
            return fail(h, HJB_E_UNSUPPORTED, "variant 8 has no fixed-label kernel for D=%d, dtype %d", a.D, h->dtype);
        HIP_TRY(h, hipGetLastError());
        return HJB_OK;
    }
    EvalDiv dv{};                                          // the divisors the kernel takes a state index and a label apart by
    for (int d = 0; d < HJB_MAX_D; ++d) dv.n[d] = hjb::magic_div(d < h->hp.D ? (uint32_t)h->hp.n[d] : 1u);
    for (int c = 0; c < 2; ++c) dv.m[c] = hjb::magic_div((uint32_t)h->hp.m[c]);
    if (stage_evaluate(a, tabled, eval_runs_m24(h, tabled), dlabels, h->d_status + 1, dv)) return fail(h, HJB_E_UNSUPPORTED, "the fixed-label stage has no kernel for D=%d, dtype %d", a.D, h->dtype);
    HIP_TRY(h, hipGetLastError());
    return HJB_OK;
}

// 24-bit index products: every factor the 32-bit form multiplies below 2^24 - sizes, the quotients of the state index (the
// first is the largest), the J strides, the strides of the tables or terms it reads and of the cost terms.  Strides are never
// negative: make_term and axis_domain form them as products of sizes (0 = broadcast), so an upper bound is a bound.  The table
// strides are axis_domain's, which ensure_tabled copies into the tables it builds: the answer is the same before and after the
// first launch has built them.  cost64[] is made from the same hjb_term as cost[] (upload_cost): the same strides.
bool eval_runs_m24(const Handle *h, bool tabled) {
    constexpr int64_t k24 = (int64_t)1 << 24;
    const DParams &P = h->hp;
    auto small = [&](const DTerm &t) { for (int d = 0; d < HJB_MAX_G; ++d) if (t.stride[d] >= k24) return false; return true; };
    bool mul24 = eval_runs_i32(h) && h->eval_m24;
    mul24 = mul24 && h->n_owned / P.n[0] < k24 && h->nU < k24;
    for (int d = 0; d < P.D && mul24; ++d) {
        mul24 = h->prob.n[d] < k24 && P.jstride[d] < k24 && h->nplanes < k24;      // (prob.n: the GLOBAL sizes the terms are indexed by)
        if (mul24 && tabled) {
            const AxisDomain dom = axis_domain(h, h->dom_mask[d]);
            for (int k = 0; k < P.D + P.C && mul24; ++k) mul24 = dom.stride[k] < k24;      // (DTabled::Axis sstride[], cstride[])
        }
        for (int k = 0; k < P.axis[d].n_terms && mul24 && !tabled; ++k) mul24 = small(P.axis[d].t[k]);
    }
    for (int k = 0; k < P.n_cost && mul24; ++k) mul24 = small(P.cost[k]);
    return mul24;
}

int eval_form(const Handle *h) {
    const bool tabled = h->eval_tables < 0 ? h->tabled_ok : h->eval_tables == 1;      // (prepare_evaluate's source, nothing built)
    return eval_runs_m24(h, tabled) ? 2 : eval_runs_i32(h) ? 1 : 0;
}

}  // namespace hjbhost
