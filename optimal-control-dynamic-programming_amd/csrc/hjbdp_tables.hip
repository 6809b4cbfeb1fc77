// hjbdp_tables.hip - libhjbdp host side: the stage-invariant (cell, weight) tables - an axis' domain, the builds (variants 2 / 4 per
// outer axis, variants 5 - 7 per axis), their rebuild and hash - the eligibility of variants 5 and 6, and K9's examination and launch.
#include "hjbdp_host.h"
#include "kernels_prep_mfma.h"

namespace hjbhost {

uint32_t axis_mask(const hjb_problem *p, int a) {
    uint32_t m = 0;
    for (int k = 0; k < p->n_next_terms[a]; ++k) m |= p->next_terms[a][k].mask;
    return m;
}

AxisDomain axis_domain(const Handle *h, uint32_t mask) {
    const int D = h->hp.D, C = h->hp.C;
    const int owned_last = h->hp.n[D - 1];
    AxisDomain dom;
    dom.mask = mask;
    dom.dsz.assign(HJB_MAX_G, 1);
    for (int d = 0; d < D + C; ++d) {
        if (!dom.has(d)) continue;
        const int sz = (d < D) ? (d == D - 1 ? owned_last : h->prob.n[d]) : h->prob.m[d - D];
        dom.dsz[(size_t)d] = sz;
        dom.stride[d] = (int32_t)dom.entries;
        dom.entries *= sz;
    }
    return dom;
}

template <typename T>
void launch_prep(int D, int grid, const DParams *dp, int a, const int32_t *dsz, int64_t n, int2 *tab) {
    dim3 g(grid), b(256);
    switch (D) {
        case 2: hipLaunchKernelGGL((k_prep_axis_table<T, 2>), g, b, 0, nullptr, dp, a, dsz, n, tab); break;
        case 3: hipLaunchKernelGGL((k_prep_axis_table<T, 3>), g, b, 0, nullptr, dp, a, dsz, n, tab); break;
        case 4: hipLaunchKernelGGL((k_prep_axis_table<T, 4>), g, b, 0, nullptr, dp, a, dsz, n, tab); break;
        case 5: hipLaunchKernelGGL((k_prep_axis_table<T, 5>), g, b, 0, nullptr, dp, a, dsz, n, tab); break;
        case 6: hipLaunchKernelGGL((k_prep_axis_table<T, 6>), g, b, 0, nullptr, dp, a, dsz, n, tab); break;
        default: break;   // D == 1 has no outer axis
    }
}

template <typename T>
void launch_prep_t(int D, int grid, const DParams *dp, int a, const int32_t *dsz, int64_t n, TabEntry<T> *tab) {
    dim3 g(grid), b(256);
    switch (D) {
        case 1: hipLaunchKernelGGL((k_prep_axis_table_t<T, 1>), g, b, 0, nullptr, dp, a, dsz, n, tab); break;
        case 2: hipLaunchKernelGGL((k_prep_axis_table_t<T, 2>), g, b, 0, nullptr, dp, a, dsz, n, tab); break;
        case 3: hipLaunchKernelGGL((k_prep_axis_table_t<T, 3>), g, b, 0, nullptr, dp, a, dsz, n, tab); break;
        case 4: hipLaunchKernelGGL((k_prep_axis_table_t<T, 4>), g, b, 0, nullptr, dp, a, dsz, n, tab); break;
        case 5: hipLaunchKernelGGL((k_prep_axis_table_t<T, 5>), g, b, 0, nullptr, dp, a, dsz, n, tab); break;
        default: hipLaunchKernelGGL((k_prep_axis_table_t<T, 6>), g, b, 0, nullptr, dp, a, dsz, n, tab); break;
    }
}

// one outer axis' (cell, t) table over its broadcast domain (variant 2 / 4), registered for rebuilds; `wait`: until it is built
int build_axis_table(Handle *h, int a, const AxisDomain &dom, bool wait) {
    const int32_t *dsz_d = nullptr;
    int2 *tab = nullptr;
    int st3 = upload(h, dom.dsz, &dsz_d);
    if (!st3) st3 = dev_alloc(h, (size_t)dom.entries * sizeof(int2), &tab);
    if (st3) return st3;
    if (h->dtype != HJB_F64) launch_prep<float>(h->hp.D, prep_grid(dom.entries), h->dp, a, dsz_d, dom.entries, tab);
    else launch_prep<double>(h->hp.D, prep_grid(dom.entries), h->dp, a, dsz_d, dom.entries, tab);
    h->preps.push_back({a, 0, dsz_d, dom.dsz, dom.entries, tab});
    h->hn.at[a].tab = tab;
    if (!wait) return HJB_OK;
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, sync_setup());
    return HJB_OK;
}

// The axis-0 table of a mode-1 problem that runs without one (axis0_inline): built on demand for the kernels that read
// tables only (forced variant 2, option "axis0_table").
int ensure_axis0_table(Handle *h) {
    if (!h->axis0_inline) return HJB_OK;
    const int st = build_axis_table(h, 0, axis_domain(h, h->axis0_dom), true);
    if (st) return st;
    h->axis0_inline = false;
    if (h->packed_pre == 4) h->packed_pre = 1;          // (the caller chooses the launch again: mode 1 is the other instantiation)
    if (h->dn) HIP_TRY(h, hipMemcpy(h->dn, &h->hn, sizeof(DNested), hipMemcpyHostToDevice));
    return HJB_OK;
}

// float64-built entries narrowed to the float32 tables the stage kernels read: the weight is rounded ONCE, here
__global__ void __launch_bounds__(256)
k_tab_narrow(const TabEntry<double> *__restrict__ in, TabEntry<float> *__restrict__ out, int64_t n) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        TabEntry<float> o;
        o.cell = in[e].cell;
        o.t = (float)in[e].t;
        out[e] = o;
    }
}

// One axis' (cell, weight) table in the handle's table dtype.
template <typename T>
int launch_prep_any(Handle *h, int D, int grid, int a, const int32_t *dsz, int64_t n, TabEntry<T> *tab) {
    if constexpr (std::is_same<T, float>::value) {
        if (h->tab64) {
            void *tmp = nullptr;
            // fault injection: hjb_test_hook("fail_tab64_scratch", 1) - an explicit call from inside the process, never the
            // environment - makes this allocation fail (tests/test_gpu_types.py checks that hjb_create then fails instead of
            // handing out a handle on float32 queries)
            if (g_test_fail_tab64_scratch.load() || hipMalloc(&tmp, (size_t)n * sizeof(TabEntry<double>)) != hipSuccess) return fail(h, HJB_E_NOMEM, "float64 table build: scratch of %lld entries", (long long)n);
            launch_prep_t<double>(D, grid, h->dp64, a, dsz, n, (TabEntry<double> *)tmp);
            hipLaunchKernelGGL(k_tab_narrow, dim3(grid), dim3(256), 0, nullptr, (const TabEntry<double> *)tmp, tab, n);
            const hipError_t e1 = sync_setup();
            (void)hipFree(tmp);
            if (e1 != hipSuccess) return fail(h, HJB_E_DEVICE, "float64 table build: %s", hipGetErrorString(e1));
            return HJB_OK;
        }
    }
    launch_prep_t<T>(D, grid, h->dp, a, dsz, n, tab);
    return HJB_OK;
}

template <typename T>
int ensure_tabled_t(Handle *h) {
    if (h->dtb) return HJB_OK;
    const int D = h->hp.D, C = h->hp.C;
    DTabled &TBh = h->htb;
    memset(&TBh, 0, sizeof TBh);
    for (int a = 0; a < D; ++a) {
        DTabled::Axis &A = TBh.ax[a];
        const AxisDomain dom = axis_domain(h, h->dom_mask[a]);
        for (int d = 0; d < D; ++d) A.sstride[d] = dom.stride[d];
        for (int c = 0; c < C; ++c)
            if (dom.has(D + c)) { A.cstride[c] = dom.stride[D + c]; A.has_ctrl = 1; }
        const int32_t *dsz_d = nullptr;
        TabEntry<T> *tab = nullptr;
        int st3 = upload(h, dom.dsz, &dsz_d);
        if (st3) return st3;
        if (g_test_fail_tabled_alloc.load()) return fail(h, HJB_E_NOMEM, "(cell, t) table of axis %d: allocation failed (test hook)", a);
        st3 = dev_alloc(h, (size_t)dom.entries * sizeof(TabEntry<T>), &tab);
        if (!st3) st3 = launch_prep_any<T>(h, D, prep_grid(dom.entries), a, dsz_d, dom.entries, tab);
        if (st3) return st3;
        h->preps.push_back({a, 1, dsz_d, dom.dsz, dom.entries, tab});
        A.tab = tab;
    }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, sync_setup());
    void *d = nullptr;
    int st3 = dev_alloc(h, sizeof(DTabled), &d);
    if (st3) return st3;
    HIP_TRY(h, hipMemcpy(d, &TBh, sizeof(DTabled), hipMemcpyHostToDevice));
    h->dtb = (DTabled *)d;
    return HJB_OK;
}

int ensure_tabled(Handle *h) { return h->dtype != HJB_F64 ? ensure_tabled_t<float>(h) : ensure_tabled_t<double>(h); }

// Variants 5 / 6 eligibility: every axis' domain (Handle::dom_mask, dom_entries; the tables are built lazily, on first use), whether
// the tables fit (tabled_ok, tabled_i32), and the row kernel's forms (row_ok, row_lean_ok, row_auto).  entry_bytes: sizeof(TabEntry<T>).
void analyse_tabled(Handle *h, const hjb_problem *p, size_t entry_bytes) {
    const DParams &P = h->hp;
    const int D = p->D;
    size_t total = 0;
    bool fits = true;
    for (int a = 0; a < D; ++a) {
        const AxisDomain dom = axis_domain(h, axis_mask(p, a));
        h->dom_mask[a] = dom.mask;
        h->dom_entries[a] = dom.entries;
        if (dom.entries >= ((int64_t)1 << 31)) fits = false;
        total += (size_t)dom.entries * entry_bytes;
    }
    // worth it only when the tables are small next to the per-stage work (nS * nU backups)
    const bool small = total <= ((size_t)512 << 20) || (double)total <= 0.5 * (double)h->n_owned * (double)h->nU;
    h->tabled_ok = fits && small && total <= ((size_t)16 << 30);
    {   // the 32-bit form of the table kernel: owned states, the haloed J, every axis table (checked above) and the largest
        // table a cost term can address (global states x controls) all below 2^31 entries
        int64_t ns_global = 1;
        for (int d = 0; d < D; ++d) ns_global *= p->n[d];
        const int64_t lim = kTab32Lim;                                     // (room for the grid-stride step on top of the last index: kernels_tabled.h)
        h->tabled_i32 = h->tabled_ok && h->n_owned < lim && h->j_elems < lim && h->nU < lim &&
                        (double)ns_global * (double)h->nU < (double)lim;
    }
    // variant 6: no axis other than axis 0 may depend on state dim 0 (its cells are then uniform along a row)
    bool rw = h->tabled_ok && D >= 2 && !p->model;
    for (int a = 1; a < D; ++a) rw = rw && (h->dom_mask[a] & 1u) == 0;
    h->row_ok = rw;
    {   // lean form: few controls, 32-bit element offsets, control terms of the cost involve controls only
        bool ln = rw && h->nU <= 64 && h->j_elems * (int64_t)h->esz < ((int64_t)1 << 32) && (P.n_cost - P.n_cost_prefix) <= kLeanMaxCu;
        const uint32_t smask = (1u << D) - 1u;
        for (int k = P.n_cost_prefix; k < P.n_cost; ++k) ln = ln && (p->cost_terms[k].mask & smask) == 0;
        h->row_lean_ok = ln;
    }
    // worth it when rows fill a fair part of the 64-lane waves (C4 120^4: 1.9x over variant 5 in the lean form; 60^4: 1.4x).  Round 4
    // measured the small and odd-sized pos-att grids too (profiles/r04_small_grids.log): the reference's own 30x30x20x15 (47 % of
    // the lanes live, 2.7e5 states) 17.9 against 22.2 us per stage, 33x64x48x32 (52 %) 134 against 170 us, 80x80x60x40 (63 %) 0.52
    // against 0.79 ms - rounds 1 - 3 asked for 70 % and 2^20 states and left those on variant 5
    const double lane_use = (double)p->n[0] / (64.0 * (double)((p->n[0] + 63) / 64));
    // (the lean form only - control terms of the cost over controls alone; with a materialised (state, control) cost table, the
    // mirrors' cost_mode 'exact', the row kernel takes 31 us per stage on that grid against the tabled kernel's 22: the old rule stays)
    h->row_auto = rw && ((h->row_lean_ok && lane_use >= 0.45) || (lane_use >= 0.7 && h->n_owned >= ((int64_t)1 << 20)));
}

// Rebuild every (cell, weight) table of the handle, with the vector term-sum kernels or - where an axis' last term
// is separable from the others - with the MFMA outer-sum kernel (kernels_prep_mfma.h).  Same bits either way.
static bool prep_split(const Handle *h, const Handle::PrepRec &R, DPrepSplit *S) {
    const hjb_problem &p = h->prob;
    const int a = R.axis, nt = p.n_next_terms[a], G = p.D + p.C;
    if (h->dtype == HJB_F64 || h->tab64 || nt < 2) return false;
    uint32_t others = 0;
    for (int k = 0; k + 1 < nt; ++k) others |= p.next_terms[a][k].mask;
    const uint32_t last = p.next_terms[a][nt - 1].mask;
    if (!last || !others || (last & others)) return false;
    memset(S, 0, sizeof *S);
    int64_t stride = 1, nr = 1, nc = 1;
    for (int d = 0; d < G; ++d) {
        const int sz = R.dsz[(size_t)d];
        const bool in_dom = ((last | others) >> d) & 1u;
        if (!in_dom) { if (sz != 1) return false; continue; }
        if ((last >> d) & 1u) {
            S->col_dim[S->n_col_dims] = d; S->col_size[S->n_col_dims] = sz; S->col_estride[S->n_col_dims++] = (int32_t)stride;
            nc *= sz;
        } else {
            S->row_dim[S->n_row_dims] = d; S->row_size[S->n_row_dims] = sz; S->row_estride[S->n_row_dims++] = (int32_t)stride;
            nr *= sz;
        }
        stride *= sz;
    }
    if (nr * nc != R.n || nr >= ((int64_t)1 << 31) || nc >= ((int64_t)1 << 31)) return false;
    S->n_rows = (int32_t)nr;
    S->n_cols = (int32_t)nc;
    return true;
}

static int rebuild_tables_timed(Handle *h, bool mfma, hipEvent_t e0, hipEvent_t e1) {
    HIP_TRY(h, hipEventRecord(e0, nullptr));
    const int D = h->hp.D;
    int n_mfma = 0;
    for (const auto &R : h->preps) {
        DPrepSplit S;
        if (mfma && prep_split(h, R, &S)) {
            const int64_t tiles = (int64_t)((S.n_rows + 31) / 32) * ((S.n_cols + 31) / 32);
            dim3 g((unsigned)std::min<int64_t>((tiles + 3) / 4, 65536)), b(256);
            switch (D) {
                case 1: hipLaunchKernelGGL((k_prep_axis_table_mfma<1>), g, b, 0, nullptr, h->dp, R.axis, S, (int2 *)R.tab); break;
                case 2: hipLaunchKernelGGL((k_prep_axis_table_mfma<2>), g, b, 0, nullptr, h->dp, R.axis, S, (int2 *)R.tab); break;
                case 3: hipLaunchKernelGGL((k_prep_axis_table_mfma<3>), g, b, 0, nullptr, h->dp, R.axis, S, (int2 *)R.tab); break;
                case 4: hipLaunchKernelGGL((k_prep_axis_table_mfma<4>), g, b, 0, nullptr, h->dp, R.axis, S, (int2 *)R.tab); break;
                case 5: hipLaunchKernelGGL((k_prep_axis_table_mfma<5>), g, b, 0, nullptr, h->dp, R.axis, S, (int2 *)R.tab); break;
                default: hipLaunchKernelGGL((k_prep_axis_table_mfma<6>), g, b, 0, nullptr, h->dp, R.axis, S, (int2 *)R.tab); break;
            }
            ++n_mfma;
            continue;
        }
        const int grid = prep_grid(R.n);
        if (h->dtype == HJB_F64) {
            if (R.kind == 0) launch_prep<double>(D, grid, h->dp, R.axis, R.dsz_d, R.n, (int2 *)R.tab);
            else launch_prep_t<double>(D, grid, h->dp, R.axis, R.dsz_d, R.n, (TabEntry<double> *)R.tab);
        } else {
            if (R.kind == 0) launch_prep<float>(D, grid, h->dp, R.axis, R.dsz_d, R.n, (int2 *)R.tab);
            else { const int pst = launch_prep_any<float>(h, D, grid, R.axis, R.dsz_d, R.n, (TabEntry<float> *)R.tab); if (pst) return pst; }
        }
    }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(e1, nullptr));
    HIP_TRY(h, hipEventSynchronize(e1));
    float ms = 0;
    HIP_TRY(h, hipEventElapsedTime(&ms, e0, e1));
    h->prep_us = (double)ms * 1e3;
    h->prep_mfma = mfma ? 1 : 0;
    h->prep_mfma_axes = n_mfma;
    return HJB_OK;
}

int rebuild_tables(Handle *h, bool mfma) {
    // the tables are rewritten IN PLACE: wait for the whole device, not only for the null stream - a stage may still be in flight
    // on the handle's own stream, a rank's strip streams or a caller's stream (hjb_backup_stage_device).  Not a hot path.  
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); return fail(h, HJB_E_DEVICE, "hipEventCreate failed"); }
    const int st = rebuild_tables_timed(h, mfma, e0, e1);
    (void)hipEventDestroy(e0);         // one exit: the events never leak
    (void)hipEventDestroy(e1);
    return st;
}

int table_hash(Handle *h, uint64_t *out) {      // FNV-1a over the bytes of every table, in registration order
    uint64_t hsh = 1469598103934665603ull;
    std::vector<unsigned char> buf;
    for (const auto &R : h->preps) {
        const size_t bytes = (size_t)R.n * ((h->dtype == HJB_F64 && R.kind == 1) ? 16 : 8);
        buf.resize(bytes);
        HIP_TRY(h, hipMemcpy(buf.data(), R.tab, bytes, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < bytes; ++i) { hsh ^= buf[i]; hsh *= 1099511628211ull; }
    }
    *out = hsh;
    return HJB_OK;
}

// K9 applies when, for every state and control, each axis' interpolation cell is the state's own cell or the one
// below (clamped to the grid): then J_k at a state depends on J_{k+1} within +-1 cell only.  Checked on the host
// from the variant-5 tables (small: 2-D problems only).
template <typename T>
int examine_tile2d_t(Handle *h) {
    h->tile2d = 0;
    const DParams &P = h->hp;
    if (P.D != 2 || h->j_elems != h->n_owned || !h->tabled_ok || h->hp.model) return HJB_OK;
    // few controls only (the launch-bound channels this is for), and tables small enough that checking them on the
    // host costs nothing next to the sweep
    if (h->nU > 64 || h->dom_entries[0] + h->dom_entries[1] > ((int64_t)1 << 24)) return HJB_OK;
    int st = ensure_tabled(h);
    if (st) return st;
    for (int a = 0; a < 2; ++a) {
        std::vector<TabEntry<T>> tab((size_t)h->dom_entries[a]);
        HIP_TRY(h, hipMemcpy(tab.data(), h->htb.ax[a].tab, tab.size() * sizeof(TabEntry<T>), hipMemcpyDeviceToHost));
        // entry index -> this axis' state index: strides of the table domain
        const DTabled::Axis &A = h->htb.ax[a];
        const int na = P.n[a];
        if (A.sstride[a] == 0) return HJB_OK;               // x_next_a does not depend on x_a: not a local problem
        // walk every entry: its axis-a index is (e / sstride[a]) % n[a] because domains are dense column-major
        for (int64_t e = 0; e < h->dom_entries[a]; ++e) {
            const int i = (int)((e / A.sstride[a]) % na);
            const int lo = std::max(i - 1, 0), hi = std::min(i, na - 2);
            if (tab[(size_t)e].cell < lo || tab[(size_t)e].cell > hi) return HJB_OK;
        }
    }
    h->tile2d = 1;
    if (P.C == 1 && h->nU <= kTileMaxU) {          // the cached form: its per-(state, control) plan, built once
        const int64_t ne = h->n_owned * h->nU;
        void *d = nullptr;
        st = dev_alloc(h, (size_t)ne * sizeof(TilePlan<T>), &d);
        if (st) return st;
        (void)stage_tile2d_plan(h->dtype, h->dp, h->dtb, d, ne);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, sync_setup());
        h->tile_plan = d;
    }
    return HJB_OK;
}

int examine_tile2d(Handle *h) { return h->dtype != HJB_F64 ? examine_tile2d_t<float>(h) : examine_tile2d_t<double>(h); }

int launch_tile2d(Handle *h, const void *dJn, void *dJo, void *didx, int K, hipStream_t st) {
    const DParams &P = h->hp;
    StageArgs a = stage_args(h, dJn, dJo, didx, st);
    a.grid = (unsigned)(((P.n[0] + kTileX - 1) / kTileX) * ((P.n[1] + kTileY - 1) / kTileY));
    a.block = 256;
    (void)stage_tile2d(a, h->tile_plan, K);      // the cached form when its plan exists
    HIP_TRY(h, hipGetLastError());
    return HJB_OK;
}

}  // namespace hjbhost
