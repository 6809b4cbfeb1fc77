// hjbdp_colsweep.hip - libhjbdp host side: variant 7 (kernels_colsweep.h, kernels_colcoop.h) - eligibility, the per-(i2, i3) plan, the
// column -> XCD map, the DPP test, the cooperative plan, the launch record and the split rule.
#include "hjbdp_host.h"

namespace hjbhost {

// the per-(i2, i3) plan, built once on the host from the variant-5 tables of axes 2 and 3 (tiny: n2 * n3 * nU entries)
template <typename T>
bool colsweep_plan(Handle *h, int gax, const std::vector<TabEntry<T>> (&tab)[2], const std::vector<std::vector<T>> &cu,
                   std::vector<int32_t> &plan, int64_t *rows_total, int *ng_max, std::vector<int32_t> &cells, int *mid_rows_out) {
    static_assert(sizeof(T) == 4, "plan words are 32-bit");
    const DParams &P = h->hp;
    const int n2 = P.n[2], n3 = P.n[3], nU = (int)h->nU, wax = 5 - gax;
    const int64_t gs = P.jstride[gax], ws = P.jstride[wax];
    const int nwk = wax == 3 ? h->nplanes : P.n[wax];        // knots of the window axis present in this handle's J buffers
    if (nwk < 3) return false;
    plan.assign((size_t)n2 * n3 * kCsPlanWords, 0);
    cells.assign((size_t)n2 * n3 * kCsGMax * 2, 0);         // (group-axis cell, first window knot) of every group
    *rows_total = 0;
    *ng_max = 1;
    int mid_rows = 0;
    auto bits = [](T x) { int32_t b; memcpy(&b, &x, 4); return b; };
    for (int i3 = 0; i3 < n3; ++i3) {
        for (int i2 = 0; i2 < n2; ++i2) {
            int32_t *q = &plan[(size_t)(i2 + n2 * i3) * kCsPlanWords];
            // a group: the cell cg of the group axis, window knots wmin .. wmin + 2 of the other axis, member slots
            // [0, MMAX/2) (window cell wmin) and [MMAX/2, MMAX) (window cell wmin + 1)
            struct Grp { int cg, wmin, slot[kCsMMax]; };
            Grp grp[kCsGMax];
            int ng = 0, bad = 0;
            int cc[2][kCsUMax];
            T tt[2][kCsUMax];
            for (int u = 0; u < nU; ++u) {
                for (int a = 2; a < 4; ++a) {
                    const DTabled::Axis &A = h->htb.ax[a];
                    const TabEntry<T> &e = tab[a - 2][(size_t)(A.sstride[2] * i2 + A.sstride[3] * i3 + A.cstride[0] * u)];
                    int c = e.cell;
                    if (a == 3) {                       // global plane -> plane of this handle's J buffers
                        c -= h->plane0;
                        if (c < 0 || c + 1 >= h->nplanes) { bad = 1; c = c < 0 ? 0 : h->nplanes - 2; }
                    }
                    cc[a - 2][u] = c;
                    tt[a - 2][u] = e.t;
                }
            }
            // windows per group-axis cell: the smallest uncovered window cell opens a window of two cells
            for (int u = 0; u < nU; ++u) {
                const int cg = cc[gax - 2][u], cw = cc[wax - 2][u];
                int wmin = cw;                              // the window this control belongs to: greedy cover, walked
                {                                           // from the smallest window cell among the controls of cg
                    int start = cw;
                    for (int v = 0; v < nU; ++v) if (cc[gax - 2][v] == cg) start = std::min(start, cc[wax - 2][v]);
                    for (;;) {
                        if (cw <= start + 1) { wmin = start; break; }
                        int nxt = cw;                       // the next uncovered cell opens the next window
                        for (int v = 0; v < nU; ++v)
                            if (cc[gax - 2][v] == cg && cc[wax - 2][v] > start + 1) nxt = std::min(nxt, cc[wax - 2][v]);
                        start = nxt;
                    }
                }
                // three knots wmin .. wmin + 2 must exist: the last window of the axis starts one knot lower
                if (wmin + 2 > nwk - 1) wmin = nwk - 3;
                const int pair = cw - wmin;                 // 0 or 1
                constexpr int PS = kCsMMax / 2;             // slots per window pair
                auto free_slot = [&](const Grp &G) {
                    for (int s = pair * PS; s < (pair + 1) * PS; ++s) if (G.slot[s] < 0) return s;
                    return -1;
                };
                int g = 0;
                for (; g < ng; ++g)
                    if (grp[g].cg == cg && grp[g].wmin == wmin && free_slot(grp[g]) >= 0) break;
                if (g == ng) {
                    if (ng == kCsGMax) return false;
                    grp[ng].cg = cg; grp[ng].wmin = wmin;
                    for (int s = 0; s < kCsMMax; ++s) grp[ng].slot[s] = -1;
                    ++ng;
                }
                grp[g].slot[free_slot(grp[g])] = u;
            }
            *ng_max = std::max(*ng_max, ng);
            q[0] = bad | (ng << 8);
            // visit the groups in ascending order of their highest control: fewer slots then come after a higher-numbered
            // control and need the (value, control number) comparison
            auto gmax = [&](const Grp &G) { int mx = -1; for (int s = 0; s < kCsMMax; ++s) mx = std::max(mx, G.slot[s]); return mx; };
            std::stable_sort(grp, grp + ng, [&](const Grp &a, const Grp &b) { return gmax(a) < gmax(b); });
            for (int g = 0; g < ng; ++g) {              // ascending control numbers inside each window pair
                std::sort(grp[g].slot, grp[g].slot + kCsMMax / 2, [](int a, int b) { return (unsigned)a < (unsigned)b; });
                std::sort(grp[g].slot + kCsMMax / 2, grp[g].slot + kCsMMax, [](int a, int b) { return (unsigned)a < (unsigned)b; });
            }
            int seen_max = -1;
            for (int g = 0; g < kCsGMax; ++g) {
                const Grp &G = grp[g < ng ? g : 0];                 // padding: a member-less copy of group 0's rows
                const int64_t off = (gs * G.cg + ws * G.wmin) * (int64_t)h->esz;
                const int nw = 3;
                int usedbits = 0;
                q[1 + g] = (int32_t)(uint32_t)off;
                cells[((size_t)(i2 + n2 * i3) * kCsGMax + g) * 2] = G.cg;
                cells[((size_t)(i2 + n2 * i3) * kCsGMax + g) * 2 + 1] = G.wmin;
                if (g < ng) {
                    // the kernels stop at a pair's first empty slot: used slots are a prefix of each pair
                    for (int pr = 0; pr < 2; ++pr)
                        for (int sidx = pr * (kCsMMax / 2) + 1; sidx < (pr + 1) * (kCsMMax / 2); ++sidx)
                            if (G.slot[sidx] >= 0 && G.slot[sidx - 1] < 0) return false;
                    *rows_total += 2 * nw;
                    for (int sidx = 0; sidx < kCsMMax; ++sidx) {
                        const int u = G.slot[sidx];
                        if (u < 0) continue;
                        usedbits |= 1 << sidx;
                        if (u < seen_max) usedbits |= 0x10000 << sidx;
                        seen_max = std::max(seen_max, u);
                        int32_t *sl = q + kCsPI + 8 * (g * kCsMMax + sidx);
                        sl[0] = bits(tt[wax - 2][u]);
                        sl[1] = bits(tt[gax - 2][u]);
                        sl[3] = u;
                        for (size_t k = 0; k < cu.size(); ++k) sl[k == 0 ? 2 : 3 + k] = bits(cu[k][(size_t)u]);
                        if (!h->cs_cu64.empty()) memcpy(&sl[4], &h->cs_cu64[(size_t)u], sizeof(double));
                    }
                }
                q[1 + kCsGMax + g] = usedbits | (nw << 8);
                if (i2 == n2 / 2 && i3 == n3 / 2 && g < ng)
                    mid_rows += 2 * (1 + ((usedbits & 7) != 0) + ((usedbits & 0x38) != 0));
            }
        }
    }
    *mid_rows_out = mid_rows;       // (the caller keeps the picked axis' count: the plans of both axes are built)
    return true;
}

// Column -> XCD assignment of variant 7 (DColSweep::xcd_ig): group-axis indices sorted by (index mod M, index), cut
// into 8 equal parts.  Default M = 1: plain contiguous ranges; option "cs_xcd_mod" sets M, -1 = the spacing of the
// groups' cells in a mid-grid plan.
static int colsweep_map(Handle *h, const std::vector<int32_t> &plan) {
    const DParams &P = h->hp;
    DColSweep &CSh = h->hcs;
    const int gax = CSh.gax, n2 = P.n[2], n3 = P.n[3];
    CSh.xcd_win = h->cs_xcd_axis ? 1 : 0;
    const int ngx = CSh.xcd_win ? P.n[5 - gax] : P.n[gax];          // indices of the axis the XCDs split
    int M = CSh.xcd_win ? 1 : h->cs_xcd_mod;
    if (M == 0) M = 1;           // measured on C4 (120^4 x 9): contiguous ranges 2.67 ms per stage, residue classes of the
                                 // group spacing (cs_xcd_mod = -1) 2.84 ms
    if (M < 0) {
        // spacing of the distinct group cells of the middle column, from the row offsets of its plan
        const int32_t *q = &plan[(size_t)(n2 / 2 + n2 * (n3 / 2)) * kCsPlanWords];
        const int ng = q[0] >> 8;
        const int64_t gb = P.jstride[gax] * (int64_t)h->esz, wb = P.jstride[5 - gax] * (int64_t)h->esz;
        std::vector<int64_t> cells;
        for (int g = 0; g < ng; ++g) {
            // row offset = gs * cg + ws * wmin (bytes): the group-axis cell is the quotient by the larger stride
            const int64_t off = (uint32_t)q[1 + g];
            cells.push_back(gax == 3 ? off / gb : (off % wb) / gb);
        }
        std::sort(cells.begin(), cells.end());
        cells.erase(std::unique(cells.begin(), cells.end()), cells.end());
        int64_t best = 0;
        for (size_t i = 1; i < cells.size(); ++i) best = best == 0 ? cells[i] - cells[i - 1] : std::min(best, cells[i] - cells[i - 1]);
        M = (int)std::max<int64_t>(1, std::min<int64_t>(best, ngx));
    }
    std::vector<int> order((size_t)ngx);
    for (int i = 0; i < ngx; ++i) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return (a % M) < (b % M); });
    const int stride = (ngx + 7) / 8;
    std::vector<int32_t> tab((size_t)8 * stride, 0);
    for (int x = 0; x < 8; ++x) {
        const int b = (int)((int64_t)ngx * x / 8), e = (int)((int64_t)ngx * (x + 1) / 8);
        CSh.xcd_cnt[x] = e - b;
        for (int i = b; i < e; ++i) tab[(size_t)x * stride + (i - b)] = order[(size_t)i];
    }
    CSh.xcd_stride = stride;
    return upload(h, tab, &CSh.xcd_ig);
}

// One-load form of variant 7: in every wave of kCsDppLanes consecutive axis-0 states, (cell - state index) is the same
// for all states but at most one (a cell clamped at the grid edge; the kernel gives that state a lane pair of its own).
template <typename T>
int colsweep_dpp_ok(Handle *h, bool *ok) {
    const DParams &P = h->hp;
    const DTabled::Axis &A0 = h->htb.ax[0];
    std::vector<TabEntry<T>> tab((size_t)h->dom_entries[0]);
    HIP_TRY(h, hipMemcpy(tab.data(), A0.tab, tab.size() * sizeof(TabEntry<T>), hipMemcpyDeviceToHost));
    const int n0 = P.n[0];
    const int r2 = A0.sstride[2] ? P.n[2] : 1, r3 = A0.sstride[3] ? P.n[3] : 1;
    *ok = true;
    for (int i3 = 0; i3 < r3 && *ok; ++i3)
        for (int i2 = 0; i2 < r2 && *ok; ++i2)
            for (int c = 0; c < n0 && *ok; c += kCsDppLanes) {
                const int e = std::min(n0, c + kCsDppLanes);
                auto rel = [&](int i0) { return tab[(size_t)(A0.sstride[0] * i0 + A0.sstride[2] * i2 + A0.sstride[3] * i3)].cell - i0; };
                // the common value is the one at least half of the states take (ties: the first state's, as in the kernel)
                const int r0 = rel(c);
                int same = 0;
                for (int i0 = c; i0 < e; ++i0) same += rel(i0) == r0;
                int kb = r0;
                if (2 * same < e - c)
                    for (int i0 = c; i0 < e; ++i0) if (rel(i0) != r0) { kb = rel(i0); break; }
                int odd = 0;
                for (int i0 = c; i0 < e; ++i0) odd += rel(i0) != kb;
                if (odd > 1) *ok = false;
            }
    return HJB_OK;
}

// Cooperative form of variant 7 (kernels_colcoop.h): a workgroup = kCcW columns that are neighbours along the window
// axis.  It applies when axis 1's cell does not depend on the window-axis index (the workgroup steps through one
// sequence of axis-1 knots), every workgroup's columns need at most `ng` distinct group-axis cells with window knots
// inside kCcNV staged ones, and their axis-0 cells inside kCcXW staged knots.  Fills plan word [1 + 2 GMAX + g] (the
// group's first corner row among the staged rows) and the per-workgroup words; sets h->cs_coop_epl.
template <typename T>
int colcoop_plan(Handle *h, std::vector<int32_t> &plan, const std::vector<int32_t> &cells, std::vector<int32_t> &wgw) {
    h->cs_coop_epl = 0;
    const DParams &P = h->hp;
    const DColSweep &CSh = h->hcs;
    const int gax = CSh.gax, wax = 5 - gax, n0 = P.n[0], n2 = P.n[2], n3 = P.n[3];
    h->cs_coop_why = 1;
    if (CSh.ng > kCcNCG) return HJB_OK;
    h->cs_coop_why = 2;
    if (h->dom_mask[1] & (1u << wax)) return HJB_OK;
    h->cs_coop_why = 3;
    const int epl = h->esz == 4 ? (n0 % 4 == 0 ? 4 : 0) : (h->esz == 2 ? (n0 % 8 == 0 ? 8 : 0) : 0);
    if (!epl || n0 < epl) return HJB_OK;
    const int nwk = wax == 3 ? h->nplanes : P.n[wax];
    const int ngx = P.n[gax], nwax = P.n[wax];
    const int chunks = (n0 + 63) / 64, nblk = (nwax + kCcW - 1) / kCcW;
    const int xw = h->esz == 2 ? kCcXWh : kCcXW;
    const int rowb = xw * (int)h->esz;
    const DTabled::Axis &A0 = h->htb.ax[0];
    std::vector<TabEntry<T>> tab0((size_t)h->dom_entries[0]);
    HIP_TRY(h, hipMemcpy(tab0.data(), A0.tab, tab0.size() * sizeof(TabEntry<T>), hipMemcpyDeviceToHost));
    wgw.assign((size_t)ngx * chunks * nblk * kCcWgWords, 0);
    auto col = [&](int ig, int iw) { return gax == 3 ? (size_t)(iw + n2 * ig) : (size_t)(ig + n2 * iw); };
    for (int ig = 0; ig < ngx; ++ig)
        for (int blk = 0; blk < nblk; ++blk) {
            // distinct group-axis cells of the block's columns, the window knots each needs
            int cg[kCcNCG], vmin[kCcNCG], vmax[kCcNCG], ncg = 0;
            for (int j = 0; j < kCcW; ++j) {
                const int iw = std::min(blk * kCcW + j, nwax - 1);
                const size_t c = col(ig, iw);
                const int ng = plan[c * kCsPlanWords] >> 8;
                for (int g = 0; g < ng; ++g) {
                    const int cgv = cells[(c * kCsGMax + g) * 2], wm = cells[(c * kCsGMax + g) * 2 + 1];
                    int ci = 0;
                    while (ci < ncg && cg[ci] != cgv) ++ci;
                    if (ci == ncg) {
                        if (ncg == CSh.ng) { h->cs_coop_why = 4; return HJB_OK; }
                        cg[ncg] = cgv; vmin[ncg] = wm; vmax[ncg] = wm + 2; ++ncg;
                    } else {
                        vmin[ci] = std::min(vmin[ci], wm);
                        vmax[ci] = std::max(vmax[ci], wm + 2);
                    }
                }
            }
            for (int ci = 0; ci < ncg; ++ci)
                if (vmax[ci] - vmin[ci] + 1 > kCcNV) { h->cs_coop_why = 5; return HJB_OK; }
            for (int j = 0; j < kCcW; ++j) {
                const int iw = blk * kCcW + j;
                if (iw >= nwax) break;
                const size_t c = col(ig, iw);
                for (int g = 0; g < kCsGMax; ++g) {         // padded groups repeat group 0's rows, like their global offsets
                    const int cgv = cells[(c * kCsGMax + g) * 2], wm = cells[(c * kCsGMax + g) * 2 + 1];
                    int ci = 0;
                    while (ci < ncg && cg[ci] != cgv) ++ci;
                    plan[c * kCsPlanWords + 1 + 2 * kCsGMax + g] = ((ci * 2) * kCcNV + (wm - vmin[ci])) * rowb;
                }
            }
            for (int chunk = 0; chunk < chunks; ++chunk) {
                int32_t *q = &wgw[((size_t)(ig * chunks + chunk) * nblk + blk) * kCcWgWords];
                int cmin = INT32_MAX, cmax = INT32_MIN;
                for (int j = 0; j < kCcW; ++j) {
                    const int iw = std::min(blk * kCcW + j, nwax - 1);
                    const int i2 = gax == 3 ? iw : ig, i3 = gax == 3 ? ig : iw;
                    for (int i0 = chunk * 64; i0 < std::min(n0, chunk * 64 + 64); ++i0) {
                        const int c0 = tab0[(size_t)(A0.sstride[0] * i0 + A0.sstride[2] * i2 + A0.sstride[3] * i3)].cell;
                        cmin = std::min(cmin, c0);
                        cmax = std::max(cmax, c0);
                    }
                }
                const int xlo = cmin / epl * epl;
                if (cmin < 0 || cmax + 1 - xlo > xw - 1) { h->cs_coop_why = 6; return HJB_OK; }
                q[0] = xlo;
                q[1] = ncg;
                for (int ci = 0; ci < ncg; ++ci) {
                    q[2 + ci] = (int32_t)(uint32_t)((P.jstride[gax] * (int64_t)cg[ci] + P.jstride[wax] * (int64_t)vmin[ci]) * (int64_t)h->esz);
                    q[2 + kCcNCG + ci] = std::min(kCcNV, nwk - vmin[ci]);
                }
            }
        }
    h->cs_coop_why = 0;
    h->cs_coop_epl = epl;
    return HJB_OK;
}

// The device copy of the column-sweep parameters, with the launch record at its head (kernels_colsweep.h CsRec): every
// scalar a wave reads before it knows its column, copied from the structures that own them.
static int colsweep_upload(Handle *h) {
    DColSweep &C = h->hcs;
    const DParams &P = h->hp;
    const DTabled &T = h->htb;
    uint32_t *r = C.rec;
    memset(r, 0, sizeof C.rec);
    auto put_ptr = [&](int i, const void *p) { const uint64_t v = (uint64_t)(uintptr_t)p; r[i] = (uint32_t)v; r[i + 1] = (uint32_t)(v >> 32); };
    for (int x = 0; x < 8; ++x) r[kRecXcdCnt + x] = (uint32_t)C.xcd_cnt[x];
    r[kRecN0] = (uint32_t)P.n[0]; r[kRecN1] = (uint32_t)P.n[1]; r[kRecN2] = (uint32_t)P.n[2]; r[kRecN3] = (uint32_t)P.n[3];
    r[kRecSplit] = (uint32_t)C.split; r[kRecWin] = (uint32_t)C.xcd_win; r[kRecXStride] = (uint32_t)C.xcd_stride; r[kRecNcu] = (uint32_t)C.ncu;
    put_ptr(kRecXcdIg, C.xcd_ig); put_ptr(kRecPlan, C.plan);
    put_ptr(kRecA0Tab, T.ax[0].tab); put_ptr(kRecA1Tab, T.ax[1].tab); put_ptr(kRecStatus, P.status);
    r[kRecGBytes] = C.g_bytes; r[kRecWBytes] = C.w_bytes; r[kRecS1Bytes] = C.s1_bytes;
    r[kRecNpreCol] = (uint32_t)C.npre_col; r[kRecNpre] = (uint32_t)P.n_cost_prefix; r[kRecStepUniform] = (uint32_t)C.step_uniform;
    r[kRecA0S0] = (uint32_t)T.ax[0].sstride[0]; r[kRecA0S2] = (uint32_t)T.ax[0].sstride[2]; r[kRecA0S3] = (uint32_t)T.ax[0].sstride[3];
    r[kRecA1S1] = (uint32_t)T.ax[1].sstride[1]; r[kRecA1S2] = (uint32_t)T.ax[1].sstride[2]; r[kRecA1S3] = (uint32_t)T.ax[1].sstride[3];
    r[kRecSlabBegin] = (uint32_t)P.slab_begin; r[kRecHaloLo] = (uint32_t)P.halo_lo;
    r[kRecJs1] = (uint32_t)P.jstride[1]; r[kRecJs2] = (uint32_t)P.jstride[2]; r[kRecJs3] = (uint32_t)P.jstride[3];
    r[kRecIndexBase] = (uint32_t)P.index_base; r[kRecIdxBytes] = (uint32_t)P.idx_bytes;
    // the cost record: up to three column-constant state terms (those before the first that depends on state dim 1) and the one
    // per-step term of the usual shape; a shape it cannot hold says so (n = -1 never equals npre_col) and the kernel reads DParams
    uint32_t *c = C.crec;
    memset(c, 0, sizeof C.crec);
    const bool holds = !h->cost64 && C.npre_col >= 0 && C.npre_col <= 3;
    c[kCRecNCol] = holds ? (uint32_t)C.npre_col : (uint32_t)-1;
    if (holds) {
        auto put_term = [&](int at, const DTerm &t, int sa, int sb, int sc) {
            const uint64_t v = (uint64_t)(uintptr_t)t.data;
            c[at] = (uint32_t)v; c[at + 1] = (uint32_t)(v >> 32);
            c[at + 2] = (uint32_t)t.stride[sa]; c[at + 3] = (uint32_t)t.stride[sb]; c[at + 4] = (uint32_t)t.stride[sc];
        };
        for (int j = 0; j < C.npre_col; ++j) put_term(kCRecTerm + 5 * j, P.cost[j], 0, 2, 3);
        if (C.step_uniform && P.n_cost_prefix - C.npre_col == 1) {
            c[kCRecHasSu] = 1;
            put_term(kCRecSu, P.cost[C.npre_col], 1, 2, 3);
        }
    }
    if (!h->dcs) return fail(h, HJB_E_DEVICE, "variant 7 parameters not allocated");
    HIP_TRY(h, hipMemcpy(h->dcs, &C, sizeof(DColSweep), hipMemcpyHostToDevice));
    return HJB_OK;
}

// Variant 7: in how many parts (waves) a column is swept (DColSweep::split).  Automatic: doubled while the launch stays
// within five times the chip's 6144 wave slots (6 waves per SIMD) and every part keeps >= 12 steps (a part starts by
// priming: about a step and a half of extra gathers).  Measured on one middle rank of an 8-GPU run of C4 (15 planes =
// 3600 columns, profiles/r02_rank_slab_timing.log): 1 / 2 / 4 / 8 parts -> 0.270 / 0.249 / 0.233 / 0.235 ms per stage;
// a boundary strip (240 columns) lasts 15 steps instead of 120.  Round 4, whole grids (launches far beyond the wave slots): parts of
// ~60 steps beat one long column by 1-2 % on every shape tried (120^4: 1 / 2 / 3 parts 1.674 / 1.640 / 1.647 ms; 160 steps: 1.551 /
// 1.527 / 1.516; 80 steps: equal; profiles/r04_c4_split.log) - so a column is also cut into round(n1 / 60) parts.
static void colsweep_split(Handle *h) {
    const DParams &P = h->hp;
    DColSweep &CSh = h->hcs;
    const int lanes = CSh.dpp ? kCsDppLanes : 64;
    const int64_t chunks = (P.n[0] + lanes - 1) / lanes;
    const int64_t waves = chunks * (int64_t)P.n[2] * (int64_t)P.n[3];
    const int n1 = P.n[1];
    int S = h->cs_split;
    if (S <= 0) {
        S = 1;
        // (five rounds of the 6144 wave slots at six waves per SIMD; rounds 2 - 3 said three rounds of 5120: a middle rank of a 4-GPU run of
        // C4 - 7200 columns - in 2 / 3 / 4 parts 0.430 / 0.419 / 0.416 ms fused, 0.456 / 0.440 / 0.438 with its strips beside the interior)
        while (S < 8 && waves * S * 2 <= 5 * 6144 && n1 / (S * 2) >= 12) S *= 2;
        // launches below one round of the wave slots (the reference's own 30x30x20x15 grid: 450 columns of 20 steps): parts as short as
        // five steps still pay - 31.3 / 18.7 / 12.8 us per stage in 1 / 2 / 4 parts (profiles/r04_small_grids.log)
        while (S < 8 && waves * S * 2 <= 4096 && n1 / (S * 2) >= 5) S *= 2;
        // round 5: with the one-round-trip prime and the batched set-up a part costs little to start, and such a launch is ONE wave's
        // critical path (5.6 us + 1.14 us per step on that grid): as many parts as fit three quarters of the wave slots, two steps
        // each at least - 17.0 / 11.3 / 10.6 -> 10.0 us per stage in 2 / 4 / 10 parts (profiles/r05_small_grids.log)
        if (waves * S <= 4608 && n1 >= 4 && n1 <= 40) S = (int)std::max<int64_t>(S, std::min<int64_t>(std::min<int64_t>(n1 / 2, 4608 / std::max<int64_t>(waves, 1)), 16));
        S = std::max(S, std::min(8, (n1 + 30) / 60));
    }
    CSh.split = std::max(1, std::min(S, std::max(1, n1)));
}

int ensure_colsweep(Handle *h) {
    using T = float;       // variant 7 is float32 arithmetic only
    if (h->cs_state >= 0) return HJB_OK;
    h->cs_state = 0;
    const DParams &P = h->hp;
    if (P.D != 4 || P.C != 1 || P.model || !h->tabled_ok || h->nU > kCsUMax) return HJB_OK;
    if (h->j_elems * (int64_t)h->esz >= ((int64_t)1 << 32) || h->n_owned >= ((int64_t)1 << 31)) return HJB_OK;
    const uint32_t cbit = 1u << 4;
    if ((h->dom_mask[0] & (cbit | 2u)) || (h->dom_mask[1] & (cbit | 1u)) || (h->dom_mask[2] & 3u) || (h->dom_mask[3] & 3u)) return HJB_OK;
    const int ncu = P.n_cost - P.n_cost_prefix;
    if (ncu > kCsMaxCu) return HJB_OK;
    for (int k = P.n_cost_prefix; k < P.n_cost; ++k)
        if (h->prob.cost_terms[k].mask != cbit) return HJB_OK;
    const int npre_col = first_term(h->prob.cost_terms, 0, P.n_cost_prefix, 2u);
    bool step_uniform = true;
    for (int k = npre_col; k < P.n_cost_prefix; ++k) step_uniform = step_uniform && (h->prob.cost_terms[k].mask & 1u) == 0;
    int st = ensure_tabled(h);
    if (st) return st;
    std::vector<TabEntry<T>> tab[2];
    for (int a = 2; a < 4; ++a) {
        tab[a - 2].resize((size_t)h->dom_entries[a]);
        HIP_TRY(h, hipMemcpy(tab[a - 2].data(), h->htb.ax[a].tab, tab[a - 2].size() * sizeof(TabEntry<T>), hipMemcpyDeviceToHost));
    }
    std::vector<std::vector<T>> cu((size_t)ncu, std::vector<T>((size_t)h->nU));
    for (int k = 0; k < ncu; ++k)
        HIP_TRY(h, hipMemcpy(cu[(size_t)k].data(), P.cost[P.n_cost_prefix + k].data, (size_t)h->nU * sizeof(T), hipMemcpyDeviceToHost));
    h->cs_cu64.clear();
    if (h->cost64 && ncu == 1) {       // the one control term in float64: a slot carries it in words 4, 5 (cost form 2)
        h->cs_cu64.resize((size_t)h->nU);
        HIP_TRY(h, hipMemcpy(h->cs_cu64.data(), P.cost64[P.n_cost_prefix].data, (size_t)h->nU * sizeof(double), hipMemcpyDeviceToHost));
    }
    // group by the axis that leaves fewer corner rows to load
    std::vector<int32_t> plan[2];
    int64_t rows[2] = {0, 0};
    int ngm[2] = {1, 1};
    std::vector<int32_t> cells[2];
    int mid[2] = {0, 0};
    const bool ok3 = colsweep_plan<T>(h, 3, tab, cu, plan[1], &rows[1], &ngm[1], cells[1], &mid[1]);
    const bool ok2 = colsweep_plan<T>(h, 2, tab, cu, plan[0], &rows[0], &ngm[0], cells[0], &mid[0]);
    if (!ok2 && !ok3) return HJB_OK;
    const int pick = (ok3 && (!ok2 || ngm[1] < ngm[0] || (ngm[1] == ngm[0] && rows[1] <= rows[0]))) ? 1 : 0;
    DColSweep &CSh = h->hcs;
    memset(&CSh, 0, sizeof CSh);
    CSh.gax = pick ? 3 : 2;
    CSh.ng = ngm[pick];
    h->cs_rows_mid = mid[pick];
    CSh.g_bytes = (uint32_t)(P.jstride[CSh.gax] * (int64_t)h->esz);
    CSh.w_bytes = (uint32_t)(P.jstride[5 - CSh.gax] * (int64_t)h->esz);
    {
        std::vector<int32_t> wgw;
        st = colcoop_plan<T>(h, plan[pick], cells[pick], wgw);      // fills the plans' staged-row offsets
        if (!st && h->cs_coop_epl) st = upload(h, wgw, &CSh.wg);
    }
    if (!st) st = upload(h, plan[pick], &CSh.plan);
    if (st) return st;
    CSh.npre_col = npre_col;
    CSh.step_uniform = step_uniform ? 1 : 0;
    CSh.ncu = ncu;
    CSh.s1_bytes = (uint32_t)(P.jstride[1] * (int64_t)h->esz);
    st = colsweep_map(h, plan[pick]);
    if (!st) st = colsweep_dpp_ok<T>(h, &h->cs_dpp_ok);
    if (!st) st = dev_alloc(h, sizeof(DColSweep), &h->dcs);
    if (!st) st = colsweep_options(h, false);
    if (st) return st;
    h->cs_state = 1;
    return HJB_OK;
}

// Variant 7's launch-time fields from the option values - the one-load (DPP) form (cs_dpp), the cooperative form (cs_coop), the parts a
// column is swept in (cs_split) and, with `remap`, the column -> XCD assignment (cs_xcd_axis, cs_xcd_mod) - uploaded with the launch
// record.  The caller chooses the launch again.
int colsweep_options(Handle *h, bool remap) {
    DColSweep &CSh = h->hcs;
    if (remap) {
        std::vector<int32_t> plan((size_t)h->hp.n[2] * h->hp.n[3] * kCsPlanWords);
        HIP_TRY(h, hipMemcpy(plan.data(), CSh.plan, plan.size() * 4, hipMemcpyDeviceToHost));
        const int st = colsweep_map(h, plan);
        if (st) return st;
    }
    CSh.dpp = (h->cs_dpp_ok && h->cs_dpp) ? 1 : 0;
    CSh.coop = h->cs_coop ? h->cs_coop_epl : 0;
    colsweep_split(h);
    return colsweep_upload(h);
}

bool colsweep_usual_cost(const Handle *h) { return h->hcs.ncu == 1 && h->hp.n_cost_prefix > 0; }

}  // namespace hjbhost
