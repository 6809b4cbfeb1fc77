// hjbdp_packed.hip - libhjbdp host side: the kernels that evaluate next-state terms themselves - variant 1's analysis (DNested),
// variants 2 / 4 (outer terms, axis tables, contraction mode), the DNested upload, and K15's set-up (kernels_uniwin.h).
#include "hjbdp_host.h"

namespace hjbhost {

// division by a launch constant as multiply-high + shifts (Granlund - Montgomery, exact for every 32-bit numerator)
static void magic(int64_t dd, uint32_t *m, int32_t *sh) {
    if (dd <= 1 || dd >= ((int64_t)1 << 31)) { *m = 0; *sh = -1; return; }      // 1: q = r; >= 2^31: the 64-bit-index modes do not use it
    const uint64_t d = (uint64_t)dd;
    int l = 0;
    while (((uint64_t)1 << l) < d) ++l;
    *m = (uint32_t)((((uint64_t)1 << 32) * (((uint64_t)1 << l) - d)) / d + 1);
    *sh = l - 1;
}

// Variant 1 (control-nested): its term split and eligibility.  Reads hp (axes and cost terms uploaded); writes hn, nested_ok, nested_fast,
// nested_lds.  elem_bytes: the size of the arithmetic type.
void analyse_nested(Handle *h, const hjb_problem *p, size_t elem_bytes) {
    const int D = p->D, C = p->C;
    const DParams &P = h->hp;
    DNested &N = h->hn;
    memset(&N, 0, sizeof N);
    for (int a = 0; a < D; ++a) magic(P.n[a], &N.div_m[a], &N.div_s[a]);
    magic(P.inner, &N.div_m_inner, &N.div_s_inner);
    const uint32_t in_bit = 1u << (D + C - 1);
    bool ok = !h->tab64;          // variants 1-4 evaluate next-state terms in the kernel, in the problem dtype
    for (int a = 0; a < D - 1; ++a)
        if (axis_mask(p, a) & in_bit) ok = false;
    const DAxis &axl = P.axis[D - 1];
    // the inner terms: from the first that depends on the innermost control on (prefix terms are summed per state anyway)
    const int ax_kin = std::max(first_term(p->next_terms[D - 1], 0, axl.n_terms, in_bit), axl.n_prefix);
    const int cost_kin = std::max(first_term(p->cost_terms, 0, P.n_cost, in_bit), P.n_cost_prefix);
    N.m_in = p->m[C - 1];
    N.nUo = (int32_t)(h->nU / p->m[C - 1]);
    N.ax_kin = ax_kin;
    N.cost_kin = cost_kin;
    N.n_ax_in = axl.n_terms - ax_kin;
    N.n_cost_in = P.n_cost - cost_kin;
    if (N.n_ax_in > kMaxInAx || N.n_cost_in > kMaxInCost) ok = false;
    int slots = 0;
    for (int s = 0; s < kMaxInner; ++s) { N.in[s].data = nullptr; N.in[s].stride_in = 0; N.in[s].lds_slot = -1; }
    if (ok) {
        for (int s = 0; s < N.n_ax_in; ++s) {
            const DTerm &t = axl.t[ax_kin + s];
            N.in[s].data = t.data;
            N.in[s].stride_in = t.stride[D + C - 1];
            if (p->next_terms[D - 1][ax_kin + s].mask == in_bit) { N.in[s].lds_slot = s; ++slots; }
        }
        for (int s = 0; s < N.n_cost_in; ++s) {
            const DTerm &t = P.cost[cost_kin + s];
            N.in[kMaxInAx + s].data = t.data;
            N.in[kMaxInAx + s].stride_in = t.stride[D + C - 1];
            if (p->cost_terms[cost_kin + s].mask == in_bit) { N.in[kMaxInAx + s].lds_slot = kMaxInAx + s; ++slots; }
        }
    }
    N.n_slots = slots;
    // loop levels (see DNested): o1 runs over control dim C-2, o0 over control dim 0 when C == 3
    N.m_o0 = (C == 3) ? p->m[0] : 1;
    N.m_o1 = (C >= 2) ? p->m[C - 2] : 1;
    magic(N.m_o1, &N.div_m_o1, &N.div_s_o1);
    const uint32_t o1_bit = (C >= 2) ? (1u << (D + C - 2)) : 0u;
    for (int a = 0; a < D; ++a)
        N.ax_l0[a] = first_term(p->next_terms[a], P.axis[a].n_prefix, (a == D - 1) ? ax_kin : P.axis[a].n_terms, o1_bit);
    N.cost_l0 = first_term(p->cost_terms, P.n_cost_prefix, cost_kin, o1_bit);
    h->nested_lds = ((size_t)2 * p->n[D - 1] + (size_t)kMaxInner * (N.m_in + 1)) * elem_bytes;
    h->nested_fast = ok && N.n_ax_in == 1 && N.n_cost_in == 1 && N.in[0].lds_slot >= 0 &&
                     N.in[kMaxInAx].lds_slot >= 0 && ax_kin > 0 && cost_kin > 0;
    if (h->nested_lds > 64 * 1024) ok = false;
    h->nested_ok = ok;
}

// The shape variants 2 / 4 start from.  Reads hp, hn, nested_ok, nested_fast; writes hn.ot[], packed_mode, packed_lds, packed2_lds.
void analyse_packed(Handle *h, const hjb_problem *p) {
    const int D = p->D, C = p->C;
    const DParams &P = h->hp;
    DNested &N = h->hn;
    const int ax_kin = N.ax_kin, cost_kin = N.cost_kin;
    h->packed_mode = 0;
    // variants 2/4: cost inner term must be a control-only table; the last axis' inner term is either a
    // control-only table b[u_in] (variants 2 and 4) or may also depend on the STATE (variant 4 only:
    // e.g. Solver_attitude.m:425  h*((J1-J2)/J3*X1V.*X2V + U3V/J3)), never on the outer controls
    const uint32_t outer_bits = ((1u << (D + C - 1)) - 1u) & ~((1u << D) - 1u);
    const bool cost_fast = N.n_cost_in == 1 && N.in[kMaxInAx].lds_slot >= 0 && cost_kin > 0;
    const bool ax_gen = N.n_ax_in == 1 && N.in[0].lds_slot < 0 && ax_kin > 0 &&
                        (p->next_terms[D - 1][ax_kin].mask & outer_bits) == 0;
    if (h->nested_ok && cost_fast && (h->nested_fast || ax_gen) && p->dtype != HJB_F64 && (h->j_elems < ((int64_t)1 << 31) || p->model) &&
        p->n[D - 1] >= 2) {
        bool pk = (ax_kin == P.axis[D - 1].n_prefix) && N.m_in <= kPackedMaxIn;   // last axis: state part + inner term only
        // canonical shape: last axis = state part + b[u_in]; <= 1 cost term per outer loop level;
        // outer axes may have any terms (their cells/weights are precomputed below)
        for (int i = 0; i < HJB_MAX_D + 2; ++i) { memset(&N.ot[i], 0, sizeof N.ot[i]); N.ot[i].lds_off = -1; }
        int32_t ot_floats = 0;
        auto fill = [&](DNested::DOuterTerm &o, const DTerm &t, uint32_t mask, bool first) {
            o.data = t.data;
            for (int a = 0; a < HJB_MAX_D; ++a) o.sstride[a] = a < D ? t.stride[a] : 0;
            o.c0 = (C == 3) ? t.stride[D + 0] : 0;
            o.c1 = (C == 3) ? t.stride[D + 1] : ((C == 2) ? t.stride[D + 0] : 0);
            o.present = 1;
            o.level = (C == 3 && !(mask & (1u << (D + 1)))) ? 0 : 1;
            o.first = first ? 1 : 0;
            o.lds_off = -1;
            o.lds_len = 0;
            if ((mask & ((1u << D) - 1u)) == 0) {      // control-only: stage the whole table in LDS
                o.lds_len = (int32_t)term_elems(p, mask);
                o.lds_off = ot_floats;
                ot_floats += o.lds_len;
            }
        };
        if (pk) {
            const int c0n = N.cost_l0 - P.n_cost_prefix, c1n = cost_kin - N.cost_l0;
            if (c0n > 1 || c1n > 1) pk = false;
            else {
                if (c0n == 1) {
                    fill(N.ot[HJB_MAX_D], P.cost[P.n_cost_prefix], p->cost_terms[P.n_cost_prefix].mask, P.n_cost_prefix == 0);
                    N.ot[HJB_MAX_D].level = 0;
                }
                if (c1n == 1) {
                    fill(N.ot[HJB_MAX_D + 1], P.cost[N.cost_l0], p->cost_terms[N.cost_l0].mask,
                         P.n_cost_prefix == 0 && c0n == 0);
                    N.ot[HJB_MAX_D + 1].level = 1;
                }
            }
        }
        h->packed_mode = pk ? (h->nested_fast ? 1 : 2) : 0;   // 2: general inner term -> variant 4 only
        h->packed_lds = (size_t)(N.m_in + 1) * 256 * 8 + (size_t)(N.m_in + 1) * 8 + (size_t)2 * p->n[D - 1] * 4 +
                        (size_t)ot_floats * 4;
        {
            const size_t np = (size_t)(N.m_in + 1) / 2;
            h->packed2_lds = (np + 1) * 256 * 8 + (np + 1) * 8 + (size_t)N.m_in * 4 + (size_t)2 * p->n[D - 1] * 4 +
                             (size_t)ot_floats * 4;
        }
        if (h->packed_lds > 64 * 1024) h->packed_mode = 0;
    }
}

// Modes 2 / 3 -> 5 / 6 (kernels_packed2.h W3P): three window planes instead of four serve when the inner control moves the last axis by
// less than its narrowest cell per control step - the second cell a sweep enters is then a neighbour of the first.  27 entries and no
// padding row in the weights: 40 KB per workgroup with 11 torque levels = four workgroups per CU instead of three.  (The kernel still
// checks every state.)  Variants 2 / 4 are float32 arithmetic: the term and the knots are read as the kernel sees them.
static bool window3_near(const Handle *h, const hjb_problem *p) {
    const DNested &N = h->hn;
    const int D = p->D;
    if (!(N.n_ax_in == 1 && p->table_dtype == HJB_TAB_DEFAULT)) return false;
    // the last axis' one inner term: (state dims of its mask) x the inner control, control slowest
    const hjb_term &bt = p->next_terms[D - 1][N.ax_kin];
    const int64_t per_ctrl = term_elems(p, bt.mask & ((1u << D) - 1u));
    const float *bj = (const float *)bt.data;
    double step = 0.0, width = 1e300;
    for (int j = 1; j < N.m_in; ++j)
        for (int64_t e = 0; e < per_ctrl; ++e)
            step = std::max(step, std::fabs((double)bj[e + j * per_ctrl] - (double)bj[e + (j - 1) * per_ctrl]));
    for (int i = 1; i < p->n[D - 1]; ++i)
        width = std::min(width, (double)(float)p->knots[D - 1][i] - (double)(float)p->knots[D - 1][i - 1]);
    return step < 0.99 * width;
}

// Variant 4's contraction mode (kernels_packed2.h MODE) from the levels of the axis tables -> packed_pre, window3_ok, hn.chunk_order,
// packed2_lds.  Axis 0 stays without a table (axis0_inline) only in mode 1: any other outcome builds it here.
static int choose_packed_mode(Handle *h, const hjb_problem *p) {
    const int D = p->D, C = p->C;
    const DNested &N = h->hn;
    h->packed_pre = 0;
    // modes 1-3 read the level cost terms from LDS only
    const bool cl_lds = (!N.ot[HJB_MAX_D].present || N.ot[HJB_MAX_D].lds_off >= 0) &&
                        (!N.ot[HJB_MAX_D + 1].present || N.ot[HJB_MAX_D + 1].lds_off >= 0);
    if (cl_lds && C == 3 && D == 3 && N.at[0].level == 0 && N.at[1].level == 1) h->packed_pre = 1;
    const int st4 = h->packed_pre != 1 ? ensure_axis0_table(h) : HJB_OK;     // mode 1 did not come about after all: the table is needed
    if (st4) return st4;
    if (h->axis0_inline) h->packed_pre = 4;          // mode 1 without the axis-0 table (kernels_packed2.h MODE 4)
    if (cl_lds && C == 3 && D >= 4 && N.at[D - 3].level == 0 && N.at[D - 2].level == 1) {
        bool pre = true;
        for (int a = 0; a < D - 3; ++a) pre = pre && N.at[a].level < 0;
        if (pre && h->packed2_lds + 36 * 256 * 4 <= 64 * 1024) {
            h->packed_pre = p->model ? 3 : 2;
            const bool near = window3_near(h, p);
            h->window3_ok = near;
            {   // visiting order of the 256-state chunks (kernels_packed2.h, option "chunk_order"): when the window slices
                // of ONE point of the level axes - the whole block of the state-only axes x 27 / 36 entries - outgrow an
                // XCD's 4 MiB L2, neighbouring chunks of that block must run together (state order); smaller blocks gain
                // more from the neighbouring points' shared window rows (transposed order).  C3: 51^3 x 27 x 4 B = 14 MB.
                int64_t blk = 1;
                for (int a = 0; a + 3 < D; ++a) blk *= p->n[a];
                h->hn.chunk_order = blk * (int64_t)h->esz * (near ? 27 : 36) > ((int64_t)4 << 20) ? 1 : 0;
            }
            if (near) {
                h->packed_pre += 3;                                        // modes 5 / 6
                h->packed2_lds += 27 * 256 * 4;
                h->packed2_lds -= 256 * 8;                                 // no padding row in the weights
            } else {
                h->packed2_lds += 36 * 256 * 4;   // the per-state window
            }
        }
    }
    return HJB_OK;
}

// Variants 2 / 4: the stage-invariant (cell, weight) tables of the outer axes over their domains, then the contraction mode.  Reads
// packed_mode, hp, dp; writes hn.at[], axis0_inline / axis0_dom / axis0_nent, preps, and what choose_packed_mode does.
int build_packed_tables(Handle *h, const hjb_problem *p) {
    if (!h->packed_mode) return HJB_OK;
    const int D = p->D, C = p->C;
    AxisDomain dom[HJB_MAX_D];
    size_t total = 0;
    bool fits = true;
    for (int a = 0; a < D - 1; ++a) {
        dom[a] = axis_domain(h, axis_mask(p, a));
        if (dom[a].entries >= ((int64_t)1 << 31)) fits = false;
        total += (size_t)dom[a].entries * sizeof(int2);
    }
    if (!fits || total > ((size_t)24 << 30)) {
        h->packed_mode = 0;   // tables too large: variant 1 evaluates on the fly
        return HJB_OK;
    }
    for (int a = 0; a < D - 1; ++a) {
        DNested::DAxisTable &A = h->hn.at[a];
        memset(&A, 0, sizeof A);
        for (int d = 0; d < D; ++d) A.sstride[d] = dom[a].stride[d];
        A.c0 = (C == 3) ? dom[a].stride[D + 0] : 0;
        A.c1 = (C == 3) ? dom[a].stride[D + 1] : ((C == 2) ? dom[a].stride[D + 0] : 0);
        const bool has_o1 = (C >= 2) && dom[a].has(D + C - 2);
        const bool has_o0 = (C == 3) && dom[a].has(D);
        A.level = has_o1 ? 1 : (has_o0 ? 0 : -1);
        if (p->n_next_terms[a] == 0) continue;     // model axis: evaluated in the stage kernel
        // The C2 shape (mode 1 below: D = 3, three control dims, axis 0 moves with control dim 0, axis 1 with
        // control dim 1): when axis 0's next value is (state-only terms) + ONE term over control dim 0 alone, the
        // stage kernel forms its (cell, t) from q in registers - same ordered sum, same exact search - and the
        // table (8 bytes per state and o0 step: 173 MB on C2, streamed every stage) is not built at all
        if (a == 0 && D == 3 && C == 3 && has_o0 && !has_o1 && h->inline_axis0 &&
            p->n_next_terms[0] == h->hp.axis[0].n_prefix + 1 && p->next_terms[0][p->n_next_terms[0] - 1].mask == (1u << D)) {
            const uint32_t m1 = axis_mask(p, 1);
            if ((m1 & (1u << (D + 1))) && !(m1 & (1u << D))) {       // A.tab stays null
                h->axis0_inline = true;
                h->axis0_dom = dom[0].mask;
                h->axis0_nent = dom[0].entries;
                continue;
            }
        }
        const int st3 = build_axis_table(h, a, dom[a], false);
        if (st3) return st3;
    }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, sync_setup());
    return choose_packed_mode(h, p);
}

// hn -> dn, for the kernels that read it (variants 1, 2, 4)
int upload_nested(Handle *h) {
    if (!h->nested_ok) return HJB_OK;
    const int st2 = dev_alloc(h, sizeof(DNested), &h->dn);
    if (st2) return st2;
    HIP_TRY(h, hipMemcpy(h->dn, &h->hn, sizeof(DNested), hipMemcpyHostToDevice));
    return HJB_OK;
}

// ---- K15 (kernels_uniwin.h): variant 4's three-plane window modes on chunks that share their rate axes -------------------
// Applies when, beyond modes 5 / 6, nothing the level axes and the last axis need depends on the state-only axes: their tables'
// domains, the last axis' state terms and its inner term (Solver_attitude.m:423-425: the next rates are functions of the rates
// and the torque).  The plan is built here; `uniwin_auto` says whether the usual shape holds on (nearly) every point.
static size_t uniwin_lds(const DNested &N, int block) {      // the window of 27 planes per state and the level cost terms staged in LDS
    size_t ot_floats = 0;
    for (int i = HJB_MAX_D; i < HJB_MAX_D + 2; ++i)
        if (N.ot[i].present) ot_floats = std::max<size_t>(ot_floats, (size_t)N.ot[i].lds_off + (size_t)N.ot[i].lds_len);
    return (size_t)27 * block * 4 + ot_floats * 4 + 16;
}

// The chunk walk's tiling and workgroup size from the options (uw_tile, uw_block) -> Handle::huw, Handle::uw_lds.
static void uniwin_tiles(Handle *h) {
    DUniwin &U = h->huw;
    U.block = h->uw_block == 64 ? 64 : 256;
    U.cpp = (int32_t)((U.inner + U.block - 1) / U.block);
    h->uw_lds = uniwin_lds(h->hn, U.block);
    auto lg = [](int n, int most) { int l = 0; while (l < most && (1 << l) < n) ++l; return l; };
    int lA = 3, lB = 2, lC = 2;
    if (h->uw_tile > 0) { lA = h->uw_tile & 7; lB = (h->uw_tile >> 3) & 7; lC = (h->uw_tile >> 6) & 7; }
    U.lA = lg(U.nA, lA);
    U.lB = lg(U.nB, lB);
    U.lC = lg(U.nC, lC);
    U.ntA = (U.nA + (1 << U.lA) - 1) >> U.lA;
    U.ntB = (U.nB + (1 << U.lB) - 1) >> U.lB;
    U.ntC = (U.nC + (1 << U.lC) - 1) >> U.lC;
    U.tile_chunks = (uint32_t)U.cpp << (U.lA + U.lB + U.lC);
    const uint64_t nv = (uint64_t)U.tile_chunks * (uint64_t)U.ntA * (uint64_t)U.ntB * (uint64_t)U.ntC;
    U.n_v = (uint32_t)std::min<uint64_t>(nv, 0xfffffff0u);
}

// Handle::huw -> the kUwSets + 1 device copies (Handle::duw); the device is idle (hjb_create) or has been synchronised
static int uniwin_upload(Handle *h) {
    DUniwin sets[kUwSets + 1];
    for (int k = 0; k <= kUwSets; ++k) {
        sets[k] = h->huw;
        sets[k].counters = (h->uw_claim && k < kUwSets) ? h->huw.counters + (size_t)kUwSetWords * k : nullptr;
    }
    HIP_TRY(h, hipMemcpy(h->duw, sets, sizeof sets, hipMemcpyHostToDevice));
    return HJB_OK;
}

int uniwin_options(Handle *h) {
    uniwin_tiles(h);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());
    return uniwin_upload(h);
}

int setup_uniwin(Handle *h, const hjb_problem *p) {
    const DParams &P = h->hp;
    const DNested &N = h->hn;
    const int D = p->D, C = p->C;
    h->uniwin_ok = h->uniwin_auto = false;
    if (!(h->packed_mode && (h->packed_pre == 5 || h->packed_pre == 6)) || !h->dn) return HJB_OK;
    if (C != 3 || D < 4 || D > 6) return HJB_OK;
    if (!(N.m_in == kUwIn || N.m_in == kUwIn - 1) || N.m_o0 > kUwMaxO || N.m_o1 > kUwMaxO) return HJB_OK;
    const int NP = D - 3, AX_A = D - 3, AX_B = D - 2;
    const uint32_t so_bits = (1u << NP) - 1u;             // the state-only dims
    for (int d = 0; d < NP; ++d)
        if (N.at[AX_A].sstride[d] != 0 || N.at[AX_B].sstride[d] != 0) return HJB_OK;
    if (N.at[AX_B].c0 != 0 || !N.at[AX_A].tab || !N.at[AX_B].tab) return HJB_OK;
    for (int k = 0; k <= N.ax_kin && k < p->n_next_terms[D - 1]; ++k)
        if (p->next_terms[D - 1][k].mask & so_bits) return HJB_OK;
    if (N.n_ax_in != 1 || N.n_cost_in != 1 || N.in[kMaxInAx].lds_slot < 0) return HJB_OK;
    int64_t inner = 1;
    for (int a = 0; a < NP; ++a) inner *= p->n[a];
    const int64_t n_points = h->n_owned / inner;
    if (inner < 128 || inner >= ((int64_t)1 << 30) || n_points >= ((int64_t)1 << 24) || h->inner >= ((int64_t)1 << 31)) return HJB_OK;
    for (int i = HJB_MAX_D; i < HJB_MAX_D + 2; ++i)
        if (N.ot[i].present && N.ot[i].lds_off < 0) return HJB_OK;
    if (uniwin_lds(N, 256) > 64 * 1024) return HJB_OK;
    DUniwin &U = h->huw;
    memset(&U, 0, sizeof U);
    U.n_points = (int32_t)n_points;
    U.inner = (int32_t)inner;
    U.nA = p->n[AX_A];
    U.nB = p->n[AX_B];
    U.nC = P.n[D - 1];                                     // owned planes
    U.cl1_per_o0 = (N.ot[HJB_MAX_D + 1].present && N.ot[HJB_MAX_D + 1].c0 != 0) ? 1 : 0;
    if ((int64_t)U.nA * U.nB * U.nC != n_points) return HJB_OK;
    int32_t *plan = nullptr, *cnt = nullptr;
    int st = dev_alloc(h, (size_t)n_points * kUwRec * sizeof(int32_t), &plan);
    if (!st) st = dev_alloc(h, sizeof(int32_t), &cnt);
    if (st) return st;
    HIP_TRY(h, hipMemset(cnt, 0, sizeof(int32_t)));
    if (stage_uniwin_plan(D, h->dp, h->dn, plan, (int)n_points, U.nA, U.nB, cnt)) return HJB_OK;
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, sync_setup());
    int32_t n_slow = 0;
    HIP_TRY(h, hipMemcpy(&n_slow, cnt, sizeof n_slow, hipMemcpyDeviceToHost));
    h->uniwin_slow = n_slow;
    U.plan = plan;
    // the per-XCD claim counters of the chunk walk (kernels_uniwin.h): 8 x one 64-byte line per stream, zeroed before every launch
    st = dev_alloc(h, (size_t)kUwSets * kUwSetWords * sizeof(uint32_t), &U.counters);
    if (st) return st;
    HIP_TRY(h, hipMemset(U.counters, 0, (size_t)kUwSets * kUwSetWords * sizeof(uint32_t)));
    uniwin_tiles(h);
    st = dev_alloc(h, (kUwSets + 1) * sizeof(DUniwin), &h->duw);
    if (!st) st = uniwin_upload(h);
    if (st) return st;
    h->uniwin_ok = true;
    h->uniwin_auto = (int64_t)n_slow * 50 <= n_points;     // at most 2 % of the points on the slow path
    return HJB_OK;
}

}  // namespace hjbhost
