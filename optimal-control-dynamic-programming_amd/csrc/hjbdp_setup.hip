// hjbdp_setup.hip - libhjbdp host side: the process-wide state, device allocation, the problem upload and hjb_create's work as a list
// of steps (build_handle); the work buffers, the status word and the probe block.
// gfx950 (MI355X) only; no CPU fallback - without a HIP device every compute entry point returns HJB_E_DEVICE.
#include "hjbdp_host.h"

namespace hjbhost {

thread_local std::string g_last_error;
std::atomic<int> g_test_fail_tab64_scratch{0};
std::atomic<int> g_test_fail_tabled_alloc{0};
std::atomic<int> g_test_rccl_only_env{0};
std::atomic<int> g_test_fail_graph_capture{0};
std::shared_mutex g_capture_mu;

int fail(Handle *h, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    g_last_error = buf;
    return code;
}

// Every device allocation of a handle.  Small ones (plans, tables, cost terms, records: dozens per handle) are carved out of 1 MiB
// chunks: hipMalloc / hipFree cost 50 - 200 us each and hipFree waits for the device, which was 8 of the 64 ms of a whole
// Solver_pos_att.simplified_run (four handles; profiles/r06_batch_split.log, block 3).  256-byte aligned (the widest access of the
// kernels is 64 bytes: s_load_dwordx16 of a launch record).
int dev_alloc(Handle *h, size_t bytes, void **out) {
    constexpr size_t kChunk = (size_t)1 << 20, kSmall = (size_t)128 << 10, kAlign = 256;
    bytes = std::max<size_t>(bytes, 16);
    if (bytes <= kSmall) {
        const size_t need = (bytes + kAlign - 1) & ~(kAlign - 1);
        if (h->arena_left < need) {
            void *c = nullptr;
            HIP_TRY(h, hipMalloc(&c, kChunk));
            h->allocs.push_back(c);
            h->arena = (char *)c;
            h->arena_left = kChunk;
        }
        *out = h->arena;
        h->arena += need;
        h->arena_left -= need;
        return HJB_OK;
    }
    void *d = nullptr;
    HIP_TRY(h, hipMalloc(&d, bytes));
    h->allocs.push_back(d);
    *out = d;
    return HJB_OK;
}

SweepScratch::~SweepScratch() {
    HoldUnlessHeld hold(held);
    if (gexec) (void)hipGraphExecDestroy(gexec);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    for (void *d : bufs) (void)hipFree(d);
}

void SweepScratch::drop_graph() {
    HoldUnlessHeld hold(held);
    if (gexec) (void)hipGraphExecDestroy(gexec);
    gexec = nullptr;
}

int capture_stage_loop(Handle *h, hipStream_t stream, const std::function<int()> &body, hipGraphExec_t *out) {
    if (g_test_fail_graph_capture.load()) return fail(h, HJB_E_DEVICE, "stage-loop graph capture failed (test hook)");
    std::unique_lock<std::shared_mutex> capture_lk(g_capture_mu);
    HIP_TRY(h, hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    const int cst = body();
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    hipError_t ce = hipStreamEndCapture(stream, &graph);
    int st = HJB_OK;
    if (cst != HJB_OK || ce != hipSuccess) st = fail(h, HJB_E_DEVICE, "stage-loop graph capture failed: %s", hipGetErrorString(ce));
    else if ((ce = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0)) != hipSuccess) st = fail(h, HJB_E_DEVICE, "hipGraphInstantiate: %s", hipGetErrorString(ce));
    if (graph) (void)hipGraphDestroy(graph);
    if (!st) *out = exec;
    return st;
}

int64_t term_elems(const hjb_problem *p, uint32_t mask) {
    int64_t s = 1;
    for (int d = 0; d < p->D + p->C; ++d)
        if (mask & (1u << d)) {
            const int64_t k = (d < p->D) ? p->n[d] : p->m[d - p->D];
            if (k < 1 || s > (INT64_MAX >> 1) / k) return INT64_MAX;      // saturates: every caller compares with a limit
            s *= k;
        }
    return s;
}

// upload one term, fill strides
template <typename T, typename TS = T>      // T: element type on the device, TS: element type of the caller's array
int make_term(Handle *h, const hjb_problem *p, const hjb_term &t, DTerm *out) {
    const int64_t s = term_elems(p, t.mask);
    for (int d = 0; d < HJB_MAX_G; ++d)      // dense, column-major over the dims of the mask: a dim's stride is the extent of those below it
        out->stride[d] = (d < p->D + p->C && (t.mask & (1u << d))) ? (int32_t)term_elems(p, t.mask & ((1u << d) - 1u)) : 0;
    std::vector<T> host((size_t)s);
    for (int64_t i = 0; i < s; ++i) host[(size_t)i] = (T)((const TS *)t.data)[i];
    out->pad = 0;
    return upload(h, host, &out->data);
}

// conservative range of an ordered term sum for a fixed index along `dim`
// (used for the halo the last axis needs)
template <typename T>
void term_minmax_along(const hjb_problem *p, const hjb_term &t, int dim, std::vector<double> &lo, std::vector<double> &hi) {
    const int nd = p->n[dim];
    std::vector<double> tlo(nd, INFINITY), thi(nd, -INFINITY);
    const int64_t total = term_elems(p, t.mask), stride_dim = term_elems(p, t.mask & ((1u << dim) - 1u));
    const T *data = (const T *)t.data;
    if (!(t.mask & (1u << dim))) {
        double mn = INFINITY, mx = -INFINITY;
        for (int64_t i = 0; i < total; ++i) { mn = std::min(mn, (double)data[i]); mx = std::max(mx, (double)data[i]); }
        for (int i = 0; i < nd; ++i) { tlo[i] = mn; thi[i] = mx; }
    } else {
        for (int64_t i = 0; i < total; ++i) {
            int id = (int)((i / stride_dim) % nd);
            tlo[id] = std::min(tlo[id], (double)data[i]);
            thi[id] = std::max(thi[id], (double)data[i]);
        }
    }
    for (int i = 0; i < nd; ++i) { lo[i] += tlo[i]; hi[i] += thi[i]; }
}

// The halo (planes of the last axis a slab must see beyond the ones it owns) implied by the last axis' next-state terms:
// host arithmetic only, conservative.  Shared by build() and by the partitioners (hjb_create_multi, hjb_rank_create),
// which must not build a whole-grid handle just to learn two integers.
template <typename T>
void halo_from_terms(const hjb_problem *p, bool tab64, int *out_lo, int *out_hi) {
    const int a = p->D - 1, n = p->n[a];
    std::vector<double> lo(n, 0.0), hi(n, 0.0);
    for (int k = 0; k < p->n_next_terms[a]; ++k) {
        if (tab64) term_minmax_along<double>(p, p->next_terms[a][k], a, lo, hi);
        else term_minmax_along<T>(p, p->next_terms[a][k], a, lo, hi);
    }
    std::vector<T> kk(n);
    for (int i = 0; i < n; ++i) kk[i] = (T)p->knots[a][i];
    auto cell_of = [&](double q) {
        int c = (int)(std::upper_bound(kk.begin(), kk.end(), (T)q) - kk.begin()) - 1;
        return std::min(std::max(c, 0), n - 2);
    };
    int need_lo = 0, need_hi = 0;
    for (int i = 0; i < n; ++i) {
        // small relative slack: the sum of per-term extrema is formed in double
        double span = std::fabs(hi[i]) + std::fabs(lo[i]);
        int clo = cell_of(lo[i] - 1e-6 * span), chi = cell_of(hi[i] + 1e-6 * span);
        need_lo = std::max(need_lo, i - clo);
        need_hi = std::max(need_hi, chi + 1 - i);
    }
    *out_lo = need_lo;
    *out_hi = need_hi;
}

// hjb_create's steps of this unit (build, below, lists them all): each reads the problem and writes the handle fields its comment names.
// slab, strides, owned states, controls -> hp (cleared first), plane0, nplanes, j_elems, inner, n_owned, nU
static void set_geometry(Handle *h, const hjb_problem *p) {
    const int D = p->D, C = p->C;
    DParams &P = h->hp;
    memset(&P, 0, sizeof P);
    P.D = D;
    P.C = C;
    int sb = p->slab_begin, se = p->slab_end, hlo = p->halo_lo, hhi = p->halo_hi;
    if (sb == 0 && se == 0) { se = p->n[D - 1]; hlo = hhi = 0; }
    h->plane0 = sb - hlo;
    h->nplanes = (se + hhi) - h->plane0;
    int64_t s = 1, inner = 1;
    for (int a = 0; a < D; ++a) {
        P.n[a] = (a == D - 1) ? (se - sb) : p->n[a];
        P.jstride[a] = s;
        s *= (a == D - 1) ? h->nplanes : p->n[a];
        if (a < D - 1) inner *= p->n[a];
    }
    h->j_elems = s;
    h->inner = inner;
    h->n_owned = inner * (se - sb);
    h->nU = 1;
    for (int c = 0; c < C; ++c) { P.m[c] = p->m[c]; h->nU *= p->m[c]; }
    for (int c = C; c < HJB_MAX_C; ++c) P.m[c] = 1;
    P.n_owned = h->n_owned;
    P.nU = h->nU;
    P.inner = inner;
    P.plane0 = h->plane0;
    P.nplanes = h->nplanes;
    P.slab_begin = sb;
    P.halo_lo = hlo;
    P.index_base = p->index_base;
    P.idx_bytes = h->idx_bytes;
}

// Every axis in TK - knots, 1/dx, the uniformity test, x0 and 1/h, the next-state terms - uploaded -> P->axis[].  The working-dtype
// axes (hp) round the caller's knots to TK and refuse those that do not stay increasing (`check`); the float64 shadow takes them as given.
template <typename TK>
static int upload_axes(Handle *h, const hjb_problem *p, DParams *P, bool check) {
    const uint32_t state_mask = (1u << p->D) - 1u;
    for (int a = 0; a < p->D; ++a) {
        DAxis &ax = P->axis[a];
        const int n = p->n[a];
        std::vector<TK> kk(n), rdx(n);
        for (int i = 0; i < n; ++i) kk[i] = (TK)p->knots[a][i];
        for (int i = 0; i + 1 < n; ++i) {
            if (check && !(kk[i + 1] > kk[i]))
                return fail(h, HJB_E_INVALID, "knots of axis %d are not strictly increasing in the working dtype at %d", a, i);
            rdx[i] = (TK)1 / (TK)(kk[i + 1] - kk[i]);
        }
        rdx[n - 1] = (TK)0;
        int st = upload(h, kk, &ax.knots);
        if (!st) st = upload(h, rdx, &ax.rdx);
        if (st) return st;
        ax.n = n;
        const double hstep = ((double)kk[n - 1] - (double)kk[0]) / (n - 1);
        double dev = 0;
        for (int i = 0; i < n; ++i) dev = std::max(dev, std::fabs((double)kk[i] - ((double)kk[0] + i * hstep)));
        ax.uniform = dev <= 1.5 * hstep ? 1 : 0;
        ax.x0 = (double)kk[0];
        ax.inv_h = 1.0 / hstep;
        ax.n_terms = p->n_next_terms[a];
        ax.n_prefix = first_term(p->next_terms[a], 0, ax.n_terms, ~state_mask);
        for (int k = 0; k < ax.n_terms; ++k) {
            // table_dtype F64: the caller's next-state terms are float64.  The float32 copy made of them serves the host-side
            // structure analysis only (no stage kernel that evaluates terms is admitted); the tables come from the float64 shadow
            st = h->tab64 ? make_term<TK, double>(h, p, p->next_terms[a][k], &ax.t[k]) : make_term<TK>(h, p, p->next_terms[a][k], &ax.t[k]);
            if (st) return st;
        }
    }
    return HJB_OK;
}

// cost terms (cost_dtype F64: and their float64 copy) -> hp.cost[], hp.cost64[], n_cost, n_cost_prefix, cost_f64
template <typename T>
static int upload_cost(Handle *h, const hjb_problem *p) {
    DParams &P = h->hp;
    const uint32_t state_mask = (1u << p->D) - 1u;
    P.n_cost = p->n_cost_terms;
    P.n_cost_prefix = first_term(p->cost_terms, 0, P.n_cost, ~state_mask);
    P.cost_f64 = h->cost64 ? 1 : 0;
    for (int k = 0; k < P.n_cost; ++k) {
        // cost_dtype F64: the caller's cost terms are float64.  The float32 copy serves the host-side structure analysis
        // only (no stage kernel that sums the cost in float32 is admitted); the kernels read the float64 copy
        int st = h->cost64 ? make_term<T, double>(h, p, p->cost_terms[k], &P.cost[k]) : make_term<T>(h, p, p->cost_terms[k], &P.cost[k]);
        if (!st && h->cost64) st = make_term<double, double>(h, p, p->cost_terms[k], &P.cost64[k]);
        if (st) return st;
    }
    return HJB_OK;
}

// the state model and its quaternion tables -> hp.model, model_h, model_tab[]
static int upload_model(Handle *h, const hjb_problem *p) {
    DParams &P = h->hp;
    P.model = p->model;
    P.model_h = (float)p->model_h;
    if (p->model == HJB_MODEL_QUAT_EULER321) {
        const size_t ne = (size_t)p->n[0] * p->n[1] * p->n[2];
        for (int i = 0; i < 4; ++i) {
            std::vector<float> v((const float *)p->model_tables[i], (const float *)p->model_tables[i] + ne);
            const int st = upload(h, v, &P.model_tab[i]);
            if (st) return st;
        }
    }
    return HJB_OK;
}

// the status words and hp -> d_status, dp; table_dtype F64: the axes once more, in float64 -> dp64
static int upload_params(Handle *h, const hjb_problem *p) {
    DParams &P = h->hp;
    int st = dev_alloc(h, 2 * sizeof(int32_t), &h->d_status);
    if (st) return st;
    HIP_TRY(h, hipMemset(h->d_status, 0, 2 * sizeof(int32_t)));
    P.status = h->d_status;
    st = dev_alloc(h, sizeof(DParams), &h->dp);
    if (st) return st;
    HIP_TRY(h, hipMemcpy(h->dp, &P, sizeof(DParams), hipMemcpyHostToDevice));
    if (!h->tab64) return HJB_OK;
    // float64 shadow of the axes for the table build (k_prep_axis_table_t<double>): knots as given, 1/dx and the
    // next-state terms in double - what griddedInterpolant sees in Solver_pos_att.m:299-327 (double grid vectors,
    // double query tables); the stage kernels never read it
    DParams Q = P;
    st = upload_axes<double>(h, p, &Q, false);
    if (!st) st = dev_alloc(h, sizeof(DParams), &h->dp64);
    if (st) return st;
    HIP_TRY(h, hipMemcpy(h->dp64, &Q, sizeof(DParams), hipMemcpyHostToDevice));
    return HJB_OK;
}

// what no kernel serves is refused here (the first refusal that applies wins); a state model leaves variant 4 alone
static int refuse_unserved(Handle *h, const hjb_problem *p) {
    if (p->model) {
        if (!(h->packed_mode && (h->packed_pre == 3 || h->packed_pre == 6)))
            return fail(h, HJB_E_UNSUPPORTED,
                        "HJB_MODEL_QUAT_EULER321 needs the canonical attitude structure: axis 3 driven by control dim 0, "
                        "axis 4 by control dim 1, axis 5 by control dim 2 (kernels_packed2.h mode 3)");
        h->tabled_ok = false;     // the other stage kernels do not evaluate the model
        h->nested_fast = false;
    }
    if (h->cost64 && !h->tabled_ok)
        return fail(h, HJB_E_UNSUPPORTED, "cost_dtype HJB_COST_F64 is served by the table-driven kernels (variants 5, 7): this grid's per-axis "
                    "(cell, weight) tables do not fit - pass the cost terms in float32 (cost_dtype HJB_COST_DEFAULT)");
    if (h->tab64 && !h->tabled_ok)
        return fail(h, HJB_E_UNSUPPORTED, "table_dtype HJB_TAB_F64 needs the per-axis (cell, weight) tables to fit (variants 5-7): this grid's tables do not - "
                    "pass table_dtype = HJB_TAB_DEFAULT (Python mirrors: table_dtype=None) to run it on float32 queries");
    return HJB_OK;
}

// hjb_create's work on a validated problem, in the order its effects are observable in (uploads and table builds against
// sync_setup(), the registration order of the tables in Handle::preps); T: the arithmetic type
template <typename T>
static int build(Handle *h, const hjb_problem *p) {
    set_geometry(h, p);
    int st = upload_axes<T>(h, p, &h->hp, true);
    if (!st) st = upload_cost<T>(h, p);
    if (!st) st = upload_model(h, p);
    if (st) return st;
    halo_from_terms<T>(p, h->tab64, &h->halo_need_lo, &h->halo_need_hi);      // conservative halo implied by the tables of the last axis
    analyse_nested(h, p, sizeof(T));                      // variant 1
    analyse_packed(h, p);                                 // variants 2 / 4: the shape they start from
    st = upload_params(h, p);
    if (!st) st = build_packed_tables(h, p);              // variants 2 / 4: axis tables, contraction mode
    if (st) return st;
    analyse_tabled(h, p, sizeof(TabEntry<T>));            // variants 5 / 6
    st = refuse_unserved(h, p);
    if (!st) st = upload_nested(h);
    if (!st) st = setup_uniwin(h, p);                     // K15
    return st;
}

int build_handle(Handle *h, const hjb_problem *p) {
    return p->dtype != HJB_F64 ? build<float>(h, p) : build<double>(h, p);
}

void halo_of_problem(const hjb_problem *p, bool tab64, int *lo, int *hi) {
    if (p->dtype != HJB_F64) halo_from_terms<float>(p, tab64, lo, hi);
    else halo_from_terms<double>(p, tab64, lo, hi);
}

int ensure_work(Handle *h) {
    if (h->dJ[0]) return HJB_OK;
    for (int i = 0; i < 2; ++i) {
        int st = dev_alloc(h, (size_t)h->j_elems * h->esz, &h->dJ[i]);
        if (st) return st;
        HIP_TRY(h, hipMemset(h->dJ[i], 0, (size_t)h->j_elems * h->esz));
    }
    int st = dev_alloc(h, (size_t)h->n_owned * h->idx_bytes, &h->d_idx);
    if (!st) st = dev_alloc(h, sizeof(double) * 2 * kReduceBlocks, &h->d_partials);
    if (!st) st = dev_alloc(h, sizeof(double) * 2, &h->d_sums);
    return st;
}

// The two status words, read in one copy.  A left slab is reported first (and alone cleared: a bad label met by the evaluation kernel
// is then reported by the next call); each flag is cleared when it is reported.
int check_status(Handle *h, hipStream_t st) {
    int32_t flag[2] = {0, 0};
    HIP_TRY(h, hipMemcpyAsync(flag, h->d_status, sizeof flag, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    if (flag[0]) {
        HIP_TRY(h, hipMemsetAsync(h->d_status, 0, sizeof(int32_t), st));
        return fail(h, HJB_E_HALO, "a next-state query left the slab's halo (halo_lo=%d halo_hi=%d; tables imply lo=%d hi=%d)",
                    h->hp.halo_lo, h->nplanes - h->hp.n[h->hp.D - 1] - h->hp.halo_lo, h->halo_need_lo, h->halo_need_hi);
    }
    if (flag[1]) {
        HIP_TRY(h, hipMemsetAsync(h->d_status + 1, 0, sizeof(int32_t), st));
        return fail(h, HJB_E_INVALID, "hjb_evaluate_stage_device met a label outside [%d, %lld): NaN was stored for those states",
                    h->hp.index_base, (long long)(h->hp.index_base + h->nU));
    }
    return HJB_OK;
}

// ---- probe block (Dynamic_Solver.m:212-219) -------------------------------------------------------------------
int make_probe(Handle *h, const hjb_probe *pb, DProbe *out) {
    if (h->hp.model) return fail(h, HJB_E_UNSUPPORTED, "the probe block is not available for problems with a state model");
    if (h->tab64) return fail(h, HJB_E_UNSUPPORTED, "the probe block reports float32 next states; not available with table_dtype HJB_TAB_F64");
    if (h->cost64) return fail(h, HJB_E_UNSUPPORTED, "the probe block reports the float32 stage cost; not available with cost_dtype HJB_COST_F64");
    memset(out, 0, sizeof *out);
    int64_t B = 1;
    for (int a = 0; a < h->hp.D; ++a) {
        if (pb->lo[a] < 0 || pb->hi[a] > h->prob.n[a] || pb->lo[a] >= pb->hi[a])
            return fail(h, HJB_E_INVALID, "probe block [%d, %d) on axis %d of %d points (the reference's taps 50:55, 52:57 need dx >= 57, "
                        "Dynamic_Solver.m:213)", pb->lo[a], pb->hi[a], a, h->prob.n[a]);
        out->lo[a] = pb->lo[a];
        out->ext[a] = pb->hi[a] - pb->lo[a];
        B *= out->ext[a];
    }
    for (int c = 0; c < HJB_MAX_C; ++c) {
        const int mc = c < h->hp.C ? h->prob.m[c] : 1;
        if (c < h->hp.C && (pb->control[c] < 0 || pb->control[c] >= mc))
            return fail(h, HJB_E_INVALID, "probe control index %d on control dim %d of %d levels (the reference's tap 105 needs du >= 105)",
                        pb->control[c], c, mc);
        out->control[c] = c < h->hp.C ? pb->control[c] : 0;
    }
    if (B > ((int64_t)1 << 24)) return fail(h, HJB_E_INVALID, "probe block of %lld states is too large", (long long)B);
    out->B = B;
    return HJB_OK;
}

int launch_probe(Handle *h, const DProbe &pr, const void *dJn, hipStream_t st) {
    dim3 g((unsigned)std::min<int64_t>((pr.B + 255) / 256, 4096)), b(256);
#define HJB_LAUNCH_PROBE(TT, TTJ)                                                                                     \
    switch (h->hp.D) {                                                                                                \
        case 1: hipLaunchKernelGGL((k_probe<TT, TTJ, 1>), g, b, 0, st, h->dp, pr, (const TTJ *)dJn); break;            \
        case 2: hipLaunchKernelGGL((k_probe<TT, TTJ, 2>), g, b, 0, st, h->dp, pr, (const TTJ *)dJn); break;            \
        case 3: hipLaunchKernelGGL((k_probe<TT, TTJ, 3>), g, b, 0, st, h->dp, pr, (const TTJ *)dJn); break;            \
        case 4: hipLaunchKernelGGL((k_probe<TT, TTJ, 4>), g, b, 0, st, h->dp, pr, (const TTJ *)dJn); break;            \
        case 5: hipLaunchKernelGGL((k_probe<TT, TTJ, 5>), g, b, 0, st, h->dp, pr, (const TTJ *)dJn); break;            \
        default: hipLaunchKernelGGL((k_probe<TT, TTJ, 6>), g, b, 0, st, h->dp, pr, (const TTJ *)dJn); break;           \
    }
    if (h->dtype == HJB_F16S) { HJB_LAUNCH_PROBE(float, _Float16) }
    else if (h->dtype == HJB_F32) { HJB_LAUNCH_PROBE(float, float) }
    else { HJB_LAUNCH_PROBE(double, double) }
#undef HJB_LAUNCH_PROBE
    HIP_TRY(h, hipGetLastError());
    return HJB_OK;
}

}  // namespace hjbhost
