// hjbdp_api.hip - the single-device C ABI of libhjbdp (include/hjbdp.h): validation, hjb_create / hjb_destroy, options, one stage
// (hjb_backup_stage*), the probe block, policy lookup, the test hook.  hjb_solve is hjbdp_solve.hip.
// gfx950 (MI355X) only; no CPU fallback - without a HIP device every compute entry point returns HJB_E_DEVICE.
#include "hjbdp_host.h"
#include "kernels_lookup.h"

using namespace hjbhost;

template <typename T>
int policy_lookup_t(int32_t D, const int32_t *n, const double *const *knots, const void *values, int64_t nq,
                           const void *queries, int32_t method, void *out) {
    Handle tmp;   // only for allocation bookkeeping and error text
    Handle *h = &tmp;
    DLookup L{};
    L.D = D;
    L.method = method;
    int64_t s = 1;
    for (int a = 0; a < D; ++a) {
        std::vector<T> kk(n[a]), rdx(n[a]);
        for (int i = 0; i < n[a]; ++i) kk[i] = (T)knots[a][i];
        for (int i = 0; i + 1 < n[a]; ++i) rdx[i] = (T)1 / (T)(kk[i + 1] - kk[i]);     // increasing: hjb_policy_lookup checked
        rdx[n[a] - 1] = (T)0;
        int st = upload(h, kk, &L.knots[a]);
        if (!st) st = upload(h, rdx, &L.rdx[a]);
        if (st) { for (void *d : h->allocs) (void)hipFree(d); return st; }
        L.n[a] = n[a];
        L.stride[a] = s;
        s *= n[a];
    }
    void *dV = nullptr, *dQ = nullptr, *dO = nullptr;
    int st = dev_alloc(h, (size_t)s * sizeof(T), &dV);
    if (!st) st = dev_alloc(h, (size_t)nq * D * sizeof(T), &dQ);
    if (!st) st = dev_alloc(h, (size_t)nq * sizeof(T), &dO);
    hipError_t e = hipSuccess;
    if (!st) {
        e = hipMemcpy(dV, values, (size_t)s * sizeof(T), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dQ, queries, (size_t)nq * D * sizeof(T), hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            dim3 g(std::max(prep_grid(nq), 1)), b(256);
            switch (D) {
                case 1: hipLaunchKernelGGL((k_policy_lookup<T, 1>), g, b, 0, nullptr, L, (const T *)dV, nq, (const T *)dQ, (T *)dO); break;
                case 2: hipLaunchKernelGGL((k_policy_lookup<T, 2>), g, b, 0, nullptr, L, (const T *)dV, nq, (const T *)dQ, (T *)dO); break;
                case 3: hipLaunchKernelGGL((k_policy_lookup<T, 3>), g, b, 0, nullptr, L, (const T *)dV, nq, (const T *)dQ, (T *)dO); break;
                case 4: hipLaunchKernelGGL((k_policy_lookup<T, 4>), g, b, 0, nullptr, L, (const T *)dV, nq, (const T *)dQ, (T *)dO); break;
                case 5: hipLaunchKernelGGL((k_policy_lookup<T, 5>), g, b, 0, nullptr, L, (const T *)dV, nq, (const T *)dQ, (T *)dO); break;
                default: hipLaunchKernelGGL((k_policy_lookup<T, 6>), g, b, 0, nullptr, L, (const T *)dV, nq, (const T *)dQ, (T *)dO); break;
            }
            e = hipGetLastError();
            if (e == hipSuccess) e = hipMemcpy(out, dO, (size_t)nq * sizeof(T), hipMemcpyDeviceToHost);
        }
    }
    for (void *d : h->allocs) (void)hipFree(d);
    h->allocs.clear();
    h->arena_left = 0;
    if (st) return st;
    if (e != hipSuccess) return fail(nullptr, HJB_E_DEVICE, "hjb_policy_lookup: %s", hipGetErrorString(e));
    return HJB_OK;
}

extern "C" {

const char *hjb_version(void) { return "hjbdp 0.1.0 (gfx950)"; }

// Fault injection for the test suite, by explicit call only (the environment never changes what the library does).
int32_t hjb_test_hook(const char *key, int64_t value) {
    if (!key) return fail(nullptr, HJB_E_INVALID, "hjb_test_hook: null key");
    if (!strcmp(key, "fail_tab64_scratch")) { g_test_fail_tab64_scratch.store(value != 0); return HJB_OK; }
    if (!strcmp(key, "fail_tabled_alloc")) { g_test_fail_tabled_alloc.store(value != 0); return HJB_OK; }
    if (!strcmp(key, "rccl_only_env")) { g_test_rccl_only_env.store(value != 0); return HJB_OK; }
    if (!strcmp(key, "fail_graph_capture")) { g_test_fail_graph_capture.store(value != 0); return HJB_OK; }
    return fail(nullptr, HJB_E_INVALID, "hjb_test_hook: unknown key '%s'", key);
}

const char *hjb_status_string(int32_t s) {
    switch (s) {
        case HJB_OK: return "ok";
        case HJB_E_INVALID: return "invalid argument";
        case HJB_E_UNSUPPORTED: return "unsupported";
        case HJB_E_DEVICE: return "device error";
        case HJB_E_NOMEM: return "out of memory";
        case HJB_E_HALO: return "query outside slab halo";
        default: return "unknown status";
    }
}

int32_t hjb_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *hjb_last_error(hjb_handle hh) {
    Handle *h = (Handle *)hh;
    return h ? h->err.c_str() : g_last_error.c_str();
}

// Everything hjb_create checks or derives WITHOUT touching a device: argument validation, the label width, and (on
// request) the halo the last axis' tables imply.  hjb_create_multi / hjb_rank_create partition on these numbers alone.
}  // extern "C"
int64_t hjbhost::first_nonfinite(const void *data, int64_t n, bool f64) {
    // x - x is 0 for finite x and NaN for inf / NaN: blocks of 4096 summed branch-free (vectorisable), the element found on a hit
    constexpr int64_t kBlk = 4096;
    for (int64_t b0 = 0; b0 < n; b0 += kBlk) {
        const int64_t b1 = std::min(n, b0 + kBlk);
        double acc = 0.0;
        if (f64) { const double *x = (const double *)data; for (int64_t i = b0; i < b1; ++i) acc += x[i] - x[i]; }
        else { const float *x = (const float *)data; for (int64_t i = b0; i < b1; ++i) acc += (double)(x[i] - x[i]); }
        if (acc != 0.0) {
            for (int64_t i = b0; i < b1; ++i)
                if (!std::isfinite(f64 ? ((const double *)data)[i] : (double)((const float *)data)[i])) return i;
        }
    }
    return -1;
}

int hjbhost::analyse_problem(const hjb_problem *p, int *idx_bytes_out, int64_t *n_states_out, int *halo_lo, int *halo_hi) {
    if (!p) return fail(nullptr, HJB_E_INVALID, "null argument");
    if (p->D < 1 || p->D > HJB_MAX_D) return fail(nullptr, HJB_E_UNSUPPORTED, "D=%d not in 1..%d", p->D, HJB_MAX_D);
    if (p->C < 1 || p->C > HJB_MAX_C) return fail(nullptr, HJB_E_UNSUPPORTED, "C=%d not in 1..%d", p->C, HJB_MAX_C);
    if (p->dtype != HJB_F32 && p->dtype != HJB_F64 && p->dtype != HJB_F16S) return fail(nullptr, HJB_E_UNSUPPORTED, "dtype %d", p->dtype);
    if (p->index_base != 0 && p->index_base != 1) return fail(nullptr, HJB_E_INVALID, "index_base must be 0 or 1");
    if (p->model != HJB_MODEL_NONE && p->model != HJB_MODEL_QUAT_EULER321) return fail(nullptr, HJB_E_INVALID, "model %d", p->model);
    if (p->model == HJB_MODEL_QUAT_EULER321) {
        if (p->D != 6 || p->C != 3 || p->dtype == HJB_F64)
            return fail(nullptr, HJB_E_UNSUPPORTED, "HJB_MODEL_QUAT_EULER321 needs D=6, C=3, float32 arithmetic");
        for (int i = 0; i < 4; ++i)
            if (!p->model_tables[i]) return fail(nullptr, HJB_E_INVALID, "model_tables[%d] is null", i);
    }
    if (p->idx_dtype < HJB_IDX_I32 || p->idx_dtype > HJB_IDX_AUTO) return fail(nullptr, HJB_E_INVALID, "idx_dtype %d", p->idx_dtype);
    if (p->table_dtype != HJB_TAB_DEFAULT && p->table_dtype != HJB_TAB_F64) return fail(nullptr, HJB_E_INVALID, "table_dtype %d", p->table_dtype);
    if (p->cost_dtype != HJB_COST_DEFAULT && p->cost_dtype != HJB_COST_F64) return fail(nullptr, HJB_E_INVALID, "cost_dtype %d", p->cost_dtype);
    if (p->cost_dtype == HJB_COST_F64 && (p->dtype == HJB_F64 || p->model))
        return fail(nullptr, HJB_E_INVALID, "cost_dtype HJB_COST_F64 is for float32 arithmetic without a state model (a float64 problem sums its cost in float64 anyway)");
    if (p->table_dtype == HJB_TAB_F64 && (p->dtype == HJB_F64 || p->model))
        return fail(nullptr, HJB_E_INVALID, "table_dtype HJB_TAB_F64 is for float32 arithmetic without a state model (a float64 problem is float64 throughout)");
    const int G = p->D + p->C;
    int64_t nS = 1, nU = 1;
    for (int a = 0; a < p->D; ++a)       // sizes first: everything below multiplies them
        if (p->n[a] < 2) return fail(nullptr, HJB_E_INVALID, "n[%d]=%d < 2", a, p->n[a]);
    for (int c = 0; c < p->C; ++c) {
        if (p->m[c] < 1) return fail(nullptr, HJB_E_INVALID, "m[%d]=%d < 1", c, p->m[c]);
        if (nU > ((int64_t)1 << 31) / p->m[c]) return fail(nullptr, HJB_E_UNSUPPORTED, "too many controls");
        nU *= p->m[c];
    }
    for (int a = 0; a < p->D; ++a) {
        if (!p->knots[a]) return fail(nullptr, HJB_E_INVALID, "knots[%d] is null", a);
        for (int i = 0; i < p->n[a]; ++i)
            if (!std::isfinite(p->knots[a][i])) return fail(nullptr, HJB_E_INVALID, "knots[%d][%d] is not finite", a, i);
        for (int i = 0; i + 1 < p->n[a]; ++i)
            if (!(p->knots[a][i + 1] > p->knots[a][i]))
                return fail(nullptr, HJB_E_INVALID, "knots[%d] not strictly increasing at %d", a, i);
        const bool model_axis = p->model == HJB_MODEL_QUAT_EULER321 && a < 3;
        if (model_axis ? p->n_next_terms[a] != 0 : (p->n_next_terms[a] < 1 || p->n_next_terms[a] > HJB_MAX_TERMS))
            return fail(nullptr, HJB_E_INVALID, "n_next_terms[%d]=%d", a, p->n_next_terms[a]);
        for (int k = 0; k < p->n_next_terms[a]; ++k) {
            const hjb_term &t = p->next_terms[a][k];
            if (!t.data || (t.mask >> G)) return fail(nullptr, HJB_E_INVALID, "next term %d of axis %d: bad mask/data", k, a);
            if (term_elems(p, t.mask) >= ((int64_t)1 << 31)) return fail(nullptr, HJB_E_UNSUPPORTED, "next term %d of axis %d has >= 2^31 elements", k, a);
            const int64_t bad = first_nonfinite(t.data, term_elems(p, t.mask), p->dtype == HJB_F64 || p->table_dtype == HJB_TAB_F64);
            if (bad >= 0) return fail(nullptr, HJB_E_INVALID, "next term %d of axis %d: element %lld is not finite", k, a, (long long)bad);
        }
        // (six axes of 2^15 points would wrap a 64-bit product to 0 and pass every later size check)
        if (nS > kMaxStates / p->n[a]) return fail(nullptr, HJB_E_UNSUPPORTED, "more than 2^40 grid points (axes 0..%d)", a);
        nS *= p->n[a];
    }
    if (p->model == HJB_MODEL_QUAT_EULER321) {
        for (int i = 0; i < 4; ++i) {
            const int64_t bad = first_nonfinite(p->model_tables[i], (int64_t)p->n[0] * p->n[1] * p->n[2], false);
            if (bad >= 0) return fail(nullptr, HJB_E_INVALID, "model_tables[%d]: element %lld is not finite", i, (long long)bad);
        }
        if (!std::isfinite(p->model_h)) return fail(nullptr, HJB_E_INVALID, "model_h is not finite");
    }
    if (nU >= (int64_t)1 << 31) return fail(nullptr, HJB_E_UNSUPPORTED, "too many controls");
    if (p->n_cost_terms < 1 || p->n_cost_terms > HJB_MAX_TERMS) return fail(nullptr, HJB_E_INVALID, "n_cost_terms=%d", p->n_cost_terms);
    for (int k = 0; k < p->n_cost_terms; ++k)
        if (!p->cost_terms[k].data || (p->cost_terms[k].mask >> G)) return fail(nullptr, HJB_E_INVALID, "cost term %d: bad mask/data", k);
    for (int k = 0; k < p->n_cost_terms; ++k) {
        if (term_elems(p, p->cost_terms[k].mask) >= ((int64_t)1 << 31)) return fail(nullptr, HJB_E_UNSUPPORTED, "cost term %d has >= 2^31 elements", k);
        const int64_t bad = first_nonfinite(p->cost_terms[k].data, term_elems(p, p->cost_terms[k].mask), p->dtype == HJB_F64 || p->cost_dtype == HJB_COST_F64);
        if (bad >= 0) return fail(nullptr, HJB_E_INVALID, "cost term %d: element %lld is not finite", k, (long long)bad);
    }
    if (p->slab_begin || p->slab_end || p->halo_lo || p->halo_hi) {
        const int nl = p->n[p->D - 1];
        if (p->slab_begin < 0 || p->slab_end > nl || p->slab_begin >= p->slab_end || p->halo_lo < 0 || p->halo_hi < 0 ||
            p->slab_begin - p->halo_lo < 0 || p->slab_end + p->halo_hi > nl)
            return fail(nullptr, HJB_E_INVALID, "bad slab [%d,%d) halo %d/%d on axis of %d planes", p->slab_begin,
                        p->slab_end, p->halo_lo, p->halo_hi, nl);
        if ((p->slab_end + p->halo_hi) - (p->slab_begin - p->halo_lo) < 2)
            return fail(nullptr, HJB_E_INVALID, "slab + halo must span at least 2 planes");
    }
    int idx_bytes = 4;
    {
        const int64_t top = nU - 1 + p->index_base;                       // the largest label
        if (p->idx_dtype == HJB_IDX_U8 || (p->idx_dtype == HJB_IDX_AUTO && top <= 255)) idx_bytes = 1;
        else if (p->idx_dtype == HJB_IDX_U16 || (p->idx_dtype == HJB_IDX_AUTO && top <= 65535)) idx_bytes = 2;
        if ((idx_bytes == 1 && top > 255) || (idx_bytes == 2 && top > 65535))
            return fail(nullptr, HJB_E_INVALID, "idx_dtype %d cannot hold the label %lld", p->idx_dtype, (long long)top);
    }
    if (idx_bytes_out) *idx_bytes_out = idx_bytes;
    if (n_states_out) *n_states_out = nS;
    if (halo_lo && halo_hi) {
        const bool tab64 = p->table_dtype == HJB_TAB_F64;
        if (p->n_next_terms[p->D - 1] < 1) { *halo_lo = *halo_hi = 0; }
        else halo_of_problem(p, tab64, halo_lo, halo_hi);
    }
    return HJB_OK;
}
extern "C" {

int32_t hjb_create(const hjb_problem *p, int32_t device, hjb_handle *out) {
    if (!p || !out) return fail(nullptr, HJB_E_INVALID, "null argument");
    *out = nullptr;
    int idx_bytes = 4;
    {
        const int ast = analyse_problem(p, &idx_bytes, nullptr, nullptr, nullptr);
        if (ast) return ast;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(nullptr, HJB_E_DEVICE, "no HIP device visible (libhjbdp has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(nullptr, HJB_E_INVALID, "device %d not in 0..%d", device, ndev - 1);
    Handle *h = new Handle();
    h->device = device;
    h->idx_bytes = idx_bytes;
    h->tab64 = p->table_dtype == HJB_TAB_F64;
    h->cost64 = p->cost_dtype == HJB_COST_F64;
    h->dtype = p->dtype;
    h->esz = p->dtype == HJB_F16S ? 2 : (p->dtype == HJB_F32 ? 4 : 8);
    h->prob = *p;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) {
        int st = fail(nullptr, HJB_E_DEVICE, "hipSetDevice(%d): %s", device, hipGetErrorString(e));
        delete h;
        return st;
    }
    std::shared_lock<std::shared_mutex> create_lk(g_capture_mu);
    int st = build_handle(h, p);
    if (st) {
        g_last_error = h->err;
        for (void *d : h->allocs) (void)hipFree(d);
        delete h;
        return st;
    }
    // pointers in the kept copy must not be dereferenced later
    for (int a = 0; a < HJB_MAX_D; ++a) {
        h->prob.knots[a] = nullptr;
        for (int k = 0; k < HJB_MAX_TERMS; ++k) h->prob.next_terms[a][k].data = nullptr;
    }
    for (int k = 0; k < HJB_MAX_TERMS; ++k) h->prob.cost_terms[k].data = nullptr;
    choose_launch(h);
    if (h->L.status != HJB_OK) {
        // float64 queries / a float64 stage cost whose tables could not be built: the handle is not handed out (the build said why)
        st = fail(h, h->L.status, "%s: the tables of kernel variant %d could not be built: %s", h->tab64 ? "table_dtype HJB_TAB_F64"
                  : "cost_dtype HJB_COST_F64", h->L.variant, h->err.c_str());
        if (h->gexec) (void)hipGraphExecDestroy(h->gexec);
        for (void *d : h->allocs) (void)hipFree(d);
        delete h;
        return st;
    }
    *out = (hjb_handle)h;
    return HJB_OK;
}

int32_t hjb_destroy(hjb_handle hh) {
    Handle *h = (Handle *)hh;
    if (!h) return HJB_OK;
    std::shared_lock<std::shared_mutex> lk(g_capture_mu);
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    if (h->gexec) (void)hipGraphExecDestroy(h->gexec);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    for (void *d : h->allocs) (void)hipFree(d);
    delete h;
    return HJB_OK;
}

int32_t hjb_get_info(hjb_handle hh, hjb_info *info) {
    Handle *h = (Handle *)hh;
    if (!h || !info) return fail(h, HJB_E_INVALID, "null argument");
    info->n_states = h->n_owned;
    info->n_controls = h->nU;
    info->j_elems = h->j_elems;
    info->kernel_variant = h->L.variant;
    info->lds_bytes = (int32_t)h->L.lds;
    info->block = h->L.block;
    info->grid = h->L.grid;
    info->halo_needed_lo = h->halo_need_lo;
    info->halo_needed_hi = h->halo_need_hi;
    info->idx_bytes = h->idx_bytes;
    info->table_dtype = h->tab64 ? HJB_TAB_F64 : HJB_TAB_DEFAULT;
    info->cost_dtype = h->cost64 ? HJB_COST_F64 : HJB_COST_DEFAULT;
    info->reserved_ = 0;
    return HJB_OK;
}

int32_t hjb_set_option(hjb_handle hh, const char *key, int64_t value) {
    Handle *h = (Handle *)hh;
    if (!h || !key) return fail(h, HJB_E_INVALID, "null argument");
    std::shared_lock<std::shared_mutex> lk(g_capture_mu);     // may build tables (allocation, device sync)
    {   // options that rewrite device-resident plans or tables IN PLACE wait for the whole device first: a stage of this handle may
        // still be in flight on a non-blocking stream - the handle's own, a rank's strip streams, a caller's.  Not hot.
        static const char *const kRewrites[] = {"prep_mfma", "cs_dpp", "cs_split", "cs_coop", "cs_xcd_axis", "cs_xcd_mod", "chunk_order",
                                                "uw_tile", "uw_block", "axis0_table", "window_planes", "uniwin"};
        for (const char *k : kRewrites)
            if (!strcmp(key, k)) {
                HIP_TRY(h, hipSetDevice(h->device));
                HIP_TRY(h, hipDeviceSynchronize());
                break;
            }
    }
    if (!strcmp(key, "variant")) {
        if (value < -1 || value > 7) return fail(h, HJB_E_INVALID, "variant %lld unknown", (long long)value);      // (8 is not forced: hjb_set_disturbance)
        const char *why = nullptr;
        const int st = value < 0 ? HJB_OK : variant_status(h, (int)value, &why);
        if (st) return fail(h, st, "variant %lld: %s", (long long)value, why);
        h->forced_variant = (int)value;
        choose_launch(h);
        return HJB_OK;
    }
    if (!strcmp(key, "prep_mfma")) {       // rebuild every (cell, weight) table: 1 = MFMA outer-sum form where it applies
        HIP_TRY(h, hipSetDevice(h->device));
        return rebuild_tables(h, value != 0);      // (variant 7's plan is derived from the tables: same bits, nothing to redo)
    }
    if (!strcmp(key, "cs_dpp") || !strcmp(key, "cs_split") || !strcmp(key, "cs_coop") || !strcmp(key, "cs_xcd_axis") ||
        !strcmp(key, "cs_xcd_mod")) {
        // variant 7: cs_dpp 0 loads both axis-0 neighbours, cs_coop 0 runs one wave per column (testing); cs_split: parts a column is
        // swept in (0 = automatic); cs_xcd_axis: which axis the XCDs split (0 = group axis, 1 = window axis); cs_xcd_mod: residue
        // modulus of the column -> XCD assignment (0 = automatic)
        const bool xcd = !strcmp(key, "cs_xcd_axis") || !strcmp(key, "cs_xcd_mod");
        if (!strcmp(key, "cs_dpp")) h->cs_dpp = value != 0;
        else if (!strcmp(key, "cs_coop")) h->cs_coop = value != 0;
        else if (!strcmp(key, "cs_split") && value >= 0 && value <= 64) h->cs_split = (int)value;
        else if (!strcmp(key, "cs_xcd_axis") && value >= 0 && value <= 1) h->cs_xcd_axis = (int)value;
        else if (!strcmp(key, "cs_xcd_mod") && value >= -1 && value <= 4096) h->cs_xcd_mod = (int)value;
        else return fail(h, HJB_E_INVALID, "%s out of range", key);
        if (h->cs_state == 1) {
            const int cst = colsweep_options(h, xcd);
            if (cst) return cst;
            choose_launch(h);
        }
        return HJB_OK;
    }
    if (!strcmp(key, "block")) {                                     // variant 3: threads per workgroup = 64 x the states a workgroup sweeps side by side
        if (h->L.variant == 8 && (value == 64 || value == 128 || value == 256)) {      // variant 8 strides by whatever it is launched with (timing, tests)
            h->L.block = (int)value;
            launch_changed(h);
            return HJB_OK;
        }
        if (h->L.variant != 3 || (value != 256 && value != 512 && value != 1024)) return fail(h, HJB_E_UNSUPPORTED, "block: 256, 512 or 1024 on kernel variant 3");
        h->L.block = (int)value;
        launch_changed(h);
        return HJB_OK;
    }
    if (!strcmp(key, "grid")) {                                      // workgroups per launch of the grid-stride stage kernels (timing experiments)
        if (value < 1 || value > (1 << 20)) return fail(h, HJB_E_INVALID, "%s out of range", key);
        if (h->L.variant == 7 || h->L.mode >= 7 || h->L.variant == 1)
            return fail(h, HJB_E_UNSUPPORTED, "the launch size of kernel variant %d is part of its plan", h->L.variant);
        h->L.grid = (int)value;                                      // (until the next option that re-chooses the launch)
        launch_changed(h);
        return HJB_OK;
    }
    if (!strcmp(key, "tabled_i32")) {                                // 0: variant 5 in its 64-bit form whatever the sizes (A/B timing, tests)
        h->tabled_i32_on = value != 0;
        launch_changed(h);
        return HJB_OK;
    }
    if (!strcmp(key, "lds_pad")) {
        if (value < 0 || value > 128 * 1024) return fail(h, HJB_E_INVALID, "lds_pad out of range");
        h->lds_pad = (size_t)value;
        choose_launch(h);            // (K15 launches ONE generation of workgroups: its grid follows the occupancy)
        return HJB_OK;
    }
    if (!strcmp(key, "row_lean")) {
        h->row_lean = value != 0;
        choose_launch(h);
        return HJB_OK;
    }
    if (!strcmp(key, "temporal")) {
        if (value < 0 || value > 2) return fail(h, HJB_E_INVALID, "temporal must be 0, 1 or 2");
        h->use_temporal = (int)value;
        return HJB_OK;
    }
    if (!strcmp(key, "graph")) {
        h->use_graph = value != 0;
        return HJB_OK;
    }
    if (!strcmp(key, "axis0_table")) {      // 1: build the axis-0 (cell, t) table a mode-1 problem runs without (A/B timing, tests)
        if (value) {
            const int ast = ensure_axis0_table(h);
            if (ast) return ast;
            choose_launch(h);        // (mode 4 became mode 1)
        }
        return HJB_OK;
    }
    if (!strcmp(key, "window_planes")) {    // 4 / 3: variant 4's window modes with four planes (modes 2 / 3) or three (5 / 6)
        const bool three = h->packed_pre == 5 || h->packed_pre == 6, four = h->packed_pre == 2 || h->packed_pre == 3;
        if (!(three || four) || (value != 3 && value != 4)) return fail(h, HJB_E_UNSUPPORTED, "window_planes: 3 or 4, window modes only");
        if (value == 3 && !h->window3_ok) return fail(h, HJB_E_UNSUPPORTED, "window_planes 3: the inner control can skip a cell");
        if (value == 4 && three) { h->packed_pre -= 3; h->packed2_lds += 9 * 256 * 4 + 256 * 8; }
        if (value == 3 && four) { h->packed_pre += 3; h->packed2_lds -= 9 * 256 * 4 + 256 * 8; }
        choose_launch(h);          // (K15 serves the three-plane modes only: the grid follows; the captured launches are the other form)
        return HJB_OK;
    }
    if (!strcmp(key, "uniwin")) {           // K15 (kernels_uniwin.h): -1 automatic, 0 never, 1 whenever the structure holds
        if (value < -1 || value > 1) return fail(h, HJB_E_INVALID, "uniwin must be -1, 0 or 1");
        if (value == 1 && !h->uniwin_ok) return fail(h, HJB_E_UNSUPPORTED, "uniwin: the problem's rate axes are not shared by a chunk (kernels_uniwin.h)");
        h->uniwin_on = (int)value;
        choose_launch(h);
        return HJB_OK;
    }
    if (!strcmp(key, "uw_claim")) {         // K15: 1 = dynamic claim of the chunk walk's positions (default), 0 = fixed stride (A/B)
        if (!h->uniwin_ok) return fail(h, HJB_E_UNSUPPORTED, "uw_claim: K15 only");
        if (value != 0 && value != 1) return fail(h, HJB_E_INVALID, "uw_claim must be 0 or 1");
        h->uw_claim = (int)value;
        const int ust = uniwin_options(h);
        if (ust) return ust;
        launch_changed(h);           // (the captured launches zero the other counters)
        return HJB_OK;
    }
    if (!strcmp(key, "uw_tile") || !strcmp(key, "uw_block")) {
        // K15: log2 tile extents lA + 8 * lB + 64 * lC of the chunk walk (0: default) / states per chunk = threads per workgroup (256, 64)
        const bool tile = !strcmp(key, "uw_tile");
        if (tile ? (value < 0 || value > 511) : (value != 64 && value != 256)) return fail(h, HJB_E_INVALID, "%s out of range", key);
        if (!h->uniwin_ok) return fail(h, HJB_E_UNSUPPORTED, "%s: K15 only", key);
        if (tile) h->uw_tile = (int)value; else h->uw_block = (int)value;
        const int ust = uniwin_options(h);
        if (ust) return ust;
        choose_launch(h);
        return HJB_OK;
    }
    if (!strcmp(key, "chunk_order")) {      // variant 4, window modes: 0 transposed visiting order of the 256-state chunks, 1 state order
        if (value != 0 && value != 1) return fail(h, HJB_E_INVALID, "chunk_order must be 0 or 1");
        if (!h->dn) return fail(h, HJB_E_UNSUPPORTED, "chunk_order: variant 4's window modes only");
        h->hn.chunk_order = (int32_t)value;
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, hipMemcpy(h->dn, &h->hn, sizeof(DNested), hipMemcpyHostToDevice));
        return HJB_OK;
    }
    if (!strcmp(key, "eval_grid")) {        // workgroups per launch of the fixed-label stage (0: one per 256 states); "grid" is the stage kernels'
        if (value < 0 || value > (1 << 22)) return fail(h, HJB_E_INVALID, "%s out of range", key);
        h->eval_grid = (int)value;
        return HJB_OK;
    }
    if (!strcmp(key, "eval_i32")) {         // 0: the fixed-label stage in its 64-bit form whatever the sizes (A/B timing, tests)
        h->eval_i32 = value != 0;
        return HJB_OK;
    }
    if (!strcmp(key, "eval_m24")) {         // 0: the fixed-label stage's 32-bit form without the 24-bit index products (A/B timing, tests)
        h->eval_m24 = value != 0;
        return HJB_OK;
    }
    if (!strcmp(key, "dist_i32")) {         // 0: variant 8 in its 64-bit form whatever the sizes (A/B timing, tests)
        h->dist_i32 = value != 0;
        launch_changed(h);           // (the captured launches are the other form)
        return HJB_OK;
    }
    if (!strcmp(key, "dist_nodes") || !strcmp(key, "dist_mode") || !strcmp(key, "dist_axes") || !strcmp(key, "dist_form") || !strcmp(key, "dist_ctrl"))
        return fail(h, HJB_E_INVALID, "%s is read-only: hjb_set_disturbance sets the disturbance, the form follows from the sizes and dist_i32", key);
    if (!strcmp(key, "eval_form")) return fail(h, HJB_E_INVALID, "eval_form is read-only: the form follows from the sizes, eval_i32, eval_m24 and eval_tables");
    if (!strcmp(key, "eval_tables")) {      // the fixed-label stage's cells and weights: -1 automatic, 0 terms summed on the fly, 1 the (cell, t) tables
        if (value < -1 || value > 1) return fail(h, HJB_E_INVALID, "eval_tables must be -1, 0 or 1");
        if (value == 0 && h->tab64) return fail(h, HJB_E_UNSUPPORTED, "eval_tables 0: table_dtype HJB_TAB_F64 is evaluated from the tables only");
        if (value == 1 && !h->tabled_ok) return fail(h, HJB_E_UNSUPPORTED, "eval_tables 1: this grid's per-axis (cell, weight) tables do not fit");
        h->eval_tables = (int)value;
        return HJB_OK;
    }
    if (!strcmp(key, "monitor_single")) {   // hjb_solve_opts.monitor_single for callers of the flat API (hjb_solve_flat)
        h->monitor_single = value != 0;
        return HJB_OK;
    }
    return fail(h, HJB_E_INVALID, "unknown option '%s'", key);
}

int32_t hjb_get_option(hjb_handle hh, const char *key, int64_t *value) {
    Handle *h = (Handle *)hh;
    if (!h || !key || !value) return fail(h, HJB_E_INVALID, "null argument");
    if (!strcmp(key, "variant")) *value = h->L.variant;
    else if (!strcmp(key, "graph")) *value = h->use_graph ? 1 : 0;
    else if (!strcmp(key, "axis0_table")) *value = h->axis0_inline ? 0 : 1;       // 0: mode 1 forms axis 0's (cell, t) in the kernel
    else if (!strcmp(key, "monitor_single")) *value = h->monitor_single ? 1 : 0;
    // variant 4's contraction mode (kernels_packed2.h; 7 / 8: K15, kernels_uniwin.h), -1: not eligible
    else if (!strcmp(key, "packed2_mode")) *value = h->packed_mode ? (uniwin_active(h) ? h->packed_pre + 2 : h->packed_pre) : -1;
    else if (!strcmp(key, "uniwin")) *value = uniwin_active(h) ? 1 : 0;               // the form in effect
    else if (!strcmp(key, "uniwin_ok")) *value = h->uniwin_ok ? 1 : 0;
    else if (!strcmp(key, "uw_block")) *value = h->uniwin_ok ? h->huw.block : 0;
    else if (!strcmp(key, "uw_claim")) *value = h->uniwin_ok ? h->uw_claim : 0;
    else if (!strcmp(key, "uniwin_slow_points")) *value = h->uniwin_ok ? h->uniwin_slow : -1;
    else if (!strcmp(key, "grid")) *value = h->L.grid;
    else if (!strcmp(key, "eval_grid")) *value = h->eval_grid;
    else if (!strcmp(key, "eval_m24")) *value = h->eval_m24 ? 1 : 0;
    else if (!strcmp(key, "eval_i32")) *value = eval_runs_i32(h) ? 1 : 0;     // the form that would run
    else if (!strcmp(key, "eval_form")) *value = eval_form(h);                // 0 64-bit, 1 32-bit, 2 32-bit with 24-bit products: the next launch's
    else if (!strcmp(key, "eval_tables")) *value = h->eval_tables < 0 ? (h->tabled_ok ? 1 : 0) : h->eval_tables;      // the source in effect
    else if (!strcmp(key, "dist_nodes")) *value = h->dist_nodes;
    else if (!strcmp(key, "dist_mode")) *value = h->dist_mode;
    else if (!strcmp(key, "dist_axes")) *value = h->dist_axes;
    else if (!strcmp(key, "dist_form")) *value = dist_runs_i32(h) ? 1 : 0;    // 0 64-bit, 1 32-bit: the next launch's
    else if (!strcmp(key, "dist_i32")) *value = h->dist_i32 ? 1 : 0;
    else if (!strcmp(key, "dist_ctrl")) *value = h->dist_ctrl ? 1 : 0;        // 1: the disturbance in effect is per control (hjb_set_control_disturbance)
    else if (!strcmp(key, "idx_bytes")) *value = h->idx_bytes;
    else if (!strcmp(key, "temporal")) *value = h->use_temporal;
    else if (!strcmp(key, "chunk_order")) *value = h->dn ? h->hn.chunk_order : 0;
    else if (!strcmp(key, "row_lean")) *value = h->row_lean ? 1 : 0;
    else if (!strcmp(key, "lds_pad")) *value = (int64_t)h->lds_pad;
    else if (!strcmp(key, "cs_xcd_mod")) *value = h->cs_xcd_mod;
    else if (!strcmp(key, "cs_xcd_axis")) *value = h->cs_xcd_axis;
    else if (!strcmp(key, "cs_split")) *value = h->L.variant == 7 ? h->hcs.split : 0;       // the value in effect
    else if (!strcmp(key, "tabled_i32")) *value = (h->tabled_i32 && h->tabled_i32_on) ? 1 : 0;      // the form variant 5 would run
    else if (!strcmp(key, "cs_coop_why")) *value = h->cs_coop_why;
    else if (!strcmp(key, "cs_rows")) *value = h->L.variant == 7 ? h->cs_rows_mid : 0;
    else if (!strcmp(key, "prep_mfma")) *value = h->prep_mfma;
    else if (!strcmp(key, "prep_mfma_tables")) *value = h->prep_mfma_axes;
    else if (!strcmp(key, "prep_tables")) *value = (int64_t)h->preps.size();
    else if (!strcmp(key, "prep_ns")) *value = (int64_t)(h->prep_us * 1e3);          // device time of the last table rebuild
    else if (!strcmp(key, "table_hash")) {
        uint64_t hv = 0;
        std::shared_lock<std::shared_mutex> lk(g_capture_mu);
        HIP_TRY(h, hipSetDevice(h->device));
        const int hst = table_hash(h, &hv);
        if (hst) return hst;
        *value = (int64_t)(hv & 0x7fffffffffffffffull);
    }
    else if (!strcmp(key, "cs_dpp")) *value = (h->L.variant == 7 && h->L.dpp) ? 1 : 0;          // the form in effect
    else if (!strcmp(key, "cs_coop")) *value = (h->L.variant == 7 && h->L.coop_grid > 0) ? 1 : 0;   // the form in effect
    else if (!strcmp(key, "cs_groups")) *value = h->L.variant == 7 ? h->hcs.ng : 0;
    else if (!strcmp(key, "cs_group_axis")) *value = h->L.variant == 7 ? h->hcs.gax : -1;
    else if (!strcmp(key, "cs_cost_form")) *value = h->L.variant == 7 ? h->L.cost_form : -1;       // the launch record's: 0 general, 1 usual, 2 usual in float64
    else return fail(h, HJB_E_INVALID, "unknown option '%s'", key);
    return HJB_OK;
}

int32_t hjb_backup_stage_device(hjb_handle hh, const void *dJ_next, void *dJ_out, void *d_idx_out, void *stream) {
    Handle *h = (Handle *)hh;
    if (!h || !dJ_next || !dJ_out) return fail(h, HJB_E_INVALID, "null argument");
    if (dJ_next == dJ_out) return fail(h, HJB_E_INVALID, "J_next and J_out must not alias");
    HIP_TRY(h, hipSetDevice(h->device));
    return launch_stage(h, dJ_next, dJ_out, d_idx_out, (hipStream_t)stream);
}

int32_t hjb_check_device_status(hjb_handle hh, void *stream) {
    Handle *h = (Handle *)hh;
    if (!h) return fail(h, HJB_E_INVALID, "null handle");
    HIP_TRY(h, hipSetDevice(h->device));
    return check_status(h, (hipStream_t)stream);
}

int32_t hjb_backup_stage(hjb_handle hh, const void *J_next, void *J_out, void *idx_out) {
    Handle *h = (Handle *)hh;
    if (!h || !J_next || !J_out) return fail(h, HJB_E_INVALID, "null argument");
    std::shared_lock<std::shared_mutex> lk(g_capture_mu);
    HIP_TRY(h, hipSetDevice(h->device));
    int st = ensure_work(h);
    if (st) return st;
    const size_t jb = (size_t)h->j_elems * h->esz;
    HIP_TRY(h, hipMemcpy(h->dJ[0], J_next, jb, hipMemcpyHostToDevice));
    // keep halo planes of the output defined: start from the input
    HIP_TRY(h, hipMemcpy(h->dJ[1], h->dJ[0], jb, hipMemcpyDeviceToDevice));
    st = launch_stage(h, h->dJ[0], h->dJ[1], h->d_idx, nullptr);
    if (st) return st;
    st = check_status(h, nullptr);
    if (st) return st;
    HIP_TRY(h, hipMemcpy(J_out, h->dJ[1], jb, hipMemcpyDeviceToHost));
    if (idx_out) HIP_TRY(h, hipMemcpy(idx_out, h->d_idx, (size_t)h->n_owned * h->idx_bytes, hipMemcpyDeviceToHost));
    return HJB_OK;
}

int32_t hjb_policy_lookup(int32_t device, int32_t dtype, int32_t D, const int32_t *n, const double *const *knots,
                          const void *values, int64_t nq, const void *queries, int32_t method, void *out) {
    if (!n || !knots || !values || !queries || !out) return fail(nullptr, HJB_E_INVALID, "null argument");
    if (D < 1 || D > HJB_MAX_D) return fail(nullptr, HJB_E_UNSUPPORTED, "D=%d", D);
    if (dtype != HJB_F32 && dtype != HJB_F64) return fail(nullptr, HJB_E_UNSUPPORTED, "dtype %d", dtype);
    if (method != HJB_LOOKUP_NEAREST && method != HJB_LOOKUP_LINEAR) return fail(nullptr, HJB_E_INVALID, "method %d", method);
    if (nq < 0) return fail(nullptr, HJB_E_INVALID, "nq < 0");
    for (int a = 0; a < D; ++a) {
        if (n[a] < 2 || !knots[a]) return fail(nullptr, HJB_E_INVALID, "axis %d: need >= 2 knots", a);
        for (int i = 0; i + 1 < n[a]; ++i) {      // strictly increasing in the arithmetic type (float32 may merge close knots)
            const bool up = dtype == HJB_F32 ? (float)knots[a][i + 1] > (float)knots[a][i] : knots[a][i + 1] > knots[a][i];
            if (!up) return fail(nullptr, HJB_E_INVALID, "lookup: knots of axis %d not strictly increasing in the value type (at %d)", a, i);
        }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(nullptr, HJB_E_DEVICE, "no HIP device visible (libhjbdp has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(nullptr, HJB_E_INVALID, "device %d", device);
    std::shared_lock<std::shared_mutex> lk(g_capture_mu);
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, HJB_E_DEVICE, "hipSetDevice failed");
    if (nq == 0) return HJB_OK;
    return dtype == HJB_F32 ? policy_lookup_t<float>(D, n, knots, values, nq, queries, method, out)
                            : policy_lookup_t<double>(D, n, knots, values, nq, queries, method, out);
}

int32_t hjb_probe_stage(hjb_handle hh, const void *J_next, const hjb_probe *probe) {
    Handle *h = (Handle *)hh;
    if (!h || !probe) return fail(h, HJB_E_INVALID, "null argument");
    if (probe->j_interp && !J_next) return fail(h, HJB_E_INVALID, "j_interp needs J_next");
    std::shared_lock<std::shared_mutex> lk(g_capture_mu);
    HIP_TRY(h, hipSetDevice(h->device));
    DProbe pr{};
    int st = make_probe(h, probe, &pr);
    if (st) return st;
    const size_t tsz = h->dtype == HJB_F64 ? 8 : 4, pb = (size_t)pr.B * tsz;
    void *dg = nullptr, *dx = nullptr, *dj = nullptr;
    auto release = [&]() { if (dg) (void)hipFree(dg); if (dx) (void)hipFree(dx); if (dj) (void)hipFree(dj); };
    if ((probe->g && hipMalloc(&dg, pb) != hipSuccess) || (probe->x_next && hipMalloc(&dx, pb * h->hp.D) != hipSuccess) ||
        (probe->j_interp && hipMalloc(&dj, pb) != hipSuccess)) {
        release();
        return fail(h, HJB_E_NOMEM, "probe buffers");
    }
    pr.g = dg; pr.x_next = dx; pr.j_interp = dj;
    const void *dJn = nullptr;
    if (probe->j_interp) {
        st = ensure_work(h);
        if (st) { release(); return st; }
        if (hipMemcpy(h->dJ[0], J_next, (size_t)h->j_elems * h->esz, hipMemcpyHostToDevice) != hipSuccess) { release(); return fail(h, HJB_E_DEVICE, "copy of J_next failed"); }
        dJn = h->dJ[0];
    }
    st = launch_probe(h, pr, dJn, nullptr);
    if (!st) st = check_status(h, nullptr);
    hipError_t e = hipSuccess;
    if (!st && dg) e = hipMemcpy(probe->g, dg, pb, hipMemcpyDeviceToHost);
    if (!st && e == hipSuccess && dx) e = hipMemcpy(probe->x_next, dx, pb * h->hp.D, hipMemcpyDeviceToHost);
    if (!st && e == hipSuccess && dj) e = hipMemcpy(probe->j_interp, dj, pb, hipMemcpyDeviceToHost);
    release();
    if (st) return st;
    if (e != hipSuccess) return fail(h, HJB_E_DEVICE, "hjb_probe_stage: %s", hipGetErrorString(e));
    return HJB_OK;
}

}  // extern "C"
