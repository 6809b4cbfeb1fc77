// hjbdp_disturb.hip - hjb_set_disturbance and hjb_set_control_disturbance (include/hjbdp.h): the disturbance a handle's stages carry.
// Everything is checked first - the checks are stated once, for both setters; then the node offsets and weights are rounded once to the
// types the kernel reads them in (kernels_disturb.h DDisturb; the per-control table of kernels_ctrldist.h), written to the handle's
// device block (and table), and the launch is chosen again (variant 8 while nodes are set, the earlier launch after detaching).
// gfx950 (MI355X) only; no CPU fallback.
#include "hjbdp_host.h"
#include "kernels_disturb.h"

using namespace hjbhost;

// offsets: [D, W] column-major, or null (the per-control form: the block's own offsets stay zero, the kernel reads the table)
template <typename TQ, typename T>
static void fill_block(DDisturb<TQ, T> *B, int D, int mode, int W, uint32_t axes, const double *offsets, const double *weights) {
    memset(B, 0, sizeof *B);
    B->n_nodes = W;
    B->mode = mode;
    B->axes = axes;
    for (int w = 0; w < W; ++w) {
        for (int a = 0; a < D && offsets; ++a) B->off[a][w] = (TQ)offsets[a + (size_t)D * w];
        B->p[w] = weights ? (T)weights[w] : (T)(1.0 / W);
    }
}

template <typename TQ, typename T>
static int write_block(Handle *h, int D, int mode, int W, uint32_t axes, const double *offsets, const double *weights) {
    DDisturb<TQ, T> B;
    fill_block(&B, D, mode, W, axes, offsets, weights);
    HIP_TRY(h, hipMemcpy(h->d_dist, &B, sizeof B, hipMemcpyHostToDevice));
    return HJB_OK;
}

// The per-control table as the kernel visits it: row r = the r-th control in visiting order (control dim 0 slowest), then the node, the D
// entries of one (control, node) contiguous; offsets is [D, W, nU] column-major by the 0-based column-major LABEL (dim 0 fastest).
template <typename TQ>
static int write_table(Handle *h, int D, int W, const double *offsets) {
    const DParams &P = h->hp;
    const int64_t m0 = P.m[0], m1 = P.C > 1 ? P.m[1] : 1, m2 = P.C > 2 ? P.m[2] : 1;
    std::vector<TQ> tab((size_t)h->nU * W * D);
    size_t at = 0;
    for (int64_t j0 = 0; j0 < m0; ++j0)
        for (int64_t j1 = 0; j1 < m1; ++j1)
            for (int64_t j2 = 0; j2 < m2; ++j2) {
                const size_t l = (size_t)(j0 + m0 * (j1 + m1 * j2));
                for (int w = 0; w < W; ++w)
                    for (int a = 0; a < D; ++a) tab[at++] = (TQ)offsets[a + (size_t)D * (w + (size_t)W * l)];
            }
    HIP_TRY(h, hipMemcpy(h->d_dist_tab, tab.data(), tab.size() * sizeof(TQ), hipMemcpyHostToDevice));
    return HJB_OK;
}

// Both setters.  n_controls < 0: hjb_set_disturbance (offsets [D, n_nodes]); else hjb_set_control_disturbance (offsets [D, n_nodes, nU]).
static int set_disturbance(Handle *h, const char *who, int32_t mode, int32_t n_nodes, int32_t n_controls, const double *offsets, const double *weights) {
    if (!h) return fail(nullptr, HJB_E_INVALID, "%s: null handle", who);
    const bool ctrl = n_controls >= 0;
    if (mode != HJB_DIST_EXPECT && mode != HJB_DIST_WORST) return fail(h, HJB_E_INVALID, "%s: mode %d (HJB_DIST_EXPECT or HJB_DIST_WORST)", who, mode);
    if (n_nodes < 0 || n_nodes > HJB_DIST_MAX_NODES) return fail(h, HJB_E_INVALID, "%s: n_nodes=%d not in 0..%d", who, n_nodes, HJB_DIST_MAX_NODES);
    const int D = h->hp.D;
    uint32_t axes = 0;
    if (n_nodes > 0) {
        if (ctrl) {     // (before the table is read: one of the wrong size is refused, not read past)
            if ((int64_t)n_controls != h->nU)
                return fail(h, HJB_E_INVALID, "%s: n_controls=%d, the handle has %lld controls", who, n_controls, (long long)h->nU);
            if ((int64_t)D * n_nodes * h->nU > HJB_CTRL_DIST_MAX_ENTRIES)
                return fail(h, HJB_E_UNSUPPORTED, "%s: a table of %d x %d x %lld entries is over the limit of 2^26", who, D, n_nodes, (long long)h->nU);
        }
        if (!offsets) return fail(h, HJB_E_INVALID, "%s: null offsets with n_nodes=%d", who, n_nodes);
        if (weights && mode == HJB_DIST_WORST) return fail(h, HJB_E_INVALID, "%s: HJB_DIST_WORST takes no weights", who);
        const int64_t cols = ctrl ? (int64_t)n_nodes * h->nU : n_nodes;      // (node, control) columns of D entries
        for (int64_t c = 0; c < cols; ++c) {
            for (int a = 0; a < D; ++a) {
                const double d = offsets[a + (size_t)D * c];
                if (!std::isfinite(d)) {
                    if (ctrl) return fail(h, HJB_E_INVALID, "%s: offset of axis %d, node %d, control %lld is not finite", who, a, (int)(c % n_nodes), (long long)(c / n_nodes));
                    return fail(h, HJB_E_INVALID, "%s: offset of axis %d, node %d is not finite", who, a, (int)c);
                }
                if (d != 0.0) axes |= 1u << a;
            }
            if (weights && c < n_nodes && !(std::isfinite(weights[c]) && weights[c] >= 0.0))
                return fail(h, HJB_E_INVALID, "%s: weight %d is not finite or is negative", who, (int)c);
        }
        const hjb_problem &p = h->prob;
        if (p.slab_begin || p.slab_end || p.halo_lo || p.halo_hi)
            return fail(h, HJB_E_UNSUPPORTED, "%s: a slab handle takes no disturbance (an offset last axis changes the halo the slab needs)", who);
        if (h->hp.model) return fail(h, HJB_E_UNSUPPORTED, "%s: a handle with a state model takes no disturbance (its next states are formed in variant 4 only)", who);
    }
    if (n_nodes == 0 && h->dist_nodes == 0) return HJB_OK;      // nothing set, nothing to detach: the handle is not touched
    std::shared_lock<std::shared_mutex> lk(g_capture_mu);        // allocation, device sync, a synchronous copy
    HIP_TRY(h, hipSetDevice(h->device));
    if (n_nodes > 0) {
        // the largest typing's block serves all (rewritten IN PLACE: a stage of this handle may still be in flight on a non-blocking stream)
        if (!h->d_dist) {
            const int ast = dev_alloc(h, sizeof(DDisturb<double, double>), &h->d_dist);
            if (ast) return ast;
        }
        HIP_TRY(h, hipDeviceSynchronize());
        const bool q64 = h->dtype == HJB_F64 || h->tab64;
        if (ctrl) {
            // the table: in place while it fits, a new allocation when it grows (nothing of this handle is in flight any more)
            const size_t bytes = (size_t)D * n_nodes * h->nU * (q64 ? sizeof(double) : sizeof(float));
            if (bytes > h->dist_tab_bytes) {
                void *d = nullptr;
                HIP_TRY(h, hipMalloc(&d, bytes));
                if (h->d_dist_tab) {
                    h->allocs.erase(std::remove(h->allocs.begin(), h->allocs.end(), h->d_dist_tab), h->allocs.end());
                    (void)hipFree(h->d_dist_tab);
                }
                h->allocs.push_back(d);
                h->d_dist_tab = d;
                h->dist_tab_bytes = bytes;
            }
            const int tst = q64 ? write_table<double>(h, D, n_nodes, offsets) : write_table<float>(h, D, n_nodes, offsets);
            if (tst) return tst;
        }
        const double *block_off = ctrl ? nullptr : offsets;
        const int bst = h->dtype == HJB_F64 ? write_block<double, double>(h, D, mode, n_nodes, axes, block_off, weights)
                        : h->tab64          ? write_block<double, float>(h, D, mode, n_nodes, axes, block_off, weights)
                                            : write_block<float, float>(h, D, mode, n_nodes, axes, block_off, weights);
        if (bst) return bst;
    }
    h->dist_nodes = n_nodes;
    h->dist_mode = n_nodes > 0 ? mode : HJB_DIST_EXPECT;
    h->dist_axes = axes;
    h->dist_ctrl = ctrl && n_nodes > 0;
    choose_launch(h);
    return HJB_OK;
}

extern "C" int32_t hjb_set_disturbance(hjb_handle hh, int32_t mode, int32_t n_nodes, const double *offsets, const double *weights) {
    return set_disturbance((Handle *)hh, "hjb_set_disturbance", mode, n_nodes, -1, offsets, weights);
}

extern "C" int32_t hjb_set_control_disturbance(hjb_handle hh, int32_t mode, int32_t n_nodes, int32_t n_controls, const double *offsets,
                                               const double *weights) {
    if (n_controls < 0) return fail((Handle *)hh, HJB_E_INVALID, "hjb_set_control_disturbance: n_controls=%d", n_controls);
    return set_disturbance((Handle *)hh, "hjb_set_control_disturbance", mode, n_nodes, n_controls, offsets, weights);
}
