// hjbdp_disturb.hip - hjb_set_disturbance (include/hjbdp.h): the disturbance a handle's stages carry.  Everything is checked first; then
// the node offsets and weights are rounded once to the types the kernel reads them in (kernels_disturb.h DDisturb), written to the
// handle's device block, and the launch is chosen again (variant 8 while nodes are set, the earlier launch after detaching).
// gfx950 (MI355X) only; no CPU fallback.
#include "hjbdp_host.h"
#include "kernels_disturb.h"

using namespace hjbhost;

template <typename TQ, typename T>
static void fill_block(DDisturb<TQ, T> *B, int D, int mode, int W, uint32_t axes, const double *offsets, const double *weights) {
    memset(B, 0, sizeof *B);
    B->n_nodes = W;
    B->mode = mode;
    B->axes = axes;
    for (int w = 0; w < W; ++w) {
        for (int a = 0; a < D; ++a) B->off[a][w] = (TQ)offsets[a + (size_t)D * w];
        B->p[w] = weights ? (T)weights[w] : (T)(1.0 / W);
    }
}

extern "C" int32_t hjb_set_disturbance(hjb_handle hh, int32_t mode, int32_t n_nodes, const double *offsets, const double *weights) {
    Handle *h = (Handle *)hh;
    if (!h) return fail(nullptr, HJB_E_INVALID, "hjb_set_disturbance: null handle");
    if (mode != HJB_DIST_EXPECT && mode != HJB_DIST_WORST) return fail(h, HJB_E_INVALID, "hjb_set_disturbance: mode %d (HJB_DIST_EXPECT or HJB_DIST_WORST)", mode);
    if (n_nodes < 0 || n_nodes > HJB_DIST_MAX_NODES) return fail(h, HJB_E_INVALID, "hjb_set_disturbance: n_nodes=%d not in 0..%d", n_nodes, HJB_DIST_MAX_NODES);
    const int D = h->hp.D;
    uint32_t axes = 0;
    if (n_nodes > 0) {
        if (!offsets) return fail(h, HJB_E_INVALID, "hjb_set_disturbance: null offsets with n_nodes=%d", n_nodes);
        if (weights && mode == HJB_DIST_WORST) return fail(h, HJB_E_INVALID, "hjb_set_disturbance: HJB_DIST_WORST takes no weights");
        for (int w = 0; w < n_nodes; ++w) {
            for (int a = 0; a < D; ++a) {
                const double d = offsets[a + (size_t)D * w];
                if (!std::isfinite(d)) return fail(h, HJB_E_INVALID, "hjb_set_disturbance: offset of axis %d, node %d is not finite", a, w);
                if (d != 0.0) axes |= 1u << a;
            }
            if (weights && !(std::isfinite(weights[w]) && weights[w] >= 0.0))
                return fail(h, HJB_E_INVALID, "hjb_set_disturbance: weight %d is not finite or is negative", w);
        }
        const hjb_problem &p = h->prob;
        if (p.slab_begin || p.slab_end || p.halo_lo || p.halo_hi)
            return fail(h, HJB_E_UNSUPPORTED, "hjb_set_disturbance: a slab handle takes no disturbance (an offset last axis changes the halo the slab needs)");
        if (h->hp.model) return fail(h, HJB_E_UNSUPPORTED, "hjb_set_disturbance: a handle with a state model takes no disturbance (its next states are formed in variant 4 only)");
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
        if (h->dtype == HJB_F64) {
            DDisturb<double, double> B;
            fill_block(&B, D, mode, n_nodes, axes, offsets, weights);
            HIP_TRY(h, hipMemcpy(h->d_dist, &B, sizeof B, hipMemcpyHostToDevice));
        } else if (h->tab64) {
            DDisturb<double, float> B;
            fill_block(&B, D, mode, n_nodes, axes, offsets, weights);
            HIP_TRY(h, hipMemcpy(h->d_dist, &B, sizeof B, hipMemcpyHostToDevice));
        } else {
            DDisturb<float, float> B;
            fill_block(&B, D, mode, n_nodes, axes, offsets, weights);
            HIP_TRY(h, hipMemcpy(h->d_dist, &B, sizeof B, hipMemcpyHostToDevice));
        }
    }
    h->dist_nodes = n_nodes;
    h->dist_mode = n_nodes > 0 ? mode : HJB_DIST_EXPECT;
    h->dist_axes = axes;
    choose_launch(h);
    return HJB_OK;
}
