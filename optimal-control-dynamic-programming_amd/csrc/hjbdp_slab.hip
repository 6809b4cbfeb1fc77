// hjbdp_slab.hip - one device's slab of a grid partitioned along its last state axis: the slab handle, the interior and strip
// handles over the same buffers, the strip streams, and the enqueue of one stage (fork, interior, strips behind the halos, join).
// What hjb_solve_multi does per device and hjb_rank_* per process; which planes each part owns and sees is hjbdp_slab.h's.
// gfx950 (MI355X) only; no CPU fallback - without a HIP device every compute entry point returns HJB_E_DEVICE.
#include "hjbdp_host.h"

namespace hjbhost {

int slab_grid(const hjb_problem *p, SlabGrid *g) {
    int ib = 4, hl = 0, hh = 0;
    int64_t ns = 0;
    const int st = analyse_problem(p, &ib, &ns, &hl, &hh);      // host arithmetic on the last axis' terms
    if (st) return st;
    g->need_lo = hl;
    g->need_hi = hh;
    g->nl = p->n[p->D - 1];
    g->dtype = p->dtype;
    g->esz = p->dtype == HJB_F16S ? 2 : (p->dtype == HJB_F32 ? 4 : 8);
    g->isz = (size_t)ib;
    g->inner = ns / g->nl;
    return HJB_OK;
}

void slab_destroy(Slab *S) {
    for (int i = 0; i < 2; ++i) {
        if (S->sdone[i]) (void)hipEventDestroy(S->sdone[i]);
        if (S->ss[i]) (void)hipStreamDestroy(S->ss[i]);
    }
    if (S->fork) (void)hipEventDestroy(S->fork);
    for (int i = 0; i < 3; ++i) if (S->part[i]) (void)hjb_destroy((hjb_handle)S->part[i]);
    if (S->whole) (void)hjb_destroy((hjb_handle)S->whole);
    *S = Slab{};
}

int slab_create(Slab *S, const hjb_problem *p, const SlabGrid &g, int device, int k, int n_slabs, bool split) {
    const SlabRange r = slab_range(g.nl, n_slabs, k);
    const SlabHalo halo = slab_halo(g.need_lo, g.need_hi, r.begin, r.end, g.nl);
    S->device = device;
    S->begin = r.begin; S->end = r.end; S->hlo = halo.lo; S->hhi = halo.hi;
    S->plane_b = (size_t)g.inner * g.esz;
    S->label_plane_b = (size_t)g.inner * g.isz;
    S->cut = slab_split(g.need_lo, g.need_hi, r.begin, r.end, halo, split, n_slabs);
    auto make = [&](int sb, int se, int hl, int hh, Handle **hout) {
        hjb_problem q = *p;
        if (n_slabs > 1) { q.slab_begin = sb; q.slab_end = se; q.halo_lo = hl; q.halo_hi = hh; }
        hjb_handle h = nullptr;
        const int s2 = hjb_create(&q, device, &h);
        *hout = (Handle *)h;
        return s2;
    };
    int st = make(S->begin, S->end, S->hlo, S->hhi, &S->whole);
    for (int i = 0; i < 3 && !st; ++i) {
        const SlabPart &c = S->cut.part[i];
        if (c.on) st = make(c.begin, c.end, c.halo_lo, c.halo_hi, &S->part[i]);
    }
    if (!st) {
        bool ok = hipSetDevice(device) == hipSuccess && hipEventCreateWithFlags(&S->fork, hipEventDisableTiming) == hipSuccess;
        for (int i = 0; i < 2 && ok; ++i)
            ok = hipEventCreateWithFlags(&S->sdone[i], hipEventDisableTiming) == hipSuccess &&
                 hipStreamCreateWithFlags(&S->ss[i], hipStreamNonBlocking) == hipSuccess;
        if (!ok) st = fail(nullptr, HJB_E_DEVICE, "stream / event creation failed on device %d", device);
    }
    if (st) {
        const std::string keep = g_last_error;
        slab_destroy(S);
        g_last_error = keep;
    }
    return st;
}

int slab_enqueue_stage(Slab &S, const void *J_in, void *J_out, void *idx, hipStream_t cs, hipEvent_t halo, bool strips_first, std::string *err) {
#define SLAB_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            const int st_ = fail(nullptr, HJB_E_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e_)); \
            *err = g_last_error;                                                               \
            return st_;                                                                        \
        }                                                                                      \
    } while (0)
    // part k (-1: the whole slab) on `stream`: its view starts row0 planes into the slab's buffers, its labels own0 planes in
    auto stage_part = [&](int k, hipStream_t stream) -> int {
        Handle *h = k < 0 ? S.whole : S.part[k];
        const int64_t row0 = k < 0 ? 0 : S.cut.part[k].row0, own0 = k < 0 ? 0 : S.cut.part[k].own0;
        const int st = launch_stage(h, (const char *)J_in + S.plane_b * row0, (char *)J_out + S.plane_b * row0,
                                    idx ? (char *)idx + S.label_plane_b * own0 : nullptr, stream);
        if (st) *err = h->err;
        return st;
    };
    if (!S.part[0]) {                        // no interior to overlap with: the halos first, then one kernel
        if (halo) SLAB_TRY(hipStreamWaitEvent(cs, halo, 0));
        return stage_part(-1, cs);
    }
    SLAB_TRY(hipEventRecord(S.fork, cs));    // fork point: everything this stage depends on, before the interior
    for (int k = 1; k <= 2; ++k)
        if (S.part[k]) SLAB_TRY(hipStreamWaitEvent(S.ss[k - 1], S.fork, 0));
    int st = strips_first ? HJB_OK : stage_part(0, cs);
    for (int k = 1; k <= 2 && !st; ++k)
        if (S.part[k]) {
            if (halo) SLAB_TRY(hipStreamWaitEvent(S.ss[k - 1], halo, 0));
            st = stage_part(k, S.ss[k - 1]);
            if (!st) SLAB_TRY(hipEventRecord(S.sdone[k - 1], S.ss[k - 1]));
        }
    if (strips_first && !st) st = stage_part(0, cs);
    if (st) return st;
    for (int k = 1; k <= 2; ++k)             // the join: later work on cs (and events recorded there) is behind both strips
        if (S.part[k]) SLAB_TRY(hipStreamWaitEvent(cs, S.sdone[k - 1], 0));
    return HJB_OK;
#undef SLAB_TRY
}

}  // namespace hjbhost
