// hjbdp_evaluate.hip - the cost of a GIVEN policy on the grid (include/hjbdp.h): hjb_evaluate_stage, hjb_evaluate_stage_device, hjb_evaluate.
// J_k(x) = g(x, u_k(x)) + F_{k+1}(x_next(x, u_k(x))): the backup without its min, on the labels hjb_backup_stage / hjb_solve write.
// gfx950 (MI355X) only; no CPU fallback - without a HIP device every compute entry point returns HJB_E_DEVICE.
#include "hjbdp_host.h"

using namespace hjbhost;

// First of n labels (idx_bytes wide) outside [lo, hi), -1: none.  The host-buffer entry points check the whole array before any
// device work, as hjb_rollout_create does.
static int64_t first_bad_label(const void *labels, int64_t n, int idx_bytes, int64_t lo, int64_t hi) {
    for (int64_t i = 0; i < n; ++i) {
        const int64_t v = idx_bytes == 4 ? (int64_t)((const int32_t *)labels)[i]
                        : idx_bytes == 1 ? (int64_t)((const uint8_t *)labels)[i] : (int64_t)((const uint16_t *)labels)[i];
        if (v < lo || v >= hi) return i;
    }
    return -1;
}

static int64_t label_at(const void *labels, int64_t i, int idx_bytes) {
    return idx_bytes == 4 ? (int64_t)((const int32_t *)labels)[i] : idx_bytes == 1 ? (int64_t)((const uint8_t *)labels)[i] : (int64_t)((const uint16_t *)labels)[i];
}

extern "C" {

int32_t hjb_evaluate_stage_device(hjb_handle hh, const void *dJ_next, const void *d_labels, void *dJ_out, void *stream) {
    Handle *h = (Handle *)hh;
    if (!h || !dJ_next || !d_labels || !dJ_out) return fail(h, HJB_E_INVALID, "null argument");
    if (dJ_next == dJ_out) return fail(h, HJB_E_INVALID, "J_next and J_out must not alias");
    HIP_TRY(h, hipSetDevice(h->device));
    return launch_evaluate(h, dJ_next, d_labels, dJ_out, (hipStream_t)stream);
}

int32_t hjb_evaluate_stage(hjb_handle hh, const void *J_next, const void *labels, void *J_out) {
    Handle *h = (Handle *)hh;
    if (!h || !J_next || !labels || !J_out) return fail(h, HJB_E_INVALID, "null argument");
    const int64_t lo = h->hp.index_base, hi = lo + h->nU;
    const int64_t bad = first_bad_label(labels, h->n_owned, h->idx_bytes, lo, hi);
    if (bad >= 0)
        return fail(h, HJB_E_INVALID, "hjb_evaluate_stage: label %lld of state %lld is outside [%lld, %lld)", (long long)label_at(labels, bad, h->idx_bytes),
                    (long long)bad, (long long)lo, (long long)hi);
    std::shared_lock<std::shared_mutex> lk(g_capture_mu);
    HIP_TRY(h, hipSetDevice(h->device));
    bool tabled = false;
    int st = prepare_evaluate(h, &tabled);
    if (!st) st = ensure_work(h);
    if (st) return st;
    const size_t jb = (size_t)h->j_elems * h->esz;
    HIP_TRY(h, hipMemcpy(h->dJ[0], J_next, jb, hipMemcpyHostToDevice));
    // keep halo planes of the output defined: start from the input
    HIP_TRY(h, hipMemcpy(h->dJ[1], h->dJ[0], jb, hipMemcpyDeviceToDevice));
    HIP_TRY(h, hipMemcpy(h->d_idx, labels, (size_t)h->n_owned * h->idx_bytes, hipMemcpyHostToDevice));
    st = launch_evaluate(h, h->dJ[0], h->d_idx, h->dJ[1], nullptr);
    if (!st) st = check_status(h, nullptr);
    if (st) return st;
    HIP_TRY(h, hipMemcpy(J_out, h->dJ[1], jb, hipMemcpyDeviceToHost));
    return HJB_OK;
}

int32_t hjb_evaluate(hjb_handle hh, int32_t n_stages, const void *terminal, const void *labels, int32_t labels_per_stage,
                     void *J_final, void *J_stages, double *sweep_ms) {
    Handle *h = (Handle *)hh;
    if (!h || !labels) return fail(h, HJB_E_INVALID, "null argument");
    if (n_stages < 1) return fail(h, HJB_E_INVALID, "n_stages=%d", n_stages);
    if (labels_per_stage != 0 && labels_per_stage != 1) return fail(h, HJB_E_INVALID, "labels_per_stage=%d (0: one stationary policy, 1: one plane per stage)", labels_per_stage);
    if (h->j_elems != h->n_owned)
        return fail(h, HJB_E_UNSUPPORTED, "hjb_evaluate runs whole grids; drive slabs with hjb_evaluate_stage_device + a halo exchange");
    const int64_t nS = h->n_owned;
    const int nlp = labels_per_stage ? n_stages : 1;          // planes of labels
    {
        const int64_t lo = h->hp.index_base, hi = lo + h->nU;
        const int64_t bad = first_bad_label(labels, nS * nlp, h->idx_bytes, lo, hi);
        if (bad >= 0)
            return fail(h, HJB_E_INVALID, "hjb_evaluate: label %lld of state %lld, plane %lld is outside [%lld, %lld)", (long long)label_at(labels, bad, h->idx_bytes),
                        (long long)(bad % nS), (long long)(bad / nS), (long long)lo, (long long)hi);
    }
    HIP_TRY(h, hipSetDevice(h->device));
    SharedHold unsafe_lk(g_capture_mu);    // allocation, synchronous copies, device sync
    bool tabled = false;
    int st = prepare_evaluate(h, &tabled);
    if (!st) st = ensure_work(h);
    if (st) return st;
    const size_t jb = (size_t)nS * h->esz, ib = (size_t)nS * h->idx_bytes;
    if (!h->stream) HIP_TRY(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    hipStream_t stream = h->stream;
    SweepScratch sc(h, unsafe_lk);
    char *dJst = nullptr, *dLab = nullptr;
    // the kernels write straight into the stage planes
    if (J_stages && (st = sc.alloc(jb * n_stages, false, &dJst, "cannot hold %d J stages on the device", n_stages))) return st;
    const char *dL = h->d_idx;                                  // a stationary policy sits in the handle's label buffer
    if (labels_per_stage) {
        if ((st = sc.alloc(ib * n_stages, false, &dLab, "cannot hold %d stages of labels on the device", n_stages))) return st;
        dL = dLab;
    }
    HIP_TRY(h, hipMemcpy((void *)dL, labels, ib * nlp, hipMemcpyHostToDevice));
    if (terminal) HIP_TRY(h, hipMemcpy(h->dJ[0], terminal, jb, hipMemcpyHostToDevice));
    else HIP_TRY(h, hipMemset(h->dJ[0], 0, jb));
    HIP_TRY(h, sync_setup());              // the loop runs on the handle's own stream from here
    HIP_TRY(h, hipEventCreate(&sc.ev0));
    HIP_TRY(h, hipEventCreate(&sc.ev1));
    HIP_TRY(h, hipEventRecord(sc.ev0, stream));
    const void *cur = h->dJ[0];
    int pp = 1;
    for (int k_s = n_stages; k_s >= 1; --k_s) {                 // the stage with reference index k_s reads label plane k_s - 1
        void *outJ = dJst ? (void *)(dJst + (size_t)(k_s - 1) * jb) : h->dJ[pp];
        if ((st = launch_evaluate(h, cur, labels_per_stage ? dL + (size_t)(k_s - 1) * ib : dL, outJ, stream))) return st;
        cur = outJ;
        if (!dJst) pp ^= 1;
    }
    HIP_TRY(h, hipEventRecord(sc.ev1, stream));
    HIP_TRY(h, hipEventSynchronize(sc.ev1));
    float ms = 0;
    HIP_TRY(h, hipEventElapsedTime(&ms, sc.ev0, sc.ev1));
    if ((st = check_status(h, stream))) return st;
    if (J_final) HIP_TRY(h, hipMemcpy(J_final, cur, jb, hipMemcpyDeviceToHost));
    if (J_stages) HIP_TRY(h, hipMemcpy(J_stages, dJst, jb * n_stages, hipMemcpyDeviceToHost));
    if (sweep_ms) *sweep_ms = ms;
    return HJB_OK;
}

}  // extern "C"
