// rollout.hip - hjb_rollout_*: batched closed-loop rollouts of a stored per-stage policy (include/hjbdp.h; kernel: kernels_rollout.h).
#include "hjbdp_host.h"
#include "kernels_rollout.h"

using namespace hjbhost;

namespace {

struct Rollout {
    std::mutex mu;                  // one call at a time per object
    int device = 0, D = 0, idx_bytes = 4, n_planes = 0;
    bool model_set = false;
    int64_t chunk = (int64_t)1 << 20;
    DRollout R{};                   // device pointers filled by create; model by set_model
    std::vector<void *> allocs;
    hipStream_t stream = nullptr;
    std::string err;
};

constexpr int64_t kMaxChunk = (int64_t)1 << 30;
constexpr size_t kLdsMax = 32 << 10;        // knots + 1/dx + u_table staged in LDS up to this size

int rfail(Rollout *ro, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ro) ro->err = buf;
    g_last_error = buf;
    return code;
}

void release(Rollout *ro) {
    for (void *p : ro->allocs) (void)hipFree(p);
    ro->allocs.clear();
    if (ro->stream) (void)hipStreamDestroy(ro->stream);
    ro->stream = nullptr;
}

template <typename TL>
int64_t first_bad_label(const void *labels, int64_t count, int64_t lo, int64_t hi) {
    const TL *l = static_cast<const TL *>(labels);
    for (int64_t i = 0; i < count; ++i)
        if ((int64_t)l[i] < lo || (int64_t)l[i] >= hi) return i;
    return -1;
}

template <int D, typename TL, int M, bool LDS>
void launch_d(const DRollout &R, int64_t nc, size_t lds, hipStream_t st, const double *X0, double *Xf, double *cost, double *Xp,
              double *Up) {
    dim3 b(256), g((unsigned)((nc + 255) / 256));
    hipLaunchKernelGGL((k_rollout<D, TL, M, LDS>), g, b, LDS ? lds : 0, st, R, nc, X0, Xf, cost, Xp, Up);
}

template <typename TL, int M, bool LDS>
void launch_t(int D, const DRollout &R, int64_t nc, size_t lds, hipStream_t st, const double *X0, double *Xf, double *cost,
              double *Xp, double *Up) {
    switch (D) {
        case 1: launch_d<1, TL, M, LDS>(R, nc, lds, st, X0, Xf, cost, Xp, Up); break;
        case 2: launch_d<2, TL, M, LDS>(R, nc, lds, st, X0, Xf, cost, Xp, Up); break;
        case 3: launch_d<3, TL, M, LDS>(R, nc, lds, st, X0, Xf, cost, Xp, Up); break;
        case 4: launch_d<4, TL, M, LDS>(R, nc, lds, st, X0, Xf, cost, Xp, Up); break;
        case 5: launch_d<5, TL, M, LDS>(R, nc, lds, st, X0, Xf, cost, Xp, Up); break;
        default: launch_d<6, TL, M, LDS>(R, nc, lds, st, X0, Xf, cost, Xp, Up); break;
    }
}

template <typename TL>
void launch_m(int D, int method, bool lds_on, const DRollout &R, int64_t nc, size_t lds, hipStream_t st, const double *X0,
              double *Xf, double *cost, double *Xp, double *Up) {
    if (method == HJB_LOOKUP_NEAREST) {
        if (lds_on) launch_t<TL, HJB_LOOKUP_NEAREST, true>(D, R, nc, lds, st, X0, Xf, cost, Xp, Up);
        else launch_t<TL, HJB_LOOKUP_NEAREST, false>(D, R, nc, lds, st, X0, Xf, cost, Xp, Up);
    } else {
        if (lds_on) launch_t<TL, HJB_LOOKUP_LINEAR, true>(D, R, nc, lds, st, X0, Xf, cost, Xp, Up);
        else launch_t<TL, HJB_LOOKUP_LINEAR, false>(D, R, nc, lds, st, X0, Xf, cost, Xp, Up);
    }
}

bool all_finite(const double *p, int64_t n) { return !p || first_nonfinite(p, n, true) < 0; }

}  // namespace

extern "C" {

int32_t hjb_rollout_create(int32_t device, int32_t D, const int32_t *n, const double *knots, int32_t idx_dtype,
                           int32_t index_base, int32_t n_planes, const void *labels, int32_t n_labels, int32_t n_u,
                           const double *u_table, void **rollout_out) {
    if (!n || !knots || !labels || !u_table || !rollout_out) return rfail(nullptr, HJB_E_INVALID, "rollout: null argument");
    *rollout_out = nullptr;
    if (D < 1 || D > HJB_MAX_D) return rfail(nullptr, HJB_E_UNSUPPORTED, "rollout: D=%d not in 1..%d", D, HJB_MAX_D);
    if (n_u < 1 || n_u > HJB_ROLLOUT_MAX_U) return rfail(nullptr, HJB_E_UNSUPPORTED, "rollout: n_u=%d not in 1..%d", n_u, HJB_ROLLOUT_MAX_U);
    int idx_bytes = 0;
    if (idx_dtype == HJB_IDX_I32) idx_bytes = 4;
    else if (idx_dtype == HJB_IDX_U8) idx_bytes = 1;
    else if (idx_dtype == HJB_IDX_U16) idx_bytes = 2;
    else return rfail(nullptr, HJB_E_INVALID, "rollout: idx_dtype %d is not HJB_IDX_I32 / _U8 / _U16", idx_dtype);
    if (index_base != 0 && index_base != 1) return rfail(nullptr, HJB_E_INVALID, "rollout: index_base %d (0 or 1)", index_base);
    if (n_planes < 1) return rfail(nullptr, HJB_E_INVALID, "rollout: n_planes=%d < 1", n_planes);
    if (n_labels < 1) return rfail(nullptr, HJB_E_INVALID, "rollout: n_labels=%d < 1", n_labels);
    int64_t nS = 1, n_knots = 0;
    for (int a = 0; a < D; ++a) {
        if (n[a] < 2) return rfail(nullptr, HJB_E_INVALID, "rollout: axis %d has %d knots (need >= 2)", a, n[a]);
        const double *kk = knots + n_knots;
        for (int i = 0; i < n[a]; ++i)
            if (!std::isfinite(kk[i])) return rfail(nullptr, HJB_E_INVALID, "rollout: knot %d of axis %d is not finite", i, a);
        for (int i = 0; i + 1 < n[a]; ++i)
            if (!(kk[i + 1] > kk[i])) return rfail(nullptr, HJB_E_INVALID, "rollout: knots of axis %d not strictly increasing (at %d)", a, i);
        n_knots += n[a];
        if (n_knots > INT32_MAX || nS > kMaxStates / n[a]) return rfail(nullptr, HJB_E_INVALID, "rollout: size overflow (grid)");
        nS *= n[a];
    }
    if ((int64_t)n_planes > kMaxStates / nS) return rfail(nullptr, HJB_E_INVALID, "rollout: size overflow (%lld states x %d planes)", (long long)nS, n_planes);
    const int64_t n_lab = nS * n_planes;
    const int64_t n_ut = (int64_t)n_labels * n_u;
    const int64_t bad_u = first_nonfinite(u_table, n_ut, true);
    if (bad_u >= 0) return rfail(nullptr, HJB_E_INVALID, "rollout: u_table element %lld is not finite", (long long)bad_u);
    const int64_t lo = index_base, hi = (int64_t)index_base + n_labels;
    const int64_t bad = idx_bytes == 4 ? first_bad_label<int32_t>(labels, n_lab, lo, hi)
                      : idx_bytes == 2 ? first_bad_label<uint16_t>(labels, n_lab, lo, hi)
                                       : first_bad_label<uint8_t>(labels, n_lab, lo, hi);
    if (bad >= 0) {
        const int64_t v = idx_bytes == 4 ? ((const int32_t *)labels)[bad] : idx_bytes == 2 ? ((const uint16_t *)labels)[bad] : ((const uint8_t *)labels)[bad];
        return rfail(nullptr, HJB_E_INVALID, "rollout: label %lld at flat position %lld (state %lld, plane %lld) outside [%lld, %lld)",
                     (long long)v, (long long)bad, (long long)(bad % nS), (long long)(bad / nS), (long long)lo, (long long)hi);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return rfail(nullptr, HJB_E_DEVICE, "no HIP device visible (libhjbdp has no CPU fallback)");
    if (device < 0 || device >= ndev) return rfail(nullptr, HJB_E_INVALID, "rollout: device %d", device);

    std::shared_lock<std::shared_mutex> lk(g_capture_mu);
    if (hipSetDevice(device) != hipSuccess) return rfail(nullptr, HJB_E_DEVICE, "hipSetDevice failed");
    const size_t lab_bytes = (size_t)n_lab * idx_bytes, tab_bytes = (size_t)(2 * n_knots + n_ut) * sizeof(double);
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) return rfail(nullptr, HJB_E_DEVICE, "hipMemGetInfo failed");
    if (lab_bytes + tab_bytes + ((size_t)64 << 20) > fr)
        return rfail(nullptr, HJB_E_NOMEM, "rollout: %zu bytes of labels and tables, %zu free on device %d", lab_bytes + tab_bytes, fr, device);

    Rollout *ro = new Rollout;
    ro->device = device;
    ro->D = D;
    ro->idx_bytes = idx_bytes;
    ro->n_planes = n_planes;
    DRollout &R = ro->R;
    R.n_u = n_u;
    R.n_labels = n_labels;
    R.index_base = index_base;
    R.n_knots = (int32_t)n_knots;
    R.nS = nS;
    std::vector<double> kk(knots, knots + n_knots), rdx(n_knots, 0.0);
    int64_t s = 1, off = 0;
    for (int a = 0; a < D; ++a) {
        const double *k = kk.data() + off;
        for (int i = 0; i + 1 < n[a]; ++i) rdx[off + i] = 1.0 / (k[i + 1] - k[i]);     // as hjb_policy_lookup builds it
        const double hstep = (k[n[a] - 1] - k[0]) / (n[a] - 1);
        double dev = 0;
        for (int i = 0; i < n[a]; ++i) dev = std::max(dev, std::fabs(k[i] - (k[0] + i * hstep)));
        R.uniform[a] = dev <= 1.5 * hstep ? 1 : 0;
        R.x0[a] = k[0];
        R.inv_h[a] = 1.0 / hstep;
        R.n[a] = n[a];
        R.koff[a] = (int32_t)off;
        R.stride[a] = s;
        s *= n[a];
        off += n[a];
    }
    auto dev_upload = [&](const void *src, size_t bytes, void **out) -> int {
        void *d = nullptr;
        if (hipMalloc(&d, std::max<size_t>(bytes, 16)) != hipSuccess) return rfail(ro, HJB_E_NOMEM, "rollout: hipMalloc of %zu bytes failed", bytes);
        ro->allocs.push_back(d);
        if (hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) != hipSuccess) return rfail(ro, HJB_E_DEVICE, "rollout: upload failed");
        *out = d;
        return HJB_OK;
    };
    void *dk = nullptr, *dr = nullptr, *du = nullptr, *dl = nullptr;
    int st = dev_upload(kk.data(), kk.size() * sizeof(double), &dk);
    if (!st) st = dev_upload(rdx.data(), rdx.size() * sizeof(double), &dr);
    if (!st) st = dev_upload(u_table, (size_t)n_ut * sizeof(double), &du);
    if (!st) st = dev_upload(labels, lab_bytes, &dl);
    if (!st && hipStreamCreateWithFlags(&ro->stream, hipStreamNonBlocking) != hipSuccess) st = rfail(ro, HJB_E_DEVICE, "rollout: stream creation failed");
    if (st) {
        release(ro);
        delete ro;
        return st;
    }
    R.knots = (const double *)dk;
    R.rdx = (const double *)dr;
    R.u_table = (const double *)du;
    R.labels = dl;
    *rollout_out = ro;
    return HJB_OK;
}

int32_t hjb_rollout_set_model(void *rollout, const double *A, const double *B, const double *c, const double *q, const double *r) {
    Rollout *ro = (Rollout *)rollout;
    if (!ro || !A || !B) return rfail(ro, HJB_E_INVALID, "rollout: null argument (A and B are required)");
    std::lock_guard<std::mutex> g(ro->mu);
    const int D = ro->D, nu = ro->R.n_u;
    if (!all_finite(A, (int64_t)D * D)) return rfail(ro, HJB_E_INVALID, "rollout: A is not finite");
    if (!all_finite(B, (int64_t)D * nu)) return rfail(ro, HJB_E_INVALID, "rollout: B is not finite");
    if (!all_finite(c, D)) return rfail(ro, HJB_E_INVALID, "rollout: c is not finite");
    if (!all_finite(q, D)) return rfail(ro, HJB_E_INVALID, "rollout: q is not finite");
    if (!all_finite(r, nu)) return rfail(ro, HJB_E_INVALID, "rollout: r is not finite");
    DRollout &R = ro->R;
    std::memset(R.A, 0, sizeof R.A);
    std::memset(R.B, 0, sizeof R.B);
    std::memset(R.c, 0, sizeof R.c);
    std::memset(R.q, 0, sizeof R.q);
    std::memset(R.r, 0, sizeof R.r);
    std::memcpy(R.A, A, sizeof(double) * D * D);
    std::memcpy(R.B, B, sizeof(double) * D * nu);
    if (c) std::memcpy(R.c, c, sizeof(double) * D);
    if (q) std::memcpy(R.q, q, sizeof(double) * D);
    if (r) std::memcpy(R.r, r, sizeof(double) * nu);
    R.has_c = c ? 1 : 0;
    ro->model_set = true;
    return HJB_OK;
}

int32_t hjb_rollout_set_option(void *rollout, const char *key, int64_t value) {
    Rollout *ro = (Rollout *)rollout;
    if (!ro || !key) return rfail(ro, HJB_E_INVALID, "rollout: null argument");
    std::lock_guard<std::mutex> g(ro->mu);
    if (!strcmp(key, "chunk")) {
        if (value < 1 || value > kMaxChunk) return rfail(ro, HJB_E_INVALID, "rollout: chunk %lld not in 1..%lld", (long long)value, (long long)kMaxChunk);
        ro->chunk = value;
        return HJB_OK;
    }
    return rfail(ro, HJB_E_INVALID, "rollout: unknown option '%s'", key);
}

int32_t hjb_rollout_run(void *rollout, int32_t method, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj,
                        const double *X0, double *X_final, double *cost, double *X_path, double *U_path, double *device_ms) {
    Rollout *ro = (Rollout *)rollout;
    if (!ro) return rfail(nullptr, HJB_E_INVALID, "rollout: null handle");
    std::lock_guard<std::mutex> g(ro->mu);
    if (method != HJB_LOOKUP_NEAREST && method != HJB_LOOKUP_LINEAR) return rfail(ro, HJB_E_INVALID, "rollout: method %d", method);
    if (n_steps < 0) return rfail(ro, HJB_E_INVALID, "rollout: n_steps=%d < 0", n_steps);
    if (n_traj < 0) return rfail(ro, HJB_E_INVALID, "rollout: n_traj=%lld < 0", (long long)n_traj);
    if (!ro->model_set) return rfail(ro, HJB_E_INVALID, "rollout: run before hjb_rollout_set_model");
    if (n_steps > 0 && !plane_of_step) return rfail(ro, HJB_E_INVALID, "rollout: null plane_of_step");
    for (int k = 0; k < n_steps; ++k)
        if (plane_of_step[k] < 0 || plane_of_step[k] >= ro->n_planes)
            return rfail(ro, HJB_E_INVALID, "rollout: plane_of_step[%d] = %d outside [0, %d)", k, plane_of_step[k], ro->n_planes);
    if (device_ms) *device_ms = 0.0;
    if (n_traj == 0) return HJB_OK;
    if (!X0 || !X_final) return rfail(ro, HJB_E_INVALID, "rollout: null X0 / X_final");
    const int D = ro->D, nu = ro->R.n_u;
    if (n_traj > INT64_MAX / (D * ((int64_t)n_steps + 1)) / 8) return rfail(ro, HJB_E_INVALID, "rollout: size overflow (n_traj x D x n_steps)");
    const int64_t bad = first_nonfinite(X0, (int64_t)D * n_traj, true);
    if (bad >= 0) return rfail(ro, HJB_E_INVALID, "rollout: X0 element %lld is not finite", (long long)bad);

    std::shared_lock<std::shared_mutex> lk(g_capture_mu);
    if (hipSetDevice(ro->device) != hipSuccess) return rfail(ro, HJB_E_DEVICE, "hipSetDevice failed");
    const int64_t nc_max = std::min(n_traj, ro->chunk);
    const size_t xb = (size_t)nc_max * D * sizeof(double);
    const size_t xpb = X_path ? (size_t)nc_max * D * ((size_t)n_steps + 1) * sizeof(double) : 0;
    const size_t upb = U_path ? (size_t)nc_max * nu * (size_t)n_steps * sizeof(double) : 0;
    const size_t cb = cost ? (size_t)nc_max * sizeof(double) : 0;
    const size_t pb = (size_t)std::max(n_steps, 1) * sizeof(int32_t);
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) return rfail(ro, HJB_E_DEVICE, "hipMemGetInfo failed");
    const size_t need = 2 * xb + xpb + upb + cb + pb;
    if (need + ((size_t)64 << 20) > fr)
        return rfail(ro, HJB_E_NOMEM, "rollout: a chunk of %lld trajectories needs %zu bytes, %zu free (lower option \"chunk\")",
                     (long long)nc_max, need, fr);
    void *bufs[6] = {};
    auto done = [&](int code) {
        for (void *p : bufs) if (p) (void)hipFree(p);
        return code;
    };
    const size_t sizes[6] = {xb, xb, cb, xpb, upb, pb};
    for (int b = 0; b < 6; ++b)
        if (sizes[b] && hipMalloc(&bufs[b], sizes[b]) != hipSuccess) return done(rfail(ro, HJB_E_NOMEM, "rollout: hipMalloc of %zu bytes failed", sizes[b]));
    double *dX0 = (double *)bufs[0], *dXf = (double *)bufs[1], *dC = (double *)bufs[2], *dXp = (double *)bufs[3], *dUp = (double *)bufs[4];
    hipStream_t st = ro->stream;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess && n_steps > 0) e = hipMemcpyAsync(bufs[5], plane_of_step, pb, hipMemcpyHostToDevice, st);
    DRollout R = ro->R;
    R.plane_of_step = (const int32_t *)bufs[5];
    R.n_steps = n_steps;
    const size_t lds = (size_t)(2 * (int64_t)R.n_knots + (int64_t)R.n_labels * nu) * sizeof(double);
    const bool lds_on = lds <= kLdsMax;
    double ms_total = 0;
    for (int64_t i0 = 0; e == hipSuccess && i0 < n_traj; i0 += nc_max) {
        const int64_t nc = std::min(nc_max, n_traj - i0);
        e = hipMemcpyAsync(dX0, X0 + D * i0, (size_t)nc * D * sizeof(double), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) break;
        (void)hipEventRecord(e0, st);
        switch (ro->idx_bytes) {
            case 1: launch_m<uint8_t>(D, method, lds_on, R, nc, lds, st, dX0, dXf, dC, dXp, dUp); break;
            case 2: launch_m<uint16_t>(D, method, lds_on, R, nc, lds, st, dX0, dXf, dC, dXp, dUp); break;
            default: launch_m<int32_t>(D, method, lds_on, R, nc, lds, st, dX0, dXf, dC, dXp, dUp); break;
        }
        e = hipGetLastError();
        if (e != hipSuccess) break;
        (void)hipEventRecord(e1, st);
        e = hipMemcpyAsync(X_final + D * i0, dXf, (size_t)nc * D * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && cost) e = hipMemcpyAsync(cost + i0, dC, (size_t)nc * sizeof(double), hipMemcpyDeviceToHost, st);
        // paths: [nc, rows] on the device -> columns i0 .. i0+nc of [n_traj, rows] on the host
        if (e == hipSuccess && X_path)
            e = hipMemcpy2DAsync(X_path + i0, (size_t)n_traj * sizeof(double), dXp, (size_t)nc * sizeof(double), (size_t)nc * sizeof(double),
                                 (size_t)D * (n_steps + 1), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && U_path && n_steps > 0)
            e = hipMemcpy2DAsync(U_path + i0, (size_t)n_traj * sizeof(double), dUp, (size_t)nc * sizeof(double), (size_t)nc * sizeof(double),
                                 (size_t)nu * n_steps, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        float ms = 0;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        ms_total += ms;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return done(rfail(ro, HJB_E_DEVICE, "hjb_rollout_run: %s", hipGetErrorString(e)));
    }
    if (device_ms) *device_ms = ms_total;
    return done(HJB_OK);
}

int32_t hjb_rollout_destroy(void *rollout) {
    Rollout *ro = (Rollout *)rollout;
    if (!ro) return HJB_OK;
    {
        std::lock_guard<std::mutex> g(ro->mu);
        std::shared_lock<std::shared_mutex> lk(g_capture_mu);
        (void)hipSetDevice(ro->device);
        if (ro->stream) (void)hipStreamSynchronize(ro->stream);
        release(ro);
    }
    delete ro;
    return HJB_OK;
}

const char *hjb_rollout_last_error(void *rollout) {
    Rollout *ro = (Rollout *)rollout;
    return ro ? ro->err.c_str() : g_last_error.c_str();
}

}  // extern "C"
