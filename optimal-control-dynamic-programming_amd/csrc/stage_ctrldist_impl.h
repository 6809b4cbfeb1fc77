// stage_ctrldist_impl.h - the instantiations of k_backup_ctrldist for one (arithmetic type, J storage type, query type): see stage_ctrldist.hip
#pragma once
#include "hjbdp_launch.h"
#include "kernels_ctrldist.h"

namespace hjb {

template <typename T, typename TJ, typename TQ, typename IX, bool FIXED>
static int ctrldist_go_d(const StageArgs &a, const DParams *dpq, const void *dist, const void *table, const void *labels, int32_t *bad_label) {
    const dim3 g(a.grid), b(a.block);
    const TJ *Jn = (const TJ *)a.Jn;
    TJ *Jo = (TJ *)a.Jo;
    const DDisturb<TQ, T> *dw = (const DDisturb<TQ, T> *)dist;
    const TQ *dt = (const TQ *)table;
    switch (a.D) {
        case 1: hipLaunchKernelGGL((k_backup_ctrldist<T, TJ, TQ, 1, IX, FIXED>), g, b, 0, a.st, a.dp, dpq, dw, dt, Jn, Jo, a.idx, labels, bad_label); break;
        case 2: hipLaunchKernelGGL((k_backup_ctrldist<T, TJ, TQ, 2, IX, FIXED>), g, b, 0, a.st, a.dp, dpq, dw, dt, Jn, Jo, a.idx, labels, bad_label); break;
        case 3: hipLaunchKernelGGL((k_backup_ctrldist<T, TJ, TQ, 3, IX, FIXED>), g, b, 0, a.st, a.dp, dpq, dw, dt, Jn, Jo, a.idx, labels, bad_label); break;
        case 4: hipLaunchKernelGGL((k_backup_ctrldist<T, TJ, TQ, 4, IX, FIXED>), g, b, 0, a.st, a.dp, dpq, dw, dt, Jn, Jo, a.idx, labels, bad_label); break;
        case 5: hipLaunchKernelGGL((k_backup_ctrldist<T, TJ, TQ, 5, IX, FIXED>), g, b, 0, a.st, a.dp, dpq, dw, dt, Jn, Jo, a.idx, labels, bad_label); break;
        case 6: hipLaunchKernelGGL((k_backup_ctrldist<T, TJ, TQ, 6, IX, FIXED>), g, b, 0, a.st, a.dp, dpq, dw, dt, Jn, Jo, a.idx, labels, bad_label); break;
        default: return 1;
    }
    return 0;
}

// a.idx32: every state index and J offset fits 31 bits (the host checked); labels: the fixed-label form
template <typename T, typename TJ, typename TQ>
static int ctrldist_go(const StageArgs &a, const DParams *dpq, const void *dist, const void *table, const void *labels, int32_t *bad_label) {
    if (labels) return a.idx32 ? ctrldist_go_d<T, TJ, TQ, uint32_t, true>(a, dpq, dist, table, labels, bad_label)
                               : ctrldist_go_d<T, TJ, TQ, int64_t, true>(a, dpq, dist, table, labels, bad_label);
    return a.idx32 ? ctrldist_go_d<T, TJ, TQ, uint32_t, false>(a, dpq, dist, table, labels, bad_label)
                   : ctrldist_go_d<T, TJ, TQ, int64_t, false>(a, dpq, dist, table, labels, bad_label);
}

}  // namespace hjb
