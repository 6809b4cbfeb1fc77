// stage_evaluate.hip - the fixed-label stage (kernels_evaluate.h): the cost of a given policy, one stage
// One translation unit per stage-kernel family (hjbdp_launch.h): built in parallel by __graft_entry__.build().
#include "hjbdp_launch.h"
#include "kernels_evaluate.h"

namespace hjb {

template <typename T, typename TJ, bool TABLED, typename IX, bool M24>
static int go(const StageArgs &a, const void *labels, int32_t *bad_label, const EvalDiv &dv) {
    const dim3 g(a.grid), b(a.block);
    const TJ *Jn = (const TJ *)a.Jn;
    TJ *Jo = (TJ *)a.Jo;
    switch (a.D) {
        case 1: hipLaunchKernelGGL((k_evaluate<T, TJ, 1, TABLED, IX, M24>), g, b, 0, a.st, a.dp, a.dtb, Jn, labels, Jo, bad_label, dv); break;
        case 2: hipLaunchKernelGGL((k_evaluate<T, TJ, 2, TABLED, IX, M24>), g, b, 0, a.st, a.dp, a.dtb, Jn, labels, Jo, bad_label, dv); break;
        case 3: hipLaunchKernelGGL((k_evaluate<T, TJ, 3, TABLED, IX, M24>), g, b, 0, a.st, a.dp, a.dtb, Jn, labels, Jo, bad_label, dv); break;
        case 4: hipLaunchKernelGGL((k_evaluate<T, TJ, 4, TABLED, IX, M24>), g, b, 0, a.st, a.dp, a.dtb, Jn, labels, Jo, bad_label, dv); break;
        case 5: hipLaunchKernelGGL((k_evaluate<T, TJ, 5, TABLED, IX, M24>), g, b, 0, a.st, a.dp, a.dtb, Jn, labels, Jo, bad_label, dv); break;
        case 6: hipLaunchKernelGGL((k_evaluate<T, TJ, 6, TABLED, IX, M24>), g, b, 0, a.st, a.dp, a.dtb, Jn, labels, Jo, bad_label, dv); break;
        default: return 1;
    }
    return 0;
}

template <bool TABLED, typename IX, bool M24>
static int by_dtype(const StageArgs &a, const void *labels, int32_t *bad_label, const EvalDiv &dv) {
    if (a.dtype == HJB_F16S) return go<float, _Float16, TABLED, IX, M24>(a, labels, bad_label, dv);
    if (a.dtype == HJB_F32) return go<float, float, TABLED, IX, M24>(a, labels, bad_label, dv);
    return go<double, double, TABLED, IX, M24>(a, labels, bad_label, dv);
}

// a.idx32: every state index, J offset and table offset fits 31 bits (the host checked): the 32-bit form of the same kernel;
// mul24: ... and every stride, index and quotient it multiplies is below 2^24
int stage_evaluate(const StageArgs &a, bool tabled, bool mul24, const void *labels, int32_t *bad_label, const EvalDiv &dv) {
    if (a.idx32 && mul24) return tabled ? by_dtype<true, uint32_t, true>(a, labels, bad_label, dv) : by_dtype<false, uint32_t, true>(a, labels, bad_label, dv);
    if (a.idx32) return tabled ? by_dtype<true, uint32_t, false>(a, labels, bad_label, dv) : by_dtype<false, uint32_t, false>(a, labels, bad_label, dv);
    return tabled ? by_dtype<true, int64_t, false>(a, labels, bad_label, dv) : by_dtype<false, int64_t, false>(a, labels, bad_label, dv);
}

}  // namespace hjb
