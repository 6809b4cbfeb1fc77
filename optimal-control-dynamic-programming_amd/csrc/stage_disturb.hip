// stage_disturb.hip - variant 8 (K24, kernels_disturb.h): the stage of a handle with a disturbance, min form and fixed-label form.
// One translation unit per (arithmetic type, J storage type, query type) - stage_disturb_f32 / _f16 / _f64 / _q64_f32 / _q64_f16.hip -
// built in parallel by __graft_entry__.build(); this one only dispatches.
#include "hjbdp_launch.h"

namespace hjb {

int stage_disturb_f32(const StageArgs &a, const DParams *dpq, const void *dist, const void *labels, int32_t *bad_label);
int stage_disturb_f16(const StageArgs &a, const DParams *dpq, const void *dist, const void *labels, int32_t *bad_label);
int stage_disturb_f64(const StageArgs &a, const DParams *dpq, const void *dist, const void *labels, int32_t *bad_label);
int stage_disturb_q64_f32(const StageArgs &a, const DParams *dpq, const void *dist, const void *labels, int32_t *bad_label);
int stage_disturb_q64_f16(const StageArgs &a, const DParams *dpq, const void *dist, const void *labels, int32_t *bad_label);

// q64: HJB_TAB_F64 - dpq is the float64 shadow of the axes and the block's offsets are doubles; else dpq == a.dp
int stage_disturb(const StageArgs &a, bool q64, const DParams *dpq, const void *dist, const void *labels, int32_t *bad_label) {
    if (a.dtype == HJB_F64) return q64 ? 1 : stage_disturb_f64(a, dpq, dist, labels, bad_label);
    if (a.dtype == HJB_F16S) return q64 ? stage_disturb_q64_f16(a, dpq, dist, labels, bad_label) : stage_disturb_f16(a, dpq, dist, labels, bad_label);
    return q64 ? stage_disturb_q64_f32(a, dpq, dist, labels, bad_label) : stage_disturb_f32(a, dpq, dist, labels, bad_label);
}

}  // namespace hjb
