// stage_ctrldist.hip - variant 8, per-control form (K32, kernels_ctrldist.h): the stage of a handle with a control-dependent
// disturbance, min form and fixed-label form.  One translation unit per (arithmetic type, J storage type, query type) -
// stage_ctrldist_f32 / _f16 / _f64 / _q64_f32 / _q64_f16.hip, as stage_disturb_*.hip - this one only dispatches.
#include "hjbdp_launch.h"

namespace hjb {

int stage_ctrldist_f32(const StageArgs &a, const DParams *dpq, const void *dist, const void *table, const void *labels, int32_t *bad_label);
int stage_ctrldist_f16(const StageArgs &a, const DParams *dpq, const void *dist, const void *table, const void *labels, int32_t *bad_label);
int stage_ctrldist_f64(const StageArgs &a, const DParams *dpq, const void *dist, const void *table, const void *labels, int32_t *bad_label);
int stage_ctrldist_q64_f32(const StageArgs &a, const DParams *dpq, const void *dist, const void *table, const void *labels, int32_t *bad_label);
int stage_ctrldist_q64_f16(const StageArgs &a, const DParams *dpq, const void *dist, const void *table, const void *labels, int32_t *bad_label);

// q64: HJB_TAB_F64 - dpq is the float64 shadow of the axes and the table's entries are doubles; else dpq == a.dp
int stage_ctrldist(const StageArgs &a, bool q64, const DParams *dpq, const void *dist, const void *table, const void *labels, int32_t *bad_label) {
    if (a.dtype == HJB_F64) return q64 ? 1 : stage_ctrldist_f64(a, dpq, dist, table, labels, bad_label);
    if (a.dtype == HJB_F16S) return q64 ? stage_ctrldist_q64_f16(a, dpq, dist, table, labels, bad_label) : stage_ctrldist_f16(a, dpq, dist, table, labels, bad_label);
    return q64 ? stage_ctrldist_q64_f32(a, dpq, dist, table, labels, bad_label) : stage_ctrldist_f32(a, dpq, dist, table, labels, bad_label);
}

}  // namespace hjb
