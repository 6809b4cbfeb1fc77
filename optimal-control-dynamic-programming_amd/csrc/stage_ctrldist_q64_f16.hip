#include "stage_ctrldist_impl.h"
namespace hjb {
int stage_ctrldist_q64_f16(const StageArgs &a, const DParams *dpq, const void *dist, const void *table, const void *labels, int32_t *bad_label) { return ctrldist_go<float, _Float16, double>(a, dpq, dist, table, labels, bad_label); }
}
