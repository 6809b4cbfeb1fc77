#include "stage_ctrldist_impl.h"
namespace hjb {
int stage_ctrldist_f64(const StageArgs &a, const DParams *dpq, const void *dist, const void *table, const void *labels, int32_t *bad_label) { return ctrldist_go<double, double, double>(a, dpq, dist, table, labels, bad_label); }
}
