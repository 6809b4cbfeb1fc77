#include "stage_disturb_impl.h"
namespace hjb {
int stage_disturb_f32(const StageArgs &a, const DParams *dpq, const void *dist, const void *labels, int32_t *bad_label) { return disturb_go<float, float, float>(a, dpq, dist, labels, bad_label); }
}
