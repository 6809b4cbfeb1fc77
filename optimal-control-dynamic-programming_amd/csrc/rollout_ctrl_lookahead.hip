// rollout_ctrl_lookahead.hip - K35's 24 nominal-plant instantiations (kernels_rollout_ctrl_lookahead.h: D x value type x LDS, FLY =
// false) in a unit of their own, behind launch_rollout_ctrl_lookahead (called by hjb_rollout_run_control_lookahead in
// rollout_ctrl_lookahead_host.hip).
#include "kernels_rollout_ctrl_lookahead.h"

namespace hjb {

hipError_t launch_rollout_ctrl_lookahead(int val_bytes, bool lds_on, int D, const DCtrlLook &A, size_t lds, hipStream_t st) {
    return launch_rollout_ctrl_lookahead_form<false>(val_bytes, lds_on, D, A, lds, st);
}

}  // namespace hjb
