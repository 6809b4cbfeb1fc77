// rollout_ctrl_lookahead_fly.hip - K35's 24 actuator-plant instantiations (kernels_rollout_ctrl_lookahead.h: D x value type x LDS,
// FLY = true) in a unit of their own, behind launch_rollout_ctrl_lookahead_fly (called by hjb_rollout_run_control_lookahead in
// rollout_ctrl_lookahead_host.hip).
#include "kernels_rollout_ctrl_lookahead.h"

namespace hjb {

hipError_t launch_rollout_ctrl_lookahead_fly(int val_bytes, bool lds_on, int D, const DCtrlLook &A, size_t lds, hipStream_t st) {
    return launch_rollout_ctrl_lookahead_form<true>(val_bytes, lds_on, D, A, lds, st);
}

}  // namespace hjb
