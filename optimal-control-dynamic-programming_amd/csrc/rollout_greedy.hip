// rollout_greedy.hip - K26's 24 instantiations (kernels_rollout_greedy.h: D x value type x LDS) in a unit of their own, behind
// launch_rollout_greedy (called by hjb_rollout_run_greedy in rollout.hip).
#include "kernels_rollout_greedy.h"
#include "rollout_dispatch.h"

namespace hjb {

hipError_t launch_rollout_greedy(int val_bytes, bool lds_on, int D, const DGreedy &G, size_t lds, hipStream_t st) {
    const dim3 b(256), g((unsigned)((G.nc + 255) / 256));
    with_bool(val_bytes == 4, [&](auto f) {
        with_bool(lds_on, [&](auto l) {
            with_dim(D, [&](auto d) {
                using TV = std::conditional_t<decltype(f)::value, float, double>;
                constexpr bool LDS = decltype(l)::value;
                hipLaunchKernelGGL((k_rollout_greedy<decltype(d)::value, TV, LDS>), g, b, LDS ? lds : 0, st, G);
            });
        });
    });
    return hipGetLastError();
}

}  // namespace hjb
