// lbk8s_policies.hip — the kernels of the on-device policies LB_POLICY_ROUND_ROBIN ..
// LB_POLICY_REWARD_GREEDY (include/lbk8s.h) that are not k_policy's (lbk8s_env.hip):
//   * lb_policy(LB_POLICY_REWARD_GREEDY): the argmax over every action of the reward lb_step
//     would return (whatif_accept_reward, lbk8s_common.h), O(E^2) per env.  In the slice
//     layout with E > 8 lanes over the endpoints, W = 16 / 32 / 64 per env as the slice
//     geometry picks them (k_policy_rg_slice: the other endpoints' history counters by
//     shuffles, the slice's (value, index) reduction); else one lane per env
//     (k_policy_rg_lane, through eidx: both layouts);
//   * lb_rollout under the four kinds: k_rollout_slice_k8s (lbk8s_slice.h) and the
//     k_rollout_tpe<NB, KIND, PRE> instantiations of KIND = 4..7 (lbk8s_tpe.h).  There are no
//     lean or image rollout kernels for these kinds.
// Not compiled next to the env (lbk8s_env_steps.hip is the build's critical path, and its slice
// kernels change their code with what else the module holds): the instantiations need only the
// kernel headers and lbk8s_host.h, and lbk8s_learn.hip, the build's shortest unit, includes this
// file at its end.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "lbk8s.h"
#include "lbk8s_common.h"
#include "lbk8s_host.h"
#include "lbk8s_slice.h"
#include "lbk8s_tpe.h"

namespace lbk {

// E <= 8, either layout: one lane per env, the env's endpoints in registers
__global__ __launch_bounds__(BLOCK) void k_policy_rg_lane(Params p, int32_t* out) {
    const int64_t env = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (env >= p.B) return;
    double lat0[TPE_E];
    uint32_t em[TPE_E], ed[TPE_E];
#pragma unroll
    for (int e = 0; e < TPE_E; ++e) {
        const int64_t i = eidx(p, env, e < p.E ? e : 0);
        lat0[e] = e < p.E ? p.lat0[i] : 0.0;
        em[e] = e < p.E ? p.emeta[i] : 0u;
        ed[e] = e < p.E ? p.edyn[i] : 0u;
    }
    TEnv v;  // the policy's view
    v.s = sc_unpack(p.sc[env]);
    v.topo = p.topo[env];
    v.acc2 = p.acc2[env];
    out[env] = tpe_policy<LB_POLICY_REWARD_GREEDY>(p, env, v, lat0, em, ed);
}

// the slice layout: one W-lane slice per env, lane l its endpoints l + k W
template <int W, int EPL>
__global__ __launch_bounds__(BLOCK) void k_policy_rg_slice(Params p, int32_t* out) {
    const int lane = threadIdx.x % W;
    const int64_t env = (int64_t)blockIdx.x * (BLOCK / W) + threadIdx.x / W;
    if (env >= p.B) return;
    SEnv<EPL> v;
    slice_load<W, EPL>(p, env, lane, v);
    const int a = slice_policy_k8s<W, EPL>(p, lane, v, LB_POLICY_REWARD_GREEDY);
    if (lane == 0) out[env] = a;
}

int launch_policy_reward_greedy(const Params& p, const Geo& g, int32_t* actions_out, hipStream_t s) {
    if (g.tpe || p.E <= TPE_E) {
        hipLaunchKernelGGL(k_policy_rg_lane, dim3(env_blocks(p.B)), dim3(BLOCK), 0, s, p, actions_out);
        return check_launch();
    }
    LB_DISPATCH_SLICE(g.W, g.EPL, {
        hipLaunchKernelGGL((k_policy_rg_slice<W, EPL>), dim3(slice_blocks(p.B, W)), dim3(BLOCK), 0, s, p, actions_out);
    });
    return check_launch();
}

int launch_rollout_k8s(const Params& p, const Geo& g, int policy, int steps, bool pre, int32_t* actions_out,
                       hipStream_t s) {
    if (!g.tpe) {
        LB_DISPATCH_SLICE(g.W, g.EPL, {
            hipLaunchKernelGGL((k_rollout_slice_k8s<W, EPL>), dim3(slice_blocks(p.B, W)), dim3(BLOCK), 0, s, p, policy,
                               steps, actions_out);
        });
        return check_launch();
    }
    // thread-per-env, N <= 64 (the caller's condition); launch shape as the kinds 0..3
    const bool small = p.B <= SMALL_TPE_MAX_B;
    const dim3 grid(small ? (unsigned)((p.B + 63) / 64) : env_blocks(p.B)), block(small ? 64 : BLOCK);
    auto launch = [&](auto kind) {
        constexpr int KIND = decltype(kind)::value;
        if (small && pre) hipLaunchKernelGGL((k_rollout_tpe<64, KIND, true>), grid, block, 0, s, p, steps, actions_out);
        else if (small) hipLaunchKernelGGL((k_rollout_tpe<64, KIND, false>), grid, block, 0, s, p, steps, actions_out);
        else if (pre) hipLaunchKernelGGL((k_rollout_tpe<BLOCK, KIND, true>), grid, block, 0, s, p, steps, actions_out);
        else hipLaunchKernelGGL((k_rollout_tpe<BLOCK, KIND, false>), grid, block, 0, s, p, steps, actions_out);
    };
    switch (policy) {
    case LB_POLICY_ROUND_ROBIN: launch(std::integral_constant<int, LB_POLICY_ROUND_ROBIN>{}); break;
    case LB_POLICY_LEAST_LOADED: launch(std::integral_constant<int, LB_POLICY_LEAST_LOADED>{}); break;
    case LB_POLICY_LEAST_LATENCY: launch(std::integral_constant<int, LB_POLICY_LEAST_LATENCY>{}); break;
    case LB_POLICY_REWARD_GREEDY: launch(std::integral_constant<int, LB_POLICY_REWARD_GREEDY>{}); break;
    default: return fail("unknown policy kind");
    }
    return check_launch();
}

}  // namespace lbk
