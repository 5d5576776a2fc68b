// lbk8s_steps256.hip — the one-launch greedy evaluation for envs of up to 256 endpoints
// (lbk8s_steps256.h) and its entry points: lb_eval_steps256, the superset of lb_eval_steps64
// (lbk8s_steps64.hip), and its _supported query.
//
// Compiled at the end of lbk8s_ds_train.hip, after lbk8s_steps64.hip (the set of units stays as
// it was: csrc/Makefile).
// Public ABI: include/lbk8s.h; the host helpers: lbk8s_host.h.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "lbk8s.h"
#include "lbk8s_common.h"
#include "lbk8s_deepsets.h"
#include "lbk8s_steps256.h"
#include "lbk8s_host.h"
#include "lbk8s_steps_host.h"

using namespace lbk;

namespace {
// lb_eval_steps256's shape (a property of the shape only, never of the device's CU count):
// whatever lb_eval_steps64 takes; or Philox draws, a forward over exactly the env's actions,
// 1..32,767 envs in the slice layout of 64 lanes with 2 or 4 endpoints each, R <= 257
bool steps256_fusable(const lb_config* cfg, int64_t num_envs, int32_t num_elements) {
    if (lb_eval_steps64_supported(cfg, num_envs, num_elements) == 1) return true;
    const int32_t A = cfg->num_endpoints + (cfg->rejection_allowed ? 1 : 0);
    if (num_envs < 1 || num_envs >= WIDE_SLICE_MAX_B || cfg->rng_mode != LB_RNG_PHILOX || num_elements != A) return false;
    const Geo g = geometry(cfg, num_envs);
    return !g.tpe && g.W == 64 && (g.EPL == 2 || g.EPL == 4) && num_elements <= STEPS256_MAX_R;
}
}  // namespace

extern "C" {

int lb_eval_steps256_supported(const lb_config* cfg, int64_t num_envs, int32_t num_elements) {
    if (validate(cfg)) return 0;
    return steps256_fusable(cfg, num_envs, num_elements) ? 1 : 0;
}

int lb_eval_steps256(const float* frag, float* obs, void* state, const lb_config* cfg, int64_t num_envs,
                     int32_t num_elements, const uint8_t* masks, int32_t steps, int32_t* actions_all,
                     float* rewards_all, uint8_t* dones_all, int32_t* actions_out, float* reward_out, uint8_t* done_out,
                     double* ep_stats_out, double* ep_sum, double* ep_cnt, float* ret32, float* ep_r32, int64_t tag0,
                     double* log, int64_t cap, uint32_t* count, void* stream) {
    if (int r = validate(cfg)) return r;
    const EvalStepsCall c{frag, obs, state, cfg, num_envs, num_elements, masks, steps, actions_all, rewards_all, dones_all,
                          actions_out, reward_out, done_out, ep_stats_out,
                          {ep_sum, ep_cnt, ret32, ep_r32, tag0, log, cap, count}, stream};
    if (int rc = eval_steps_check("lb_eval_steps256", c)) return rc;
    if (!steps256_fusable(cfg, num_envs, num_elements)) return steps_unsupported("lb_eval_steps256", "evaluation");
    if (lb_eval_steps64_supported(cfg, num_envs, num_elements)) return eval_steps64_launch(c);  // E <= 64
    DSParams d;
    Params e;
    EvalSteps r;
    eval_steps_params(c, d, e, r);
    const Geo g = geometry(cfg, num_envs);
    const bool chunk = num_elements > LB_DS_MAX_ELEMENTS;  // (lb_ds_q_argmax's rule: the chunked forward)
    const unsigned grid = ds_grid_spread(num_envs);        // a wave per env
    const hipStream_t s = (hipStream_t)stream;
    if (!chunk && g.EPL == 2) hipLaunchKernelGGL((k_eval_steps256<2, false>), dim3(grid), dim3(DS_BLOCK), 0, s, d, e, r);
    else if (chunk && g.EPL == 2) hipLaunchKernelGGL((k_eval_steps256<2, true>), dim3(grid), dim3(DS_BLOCK), 0, s, d, e, r);
    else if (chunk && g.EPL == 4) hipLaunchKernelGGL((k_eval_steps256<4, true>), dim3(grid), dim3(DS_BLOCK), 0, s, d, e, r);
    else return fail("lb_eval_steps256: unsupported geometry");
    return check_launch();
}

}  // extern "C"
