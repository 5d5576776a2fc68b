// lbk8s_steps256.hip — the one-launch greedy evaluation, DQN train period and PPO rollout for envs
// of up to 256 endpoints (lbk8s_steps256.h, lbk8s_dqn256.h, lbk8s_ppo256.h) and their entry points:
// lb_eval_steps256, lb_dqn_steps256 and lb_ppo_steps256, the supersets of lb_eval_steps64,
// lb_dqn_steps64 and lb_ppo_steps64 (lbk8s_steps64.hip), and their _supported queries.
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
#include "lbk8s_dqn256.h"
#include "lbk8s_ppo256.h"
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

// lb_dqn_steps256's shape: lb_dqn_steps64's (which asks neither for Philox mode nor for the action
// count on the 16-lane shapes: the launch refuses those), or the rule above
bool dqn_steps256_fusable(const lb_config* cfg, int64_t num_envs, int32_t num_elements) {
    return lb_dqn_steps64_supported(cfg, num_envs, num_elements) == 1 || steps256_fusable(cfg, num_envs, num_elements);
}

// lb_ppo_steps256's shape: lb_ppo_steps64's, or the rule above (the sampling forward in place of
// the greedy one)
bool ppo_steps256_fusable(const lb_config* cfg, int64_t num_envs, int32_t num_elements) {
    return lb_ppo_steps64_supported(cfg, num_envs, num_elements) == 1 || steps256_fusable(cfg, num_envs, num_elements);
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

int lb_dqn_steps256_supported(const lb_config* cfg, int64_t num_envs, int32_t num_elements) {
    if (validate(cfg)) return 0;
    return dqn_steps256_fusable(cfg, num_envs, num_elements) ? 1 : 0;
}

int lb_dqn_steps256(const float* frag, float* obs, int64_t num_envs, int32_t num_elements, const uint8_t* masks,
                    void* state, const lb_config* cfg, const lb_dqn_explore* ex, int32_t* actions_out,
                    float* next_obs_out, float* reward_out, uint8_t* done_out, float* terminal_obs_out,
                    double* ep_stats_out, int64_t slots, const int64_t* pos_in, int64_t* pos_out, float* rb_obs,
                    float* rb_next_obs, int64_t* rb_actions, float* rb_rewards, float* rb_dones, double* ep_sum,
                    double* ep_cnt, int32_t steps, int32_t* sync, void* stream) {
    if (int r = validate(cfg)) return r;
    const DQNStepsCall c{frag, obs, num_envs, num_elements, masks, state, cfg, ex, actions_out, next_obs_out, reward_out,
                         done_out, terminal_obs_out, ep_stats_out, slots, pos_in, pos_out, rb_obs, rb_next_obs,
                         rb_actions, rb_rewards, rb_dones, ep_sum, ep_cnt, steps, sync, stream};
    if (int rc = dqn_period_check("lb_dqn_steps256", c)) return rc;
    if (int rc = dqn_steps_check("lb_dqn_steps256", c, false)) return rc;
    if (!dqn_steps256_fusable(cfg, num_envs, num_elements)) return steps_unsupported("lb_dqn_steps256", "vector step");
    if (lb_dqn_steps64_supported(cfg, num_envs, num_elements)) return dqn_steps64_launch(c);  // E <= 64
    DSParams d;
    Params e;
    DQNReplay r;
    dqn_steps_params(c, d, e, r);
    const Geo g = geometry(cfg, num_envs);
    const bool chunk = num_elements > LB_DS_MAX_ELEMENTS;  // (lb_ds_q_argmax's rule: the chunked forward)
    const unsigned grid = ds_grid_spread(num_envs);        // a wave per env
    const hipStream_t s = (hipStream_t)stream;
    const int n = (int)steps;
    if (!chunk && g.EPL == 2)
        hipLaunchKernelGGL((k_dqn_steps256<2, false>), dim3(grid), dim3(DS_BLOCK), 0, s, d, e, r, n, sync);
    else if (chunk && g.EPL == 2)
        hipLaunchKernelGGL((k_dqn_steps256<2, true>), dim3(grid), dim3(DS_BLOCK), 0, s, d, e, r, n, sync);
    else if (chunk && g.EPL == 4)
        hipLaunchKernelGGL((k_dqn_steps256<4, true>), dim3(grid), dim3(DS_BLOCK), 0, s, d, e, r, n, sync);
    else return fail("lb_dqn_steps256: unsupported geometry");
    return check_launch();
}

int lb_ppo_steps256_supported(const lb_config* cfg, int64_t num_envs, int32_t num_elements) {
    if (validate(cfg)) return 0;
    return ppo_steps256_fusable(cfg, num_envs, num_elements) ? 1 : 0;
}

int lb_ppo_steps256(const float* frag, const float* obs, void* state, const lb_config* cfg, int64_t num_envs,
                    int32_t num_elements, int32_t steps, int32_t store_rows, const float* uniforms, float* actions_f32,
                    float* logprobs, float* values, float* rewards, float* obs_next, float* dones_next,
                    float* last_obs, float* last_done, int32_t* actions_out, uint8_t* done_out, double* ep_stats_out,
                    double* ep_sum, double* ep_cnt, float* ret32, float* ep_r32, int64_t tag0, double* log, int64_t cap,
                    uint32_t* count, void* stream) {
    if (int r = validate(cfg)) return r;
    const PPOStepsCall c{frag, obs, state, cfg, num_envs, num_elements, steps, store_rows, uniforms, actions_f32, logprobs,
                         values, rewards, obs_next, dones_next, last_obs, last_done, actions_out, done_out, ep_stats_out,
                         {ep_sum, ep_cnt, ret32, ep_r32, tag0, log, cap, count}, stream};
    if (int rc = ppo_steps_check("lb_ppo_steps256", c)) return rc;
    if (!ppo_steps256_fusable(cfg, num_envs, num_elements)) return steps_unsupported("lb_ppo_steps256", "rollout");
    if (lb_ppo_steps64_supported(cfg, num_envs, num_elements)) return ppo_steps64_launch(c);  // E <= 64
    DSParams d;
    Params e;
    PPOSteps r;
    ppo_steps_params(c, d, e, r);
    const Geo g = geometry(cfg, num_envs);
    const bool chunk = num_elements > LB_DS_MAX_ELEMENTS;  // (lb_ds_sample's rule: the chunked forward)
    const unsigned grid = ds_grid_spread(num_envs);        // a wave per env
    const hipStream_t s = (hipStream_t)stream;
    if (!chunk && g.EPL == 2) hipLaunchKernelGGL((k_ppo_steps256<2, false>), dim3(grid), dim3(DS_BLOCK), 0, s, d, e, r);
    else if (chunk && g.EPL == 2) hipLaunchKernelGGL((k_ppo_steps256<2, true>), dim3(grid), dim3(DS_BLOCK), 0, s, d, e, r);
    else if (chunk && g.EPL == 4) hipLaunchKernelGGL((k_ppo_steps256<4, true>), dim3(grid), dim3(DS_BLOCK), 0, s, d, e, r);
    else return fail("lb_ppo_steps256: unsupported geometry");
    return check_launch();
}

}  // extern "C"
