// lbk8s_steps64.hip — the one-launch step kernels for envs of up to 64 endpoints (lbk8s_steps64.h,
// lbk8s_dqn64.h) and their entry points: lb_ppo_steps64, lb_eval_steps64 and lb_dqn_steps64, the
// supersets of lb_ppo_steps, lb_eval_steps and lb_dqn_steps (lbk8s_steps.hip).
//
// Compiled at the end of lbk8s_ds_train.hip, the build's shortest unit (the set of units stays
// as it was: csrc/Makefile).  Public ABI: include/lbk8s.h; the host helpers: lbk8s_host.h.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "lbk8s.h"
#include "lbk8s_common.h"
#include "lbk8s_deepsets.h"
#include "lbk8s_steps64.h"
#include "lbk8s_dqn64.h"
#include "lbk8s_host.h"
#include "lbk8s_steps_host.h"

using namespace lbk;

namespace {
// lb_ppo_steps64's and lb_eval_steps64's shape (a property of the shape only, never of the
// device's CU count): Philox draws, a forward over exactly the env's actions, 1..32,767 envs in
// the slice layout with one endpoint per lane, R <= 65; and whatever lb_ppo_steps takes (a
// superset: its 16-lane layout of E = 9..16 holds at 32,768 envs and above too)
bool steps64_fusable(const lb_config* cfg, int64_t num_envs, int32_t num_elements) {
    if (lb_ppo_steps_supported(cfg, num_envs, num_elements) == 1) return true;
    const int32_t A = cfg->num_endpoints + (cfg->rejection_allowed ? 1 : 0);
    if (num_envs < 1 || num_envs >= WIDE_SLICE_MAX_B || cfg->rng_mode != LB_RNG_PHILOX || num_elements != A) return false;
    const Geo g = geometry(cfg, num_envs);
    return !g.tpe && g.EPL == 1 && num_elements <= STEPS64_MAX_R;
}

// lb_dqn_steps64's shape: lb_dqn_steps' (which asks neither for Philox mode nor for the action
// count: its launch refuses those), or the rule above
bool dqn_steps64_fusable(const lb_config* cfg, int64_t num_envs, int32_t num_elements) {
    return lb_dqn_steps_supported(cfg, num_envs, num_elements) == 1 || steps64_fusable(cfg, num_envs, num_elements);
}

// BODY with the env's slice width and the forward's set tiles as the constants W and TS: the six
// shapes of lbk8s_steps64.h's table (steps64_fusable holds and the 16-lane kernels do not apply)
#define LB_DISPATCH_STEPS64(W_, TS_, BODY)                                     \
    do {                                                                       \
        if (W_ == 16 && TS_ == 2) { constexpr int W = 16, TS = 2; BODY; }      \
        else if (W_ == 32 && TS_ == 2) { constexpr int W = 32, TS = 2; BODY; } \
        else if (W_ == 32 && TS_ == 3) { constexpr int W = 32, TS = 3; BODY; } \
        else if (W_ == 64 && TS_ == 3) { constexpr int W = 64, TS = 3; BODY; } \
        else if (W_ == 64 && TS_ == 4) { constexpr int W = 64, TS = 4; BODY; } \
        else if (W_ == 64 && TS_ == 5) { constexpr int W = 64, TS = 5; BODY; } \
        else return fail("lb_steps64: unsupported geometry");                  \
    } while (0)
// The launch of KERNEL<W, TS> for the call c, a wave per env (returns on an unsupported geometry)
#define LB_LAUNCH_STEPS64(KERNEL, c, ...)                                                                    \
    do {                                                                                                     \
        const Geo g = geometry((c).cfg, (c).num_envs);                                                       \
        const int ts = ((c).num_elements + 15) / 16;                                                         \
        const unsigned grid = ds_grid_spread((c).num_envs);                                                  \
        LB_DISPATCH_STEPS64(g.W, ts, hipLaunchKernelGGL((KERNEL<W, TS>), dim3(grid), dim3(DS_BLOCK), 0,      \
                                                        (hipStream_t)(c).stream, __VA_ARGS__));              \
    } while (0)
}  // namespace

namespace lbk {
int ppo_steps64_launch(const PPOStepsCall& c) {
    if (lb_ppo_steps_supported(c.cfg, c.num_envs, c.num_elements)) return ppo_steps_launch(c);  // the 16-lane shape
    DSParams d;
    Params e;
    PPOSteps r;
    ppo_steps_params(c, d, e, r);
    LB_LAUNCH_STEPS64(k_ppo_steps64, c, d, e, r);
    return check_launch();
}

int eval_steps64_launch(const EvalStepsCall& c) {
    if (lb_eval_steps_supported(c.cfg, c.num_envs, c.num_elements)) return eval_steps_launch(c);  // the 16-lane shape
    DSParams d;
    Params e;
    EvalSteps r;
    eval_steps_params(c, d, e, r);
    LB_LAUNCH_STEPS64(k_eval_steps64, c, d, e, r);
    return check_launch();
}

int dqn_steps64_launch(const DQNStepsCall& c) {
    if (lb_dqn_steps_supported(c.cfg, c.num_envs, c.num_elements)) return dqn_steps_launch(c);  // the 16-lane shape
    DSParams d;
    Params e;
    DQNReplay r;
    dqn_steps_params(c, d, e, r);
    LB_LAUNCH_STEPS64(k_dqn_steps64, c, d, e, r, (int)c.steps, c.sync);
    return check_launch();
}
}  // namespace lbk

extern "C" {

int lb_ppo_steps64_supported(const lb_config* cfg, int64_t num_envs, int32_t num_elements) {
    if (validate(cfg)) return 0;
    return steps64_fusable(cfg, num_envs, num_elements) ? 1 : 0;
}

int lb_ppo_steps64(const float* frag, const float* obs, void* state, const lb_config* cfg, int64_t num_envs,
                   int32_t num_elements, int32_t steps, int32_t store_rows, const float* uniforms, float* actions_f32,
                   float* logprobs, float* values, float* rewards, float* obs_next, float* dones_next,
                   float* last_obs, float* last_done, int32_t* actions_out, uint8_t* done_out, double* ep_stats_out,
                   double* ep_sum, double* ep_cnt, float* ret32, float* ep_r32, int64_t tag0, double* log, int64_t cap,
                   uint32_t* count, void* stream) {
    if (int r = validate(cfg)) return r;
    const PPOStepsCall c{frag, obs, state, cfg, num_envs, num_elements, steps, store_rows, uniforms, actions_f32, logprobs,
                         values, rewards, obs_next, dones_next, last_obs, last_done, actions_out, done_out, ep_stats_out,
                         {ep_sum, ep_cnt, ret32, ep_r32, tag0, log, cap, count}, stream};
    if (int rc = ppo_steps_check("lb_ppo_steps64", c)) return rc;
    if (!steps64_fusable(cfg, num_envs, num_elements)) return steps_unsupported("lb_ppo_steps64", "rollout");
    return ppo_steps64_launch(c);
}

// lb_eval_steps64's shape is lb_ppo_steps64's (the greedy forward in place of the sampling one)
int lb_eval_steps64_supported(const lb_config* cfg, int64_t num_envs, int32_t num_elements) {
    if (validate(cfg)) return 0;
    return steps64_fusable(cfg, num_envs, num_elements) ? 1 : 0;
}

int lb_eval_steps64(const float* frag, float* obs, void* state, const lb_config* cfg, int64_t num_envs,
                    int32_t num_elements, const uint8_t* masks, int32_t steps, int32_t* actions_all,
                    float* rewards_all, uint8_t* dones_all, int32_t* actions_out, float* reward_out, uint8_t* done_out,
                    double* ep_stats_out, double* ep_sum, double* ep_cnt, float* ret32, float* ep_r32, int64_t tag0,
                    double* log, int64_t cap, uint32_t* count, void* stream) {
    if (int r = validate(cfg)) return r;
    const EvalStepsCall c{frag, obs, state, cfg, num_envs, num_elements, masks, steps, actions_all, rewards_all, dones_all,
                          actions_out, reward_out, done_out, ep_stats_out,
                          {ep_sum, ep_cnt, ret32, ep_r32, tag0, log, cap, count}, stream};
    if (int rc = eval_steps_check("lb_eval_steps64", c)) return rc;
    if (!steps64_fusable(cfg, num_envs, num_elements)) return steps_unsupported("lb_eval_steps64", "evaluation");
    return eval_steps64_launch(c);
}

int lb_dqn_steps64_supported(const lb_config* cfg, int64_t num_envs, int32_t num_elements) {
    if (validate(cfg)) return 0;
    return dqn_steps64_fusable(cfg, num_envs, num_elements) ? 1 : 0;
}

int lb_dqn_steps64(const float* frag, float* obs, int64_t num_envs, int32_t num_elements, const uint8_t* masks,
                   void* state, const lb_config* cfg, const lb_dqn_explore* ex, int32_t* actions_out,
                   float* next_obs_out, float* reward_out, uint8_t* done_out, float* terminal_obs_out,
                   double* ep_stats_out, int64_t slots, const int64_t* pos_in, int64_t* pos_out, float* rb_obs,
                   float* rb_next_obs, int64_t* rb_actions, float* rb_rewards, float* rb_dones, double* ep_sum,
                   double* ep_cnt, int32_t steps, int32_t* sync, void* stream) {
    if (int r = validate(cfg)) return r;
    const DQNStepsCall c{frag, obs, num_envs, num_elements, masks, state, cfg, ex, actions_out, next_obs_out, reward_out,
                         done_out, terminal_obs_out, ep_stats_out, slots, pos_in, pos_out, rb_obs, rb_next_obs,
                         rb_actions, rb_rewards, rb_dones, ep_sum, ep_cnt, steps, sync, stream};
    if (int rc = dqn_period_check("lb_dqn_steps64", c)) return rc;
    if (int rc = dqn_steps_check("lb_dqn_steps64", c, false)) return rc;
    if (!dqn_steps64_fusable(cfg, num_envs, num_elements)) return steps_unsupported("lb_dqn_steps64", "vector step");
    return dqn_steps64_launch(c);
}

}  // extern "C"
