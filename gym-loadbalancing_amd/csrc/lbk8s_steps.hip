// lbk8s_steps.hip — the one-launch step kernels (lbk8s_steps.h: k_dqn_step of lbk8s_dqn.h,
// k_ppo_steps of lbk8s_ppo.h, k_eval_steps of lbk8s_eval.h) and their entry points.
//
// Compiled after lbk8s_env.hip in one unit (lbk8s_env_steps.hip says why); it stands as a unit of
// its own as well.  Public ABI: include/lbk8s.h; the host helpers: lbk8s_host.h.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "lbk8s.h"
#include "lbk8s_common.h"
#include "lbk8s_deepsets.h"
#include "lbk8s_steps.h"
#include "lbk8s_dqn.h"
#include "lbk8s_ppo.h"
#include "lbk8s_eval.h"
#include "lbk8s_host.h"
#include "lbk8s_steps_host.h"

using namespace lbk;

namespace {
// The launch of a one-launch step kernel: a wave per group of STEPS_P envs.  2 puts the 4096-env
// batch on every wave of the grid (4: half the waves idle; one env per wave measured slower:
// profiles/r06_dqn_p1_ab.jsonl), and is what k_ppo_steps' LDS budget allows (lbk8s_ppo.h)
constexpr int STEPS_P = 2;
template <typename... A>
int steps_launch(void (*kernel)(A...), int64_t num_envs, void* stream, A... args) {
    const unsigned grid = ds_grid_spread((num_envs + STEPS_P - 1) / STEPS_P);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(DS_BLOCK), 0, (hipStream_t)stream, args...);
    return check_launch();
}

// lb_dqn_step's one-launch shape: the env in the slice layout with 16 lanes per env (E <= 16
// below 32,768 envs) and R <= 16.  A property of the shape only (not of the device's CU count):
// the kernel is correct for any number of envs, and the learner's path must not change with the
// part it runs on
bool dqn_step_fusable(const lb_config* cfg, int64_t num_envs, int32_t num_elements) {
    const Geo g = geometry(cfg, num_envs);
    return !g.tpe && g.W == 16 && g.EPL == 1 && num_elements <= 16;
}

// lb_ppo_steps' and lb_eval_steps' shape: lb_dqn_step's one-launch shape (a property of the shape
// only), Philox draws and a forward over exactly the env's actions
bool steps_fusable(const lb_config* cfg, int64_t num_envs, int32_t num_elements) {
    const int32_t A = cfg->num_endpoints + (cfg->rejection_allowed ? 1 : 0);
    return num_envs >= 1 && cfg->rng_mode == LB_RNG_PHILOX && num_elements == A &&
           dqn_step_fusable(cfg, num_envs, num_elements);
}
}  // namespace

namespace lbk {
int ppo_steps_launch(const PPOStepsCall& c) {
    DSParams d;
    Params e;
    PPOSteps r;
    ppo_steps_params(c, d, e, r);
    return steps_launch(k_ppo_steps<STEPS_P>, c.num_envs, c.stream, d, e, r);
}

int ppo_steps_tl_launch(const PPOStepsCall& c) {
    DSParams d;
    Params e;
    PPOStepsTL r;
    ppo_steps_params(c, d, e, r);  // (e.term_obs: the call's terminal_obs)
    r.term_values = c.term_values;
    return steps_launch(k_ppo_steps<STEPS_P, true>, c.num_envs, c.stream, d, e, r);
}

int eval_steps_launch(const EvalStepsCall& c) {
    DSParams d;
    Params e;
    EvalSteps r;
    eval_steps_params(c, d, e, r);
    return steps_launch(k_eval_steps<STEPS_P>, c.num_envs, c.stream, d, e, r);
}

int dqn_steps_launch(const DQNStepsCall& c) {
    DSParams d;
    Params e;
    DQNReplay r;
    dqn_steps_params(c, d, e, r);
    return steps_launch(k_dqn_step<STEPS_P>, c.num_envs, c.stream, d, e, r, (int)c.steps, c.sync);
}
}  // namespace lbk

extern "C" {

int lb_dqn_step(const float* frag, float* obs, int64_t num_envs, int32_t num_elements, const uint8_t* masks,
                void* state, const lb_config* cfg, const lb_dqn_explore* ex, int32_t* actions_out,
                float* next_obs_out, float* reward_out, uint8_t* done_out, float* terminal_obs_out,
                double* ep_stats_out, int64_t slots, const int64_t* pos_in, int64_t* pos_out, float* rb_obs,
                float* rb_next_obs, int64_t* rb_actions, float* rb_rewards, float* rb_dones, double* ep_sum,
                double* ep_cnt, void* stream) {
    if (int r = validate(cfg)) return r;
    if (!dqn_step_fusable(cfg, num_envs, num_elements)) {  // the three launches
        if (int rc = lb_dqn_act(frag, obs, num_envs, num_elements, masks, state, cfg, ex, actions_out, stream)) return rc;
        if (int rc = lb_step(state, cfg, num_envs, actions_out, next_obs_out, reward_out, done_out, terminal_obs_out,
                             ep_stats_out, nullptr, stream))
            return rc;
        return lb_replay_add(num_envs, num_elements * 8, slots, pos_in, pos_out, obs, next_obs_out, actions_out,
                             reward_out, done_out, ep_stats_out, rb_obs, rb_next_obs, rb_actions, rb_rewards, rb_dones,
                             ep_sum, ep_cnt, stream);
    }
    const DQNStepsCall c{frag, obs, num_envs, num_elements, masks, state, cfg, ex, actions_out, next_obs_out, reward_out,
                         done_out, terminal_obs_out, ep_stats_out, slots, pos_in, pos_out, rb_obs, rb_next_obs,
                         rb_actions, rb_rewards, rb_dones, ep_sum, ep_cnt, 1, nullptr, stream};
    if (int rc = dqn_steps_check("lb_dqn_step", c, true)) return rc;
    return dqn_steps_launch(c);
}

int lb_dqn_steps_supported(const lb_config* cfg, int64_t num_envs, int32_t num_elements) {
    if (validate(cfg)) return 0;
    return dqn_step_fusable(cfg, num_envs, num_elements) ? 1 : 0;
}

int lb_dqn_steps(const float* frag, float* obs, int64_t num_envs, int32_t num_elements, const uint8_t* masks,
                 void* state, const lb_config* cfg, const lb_dqn_explore* ex, int32_t* actions_out,
                 float* next_obs_out, float* reward_out, uint8_t* done_out, float* terminal_obs_out,
                 double* ep_stats_out, int64_t slots, const int64_t* pos_in, int64_t* pos_out, float* rb_obs,
                 float* rb_next_obs, int64_t* rb_actions, float* rb_rewards, float* rb_dones, double* ep_sum,
                 double* ep_cnt, int32_t steps, int32_t* sync, void* stream) {
    if (int r = validate(cfg)) return r;
    const DQNStepsCall c{frag, obs, num_envs, num_elements, masks, state, cfg, ex, actions_out, next_obs_out, reward_out,
                         done_out, terminal_obs_out, ep_stats_out, slots, pos_in, pos_out, rb_obs, rb_next_obs,
                         rb_actions, rb_rewards, rb_dones, ep_sum, ep_cnt, steps, sync, stream};
    if (int rc = dqn_period_check("lb_dqn_steps", c)) return rc;
    if (!dqn_step_fusable(cfg, num_envs, num_elements)) return steps_unsupported("lb_dqn_steps", "vector step");
    if (int rc = dqn_steps_check("lb_dqn_steps", c, false)) return rc;
    return dqn_steps_launch(c);
}

int lb_ppo_steps_supported(const lb_config* cfg, int64_t num_envs, int32_t num_elements) {
    if (validate(cfg)) return 0;
    return steps_fusable(cfg, num_envs, num_elements) ? 1 : 0;
}

int lb_ppo_steps(const float* frag, const float* obs, void* state, const lb_config* cfg, int64_t num_envs,
                 int32_t num_elements, int32_t steps, int32_t store_rows, const float* uniforms, float* actions_f32,
                 float* logprobs, float* values, float* rewards, float* obs_next, float* dones_next, float* last_obs,
                 float* last_done, int32_t* actions_out, uint8_t* done_out, double* ep_stats_out, double* ep_sum,
                 double* ep_cnt, float* ret32, float* ep_r32, int64_t tag0, double* log, int64_t cap, uint32_t* count,
                 void* stream) {
    if (int r = validate(cfg)) return r;
    const PPOStepsCall c{frag, obs, state, cfg, num_envs, num_elements, steps, store_rows, uniforms, actions_f32, logprobs,
                         values, rewards, obs_next, dones_next, last_obs, last_done, actions_out, done_out, ep_stats_out,
                         {ep_sum, ep_cnt, ret32, ep_r32, tag0, log, cap, count}, stream};
    if (int rc = ppo_steps_check("lb_ppo_steps", c)) return rc;
    if (!steps_fusable(cfg, num_envs, num_elements)) return steps_unsupported("lb_ppo_steps", "rollout");
    return ppo_steps_launch(c);
}

// lb_ppo_steps with the terminal values (include/lbk8s_abi_ppo_tl.h): lb_ppo_steps' shape
int lb_ppo_steps_tl_supported(const lb_config* cfg, int64_t num_envs, int32_t num_elements) {
    return lb_ppo_steps_supported(cfg, num_envs, num_elements);
}

int lb_ppo_steps_tl(const float* frag, const float* obs, void* state, const lb_config* cfg, int64_t num_envs,
                    int32_t num_elements, int32_t steps, int32_t store_rows, const float* uniforms, float* actions_f32,
                    float* logprobs, float* values, float* rewards, float* obs_next, float* dones_next,
                    float* last_obs, float* last_done, int32_t* actions_out, uint8_t* done_out, double* ep_stats_out,
                    double* ep_sum, double* ep_cnt, float* ret32, float* ep_r32, int64_t tag0, double* log,
                    int64_t cap, uint32_t* count, float* terminal_obs, float* term_values, void* stream) {
    if (int r = validate(cfg)) return r;
    const PPOStepsCall c{frag, obs, state, cfg, num_envs, num_elements, steps, store_rows, uniforms, actions_f32, logprobs,
                         values, rewards, obs_next, dones_next, last_obs, last_done, actions_out, done_out, ep_stats_out,
                         {ep_sum, ep_cnt, ret32, ep_r32, tag0, log, cap, count}, stream, terminal_obs, term_values};
    if (int rc = ppo_steps_check("lb_ppo_steps_tl", c)) return rc;
    if (!terminal_obs || !term_values) return steps_fail("lb_ppo_steps_tl", ": terminal_obs / term_values NULL");
    if (!steps_fusable(cfg, num_envs, num_elements)) return steps_unsupported("lb_ppo_steps_tl", "rollout");
    return ppo_steps_tl_launch(c);
}

// lb_eval_steps' shape is lb_ppo_steps' (the greedy forward in place of the sampling one)
int lb_eval_steps_supported(const lb_config* cfg, int64_t num_envs, int32_t num_elements) {
    if (validate(cfg)) return 0;
    return steps_fusable(cfg, num_envs, num_elements) ? 1 : 0;
}

int lb_eval_steps(const float* frag, float* obs, void* state, const lb_config* cfg, int64_t num_envs,
                  int32_t num_elements, const uint8_t* masks, int32_t steps, int32_t* actions_all, float* rewards_all,
                  uint8_t* dones_all, int32_t* actions_out, float* reward_out, uint8_t* done_out,
                  double* ep_stats_out, double* ep_sum, double* ep_cnt, float* ret32, float* ep_r32, int64_t tag0,
                  double* log, int64_t cap, uint32_t* count, void* stream) {
    if (int r = validate(cfg)) return r;
    const EvalStepsCall c{frag, obs, state, cfg, num_envs, num_elements, masks, steps, actions_all, rewards_all, dones_all,
                          actions_out, reward_out, done_out, ep_stats_out,
                          {ep_sum, ep_cnt, ret32, ep_r32, tag0, log, cap, count}, stream};
    if (int rc = eval_steps_check("lb_eval_steps", c)) return rc;
    if (!steps_fusable(cfg, num_envs, num_elements)) return steps_unsupported("lb_eval_steps", "evaluation");
    return eval_steps_launch(c);
}

}  // extern "C"
