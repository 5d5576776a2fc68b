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

// lb_ppo_steps' and lb_eval_steps' checks of their record arguments (fn: the entry point's name)
int steps_record_check(const char* fn, const StepsRecord& rec) {
    const char* msg = nullptr;
    if ((rec.ep_sum == nullptr) != (rec.ep_cnt == nullptr)) msg = ": ep_sum and ep_cnt go together";
    else if (rec.log && (!rec.ret32 || !rec.count || rec.cap < 0)) msg = ": a log needs ret32, count and cap >= 0";
    if (!msg) return 0;
    g_err = std::string(fn) + msg;
    return -1;
}

// lb_dqn_step's one-launch shape: the env in the slice layout with 16 lanes per env (E <= 16
// below 32,768 envs) and R <= 16.  A property of the shape only (not of the device's CU count):
// the kernel is correct for any number of envs, and the learner's path must not change with the
// part it runs on
bool dqn_step_fusable(const lb_config* cfg, int64_t num_envs, int32_t num_elements) {
    const Geo g = geometry(cfg, num_envs);
    return !g.tpe && g.W == 16 && g.EPL == 1 && num_elements <= 16;
}

int dqn_steps_launch(const float* frag, float* obs, int64_t num_envs, int32_t num_elements, const uint8_t* masks,
                     void* state, const lb_config* cfg, const lb_dqn_explore* ex, int32_t* actions_out,
                     float* next_obs_out, float* reward_out, uint8_t* done_out, float* terminal_obs_out,
                     double* ep_stats_out, int64_t slots, const int64_t* pos_in, int64_t* pos_out, float* rb_obs,
                     float* rb_next_obs, int64_t* rb_actions, float* rb_rewards, float* rb_dones, double* ep_sum,
                     double* ep_cnt, int32_t steps, int32_t* sync, void* stream) {
    // (the three entry points' checks)
    if (!frag || !obs || !state || !ex || !actions_out || !next_obs_out || !reward_out || !done_out || num_envs < 1)
        return fail("lb_dqn_step: frag/obs/state/ex/actions/next_obs/reward/done NULL or num_envs < 1");
    if (!ex->vstep_in || !ex->vstep_out || (!sync && ex->vstep_in == ex->vstep_out) || !ex->explore_out)
        return fail("lb_dqn_explore: device words NULL (or vstep_in == vstep_out)");
    if (cfg->rng_mode != LB_RNG_PHILOX) return fail("lb_dqn_step draws in Philox mode only");
    const int32_t A = cfg->num_endpoints + (cfg->rejection_allowed ? 1 : 0);
    if (num_elements != A) return fail("lb_dqn_step: num_elements must be the env's action count (R)");
    if (slots < 1 || !pos_in || !pos_out || (!sync && pos_in == pos_out) || !rb_obs || !rb_next_obs ||
        !rb_actions || !rb_rewards || !rb_dones || ((ep_sum || ep_cnt) && !(ep_sum && ep_cnt && ep_stats_out)))
        return fail("replay buffers NULL (or pos_in == pos_out)");
    Params e = make_params(state, cfg, num_envs);
    e.obs = next_obs_out;
    e.reward = reward_out;
    e.done = done_out;
    e.term_obs = terminal_obs_out;
    e.ep_stats = ep_stats_out;
    DSParams d{obs, frag, nullptr, nullptr, num_envs, num_elements, 1, 0, nullptr, nullptr, nullptr, nullptr,
               actions_out, masks};
    d.ex_on = 1;
    d.ex = *ex;
    d.ex_acc3 = e.acc3;
    d.ex_sc = e.sc;
    d.ex_env_offset = e.env_id_offset;
    d.ex_key0 = e.key0;
    d.ex_key1 = e.key1;
    DQNReplay r{slots, num_elements * 2, pos_in, pos_out, reinterpret_cast<float4*>(obs),
                reinterpret_cast<float4*>(rb_obs), reinterpret_cast<float4*>(rb_next_obs), rb_actions, rb_rewards,
                rb_dones, ep_sum, ep_cnt};
    return steps_launch(k_dqn_step<STEPS_P>, num_envs, stream, d, e, r, (int)steps, sync);
}

// lb_ppo_steps' and lb_eval_steps' shape: lb_dqn_step's one-launch shape (a property of the shape
// only), Philox draws and a forward over exactly the env's actions
bool steps_fusable(const lb_config* cfg, int64_t num_envs, int32_t num_elements) {
    const int32_t A = cfg->num_endpoints + (cfg->rejection_allowed ? 1 : 0);
    return num_envs >= 1 && cfg->rng_mode == LB_RNG_PHILOX && num_elements == A &&
           dqn_step_fusable(cfg, num_envs, num_elements);
}
}  // namespace

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
    return dqn_steps_launch(frag, obs, num_envs, num_elements, masks, state, cfg, ex, actions_out, next_obs_out,
                            reward_out, done_out, terminal_obs_out, ep_stats_out, slots, pos_in, pos_out, rb_obs,
                            rb_next_obs, rb_actions, rb_rewards, rb_dones, ep_sum, ep_cnt, 1, nullptr, stream);
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
    if (steps < 1 || steps > 32) return fail("lb_dqn_steps: steps must be in [1, 32]");
    if (!sync) return fail("lb_dqn_steps: sync (a device int32 that is 0) is required");
    if (!dqn_step_fusable(cfg, num_envs, num_elements))
        return fail("lb_dqn_steps: the env's shape has no one-launch vector step (lb_dqn_steps_supported)");
    return dqn_steps_launch(frag, obs, num_envs, num_elements, masks, state, cfg, ex, actions_out, next_obs_out,
                            reward_out, done_out, terminal_obs_out, ep_stats_out, slots, pos_in, pos_out, rb_obs,
                            rb_next_obs, rb_actions, rb_rewards, rb_dones, ep_sum, ep_cnt, steps, sync, stream);
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
    if (num_envs < 1) return fail("lb_ppo_steps: num_envs < 1");
    if (steps < 1 || steps > LB_PPO_STEPS_MAX) return fail("lb_ppo_steps: steps must be in [1, 4096]");
    if (store_rows != steps && store_rows != steps - 1)
        return fail("lb_ppo_steps: store_rows must be steps or steps - 1");
    if (!frag || !obs || !state || !uniforms || !actions_f32 || !logprobs || !values || !rewards || !actions_out ||
        !done_out || !ep_stats_out)
        return fail("lb_ppo_steps: frag/obs/state/uniforms/actions_f32/logprobs/values/rewards/actions_out/done_out/"
                    "ep_stats_out NULL");
    if (store_rows > 0 && (!obs_next || !dones_next)) return fail("lb_ppo_steps: obs_next / dones_next NULL");
    if (store_rows < steps && (!last_obs || !last_done))
        return fail("lb_ppo_steps: store_rows == steps - 1 needs last_obs and last_done");
    const StepsRecord rec{ep_sum, ep_cnt, ret32, ep_r32, tag0, log, cap, count};
    if (int rc = steps_record_check("lb_ppo_steps", rec)) return rc;
    if (!steps_fusable(cfg, num_envs, num_elements))
        return fail("lb_ppo_steps: the env's shape has no one-launch rollout (lb_ppo_steps_supported)");
    Params e = make_params(state, cfg, num_envs);
    e.done = done_out;
    e.ep_stats = ep_stats_out;
    DSParams d{nullptr, frag, nullptr, nullptr, num_envs, num_elements, 1, 1, nullptr, nullptr, nullptr, nullptr,
               actions_out, nullptr};
    PPOSteps r{steps, store_rows, obs, uniforms, actions_f32, logprobs, values, rewards,
               reinterpret_cast<float4*>(obs_next), dones_next, reinterpret_cast<float4*>(last_obs), last_done, rec};
    return steps_launch(k_ppo_steps<STEPS_P>, num_envs, stream, d, e, r);
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
    if (num_envs < 1) return fail("lb_eval_steps: num_envs < 1");
    if (steps < 1 || steps > LB_EVAL_STEPS_MAX) return fail("lb_eval_steps: steps must be in [1, 4096]");
    if (!frag || !obs || !state || !actions_out || !reward_out || !done_out || !ep_stats_out)
        return fail("lb_eval_steps: frag/obs/state/actions_out/reward_out/done_out/ep_stats_out NULL");
    const StepsRecord rec{ep_sum, ep_cnt, ret32, ep_r32, tag0, log, cap, count};
    if (int rc = steps_record_check("lb_eval_steps", rec)) return rc;
    if (!steps_fusable(cfg, num_envs, num_elements))
        return fail("lb_eval_steps: the env's shape has no one-launch evaluation (lb_eval_steps_supported)");
    Params e = make_params(state, cfg, num_envs);
    e.reward = reward_out;
    e.done = done_out;
    e.ep_stats = ep_stats_out;
    DSParams d{nullptr, frag, nullptr, nullptr, num_envs, num_elements, 1, 0, nullptr, nullptr, nullptr, nullptr,
               actions_out, masks};
    EvalSteps r{steps, reinterpret_cast<float4*>(obs), actions_all, rewards_all, dones_all, rec};
    return steps_launch(k_eval_steps<STEPS_P>, num_envs, stream, d, e, r);
}

}  // extern "C"
