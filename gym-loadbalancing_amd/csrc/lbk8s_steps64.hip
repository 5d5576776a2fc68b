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

// (lbk8s_steps.hip's steps_record_check, with this file's entry points' names)
int steps64_record_check(const char* fn, const StepsRecord& rec) {
    const char* msg = nullptr;
    if ((rec.ep_sum == nullptr) != (rec.ep_cnt == nullptr)) msg = ": ep_sum and ep_cnt go together";
    else if (rec.log && (!rec.ret32 || !rec.count || rec.cap < 0)) msg = ": a log needs ret32, count and cap >= 0";
    if (!msg) return 0;
    g_err = std::string(fn) + msg;
    return -1;
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
}  // namespace

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
    if (num_envs < 1) return fail("lb_ppo_steps64: num_envs < 1");
    if (steps < 1 || steps > LB_PPO_STEPS_MAX) return fail("lb_ppo_steps64: steps must be in [1, 4096]");
    if (store_rows != steps && store_rows != steps - 1)
        return fail("lb_ppo_steps64: store_rows must be steps or steps - 1");
    if (!frag || !obs || !state || !uniforms || !actions_f32 || !logprobs || !values || !rewards || !actions_out ||
        !done_out || !ep_stats_out)
        return fail("lb_ppo_steps64: frag/obs/state/uniforms/actions_f32/logprobs/values/rewards/actions_out/done_out/"
                    "ep_stats_out NULL");
    if (store_rows > 0 && (!obs_next || !dones_next)) return fail("lb_ppo_steps64: obs_next / dones_next NULL");
    if (store_rows < steps && (!last_obs || !last_done))
        return fail("lb_ppo_steps64: store_rows == steps - 1 needs last_obs and last_done");
    const StepsRecord rec{ep_sum, ep_cnt, ret32, ep_r32, tag0, log, cap, count};
    if (int rc = steps64_record_check("lb_ppo_steps64", rec)) return rc;
    if (!steps64_fusable(cfg, num_envs, num_elements))
        return fail("lb_ppo_steps64: the env's shape has no one-launch rollout (lb_ppo_steps64_supported)");
    if (lb_ppo_steps_supported(cfg, num_envs, num_elements))  // the 16-lane shape: k_ppo_steps
        return lb_ppo_steps(frag, obs, state, cfg, num_envs, num_elements, steps, store_rows, uniforms, actions_f32,
                            logprobs, values, rewards, obs_next, dones_next, last_obs, last_done, actions_out, done_out,
                            ep_stats_out, ep_sum, ep_cnt, ret32, ep_r32, tag0, log, cap, count, stream);
    Params e = make_params(state, cfg, num_envs);
    e.done = done_out;
    e.ep_stats = ep_stats_out;
    DSParams d{nullptr, frag, nullptr, nullptr, num_envs, num_elements, 1, 1, nullptr, nullptr, nullptr, nullptr,
               actions_out, nullptr};
    PPOSteps r{steps, store_rows, obs, uniforms, actions_f32, logprobs, values, rewards,
               reinterpret_cast<float4*>(obs_next), dones_next, reinterpret_cast<float4*>(last_obs), last_done, rec};
    const Geo g = geometry(cfg, num_envs);
    const int ts = (num_elements + 15) / 16;
    const unsigned grid = ds_grid_spread(num_envs);  // a wave per env
    LB_DISPATCH_STEPS64(g.W, ts, hipLaunchKernelGGL((k_ppo_steps64<W, TS>), dim3(grid), dim3(DS_BLOCK), 0,
                                                    (hipStream_t)stream, d, e, r));
    return check_launch();
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
    if (num_envs < 1) return fail("lb_eval_steps64: num_envs < 1");
    if (steps < 1 || steps > LB_EVAL_STEPS_MAX) return fail("lb_eval_steps64: steps must be in [1, 4096]");
    if (!frag || !obs || !state || !actions_out || !reward_out || !done_out || !ep_stats_out)
        return fail("lb_eval_steps64: frag/obs/state/actions_out/reward_out/done_out/ep_stats_out NULL");
    const StepsRecord rec{ep_sum, ep_cnt, ret32, ep_r32, tag0, log, cap, count};
    if (int rc = steps64_record_check("lb_eval_steps64", rec)) return rc;
    if (!steps64_fusable(cfg, num_envs, num_elements))
        return fail("lb_eval_steps64: the env's shape has no one-launch evaluation (lb_eval_steps64_supported)");
    if (lb_eval_steps_supported(cfg, num_envs, num_elements))  // the 16-lane shape: k_eval_steps
        return lb_eval_steps(frag, obs, state, cfg, num_envs, num_elements, masks, steps, actions_all, rewards_all,
                             dones_all, actions_out, reward_out, done_out, ep_stats_out, ep_sum, ep_cnt, ret32, ep_r32,
                             tag0, log, cap, count, stream);
    Params e = make_params(state, cfg, num_envs);
    e.reward = reward_out;
    e.done = done_out;
    e.ep_stats = ep_stats_out;
    DSParams d{nullptr, frag, nullptr, nullptr, num_envs, num_elements, 1, 0, nullptr, nullptr, nullptr, nullptr,
               actions_out, masks};
    EvalSteps r{steps, reinterpret_cast<float4*>(obs), actions_all, rewards_all, dones_all, rec};
    const Geo g = geometry(cfg, num_envs);
    const int ts = (num_elements + 15) / 16;
    const unsigned grid = ds_grid_spread(num_envs);  // a wave per env
    LB_DISPATCH_STEPS64(g.W, ts, hipLaunchKernelGGL((k_eval_steps64<W, TS>), dim3(grid), dim3(DS_BLOCK), 0,
                                                    (hipStream_t)stream, d, e, r));
    return check_launch();
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
    if (steps < 1 || steps > 32) return fail("lb_dqn_steps64: steps must be in [1, 32]");
    if (!sync) return fail("lb_dqn_steps64: sync (a device int32 that is 0) is required");
    // (lb_dqn_steps' checks, under this entry point's name)
    if (!frag || !obs || !state || !ex || !actions_out || !next_obs_out || !reward_out || !done_out || num_envs < 1)
        return fail("lb_dqn_steps64: frag/obs/state/ex/actions/next_obs/reward/done NULL or num_envs < 1");
    if (!ex->vstep_in || !ex->vstep_out || !ex->explore_out)
        return fail("lb_dqn_steps64: lb_dqn_explore's device words NULL");
    if (cfg->rng_mode != LB_RNG_PHILOX) return fail("lb_dqn_steps64 draws in Philox mode only");
    const int32_t A = cfg->num_endpoints + (cfg->rejection_allowed ? 1 : 0);
    if (num_elements != A) return fail("lb_dqn_steps64: num_elements must be the env's action count (R)");
    if (slots < 1 || !pos_in || !pos_out || !rb_obs || !rb_next_obs || !rb_actions || !rb_rewards || !rb_dones ||
        ((ep_sum || ep_cnt) && !(ep_sum && ep_cnt && ep_stats_out)))
        return fail("lb_dqn_steps64: replay buffers NULL (or ep_sum / ep_cnt without the other or ep_stats_out)");
    if (!dqn_steps64_fusable(cfg, num_envs, num_elements))
        return fail("lb_dqn_steps64: the env's shape has no one-launch vector step (lb_dqn_steps64_supported)");
    if (lb_dqn_steps_supported(cfg, num_envs, num_elements))  // the 16-lane shape: k_dqn_step
        return lb_dqn_steps(frag, obs, num_envs, num_elements, masks, state, cfg, ex, actions_out, next_obs_out,
                            reward_out, done_out, terminal_obs_out, ep_stats_out, slots, pos_in, pos_out, rb_obs,
                            rb_next_obs, rb_actions, rb_rewards, rb_dones, ep_sum, ep_cnt, steps, sync, stream);
    // (dqn_steps_launch's parameters)
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
    const Geo g = geometry(cfg, num_envs);
    const int ts = (num_elements + 15) / 16;
    const unsigned grid = ds_grid_spread(num_envs);  // a wave per env
    LB_DISPATCH_STEPS64(g.W, ts, hipLaunchKernelGGL((k_dqn_steps64<W, TS>), dim3(grid), dim3(DS_BLOCK), 0,
                                                    (hipStream_t)stream, d, e, r, (int)steps, sync));
    return check_launch();
}

}  // extern "C"
