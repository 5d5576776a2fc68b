// lbk8s_steps_host.h — the host side the one-launch step entry points share (lbk8s_steps.hip,
// lbk8s_steps64.hip, lbk8s_steps256.hip): per family (PPO rollout, greedy evaluation, DQN train
// period) the call's arguments as one struct, their checks under the called entry point's name
// (fn) and the kernels' parameter structs.  An entry point packs its arguments once, checks them,
// refuses what its _supported query refuses and chooses a kernel by the env's geometry; a wide one
// that lands on a narrower kernel hands the struct to that kernel's launch below.
#pragma once

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

namespace lbk {

struct PPOStepsCall {  // lb_ppo_steps' arguments (include/lbk8s.h)
    const float *frag, *obs;
    void* state;
    const lb_config* cfg;
    int64_t num_envs;
    int32_t num_elements, steps, store_rows;
    const float* uniforms;
    float *actions_f32, *logprobs, *values, *rewards, *obs_next, *dones_next, *last_obs, *last_done;
    int32_t* actions_out;
    uint8_t* done_out;
    double* ep_stats_out;
    StepsRecord rec;
    void* stream;
    float *terminal_obs = nullptr, *term_values = nullptr;  // lb_ppo_steps_tl's (else NULL)
};

struct EvalStepsCall {  // lb_eval_steps' arguments
    const float* frag;
    float* obs;
    void* state;
    const lb_config* cfg;
    int64_t num_envs;
    int32_t num_elements;
    const uint8_t* masks;
    int32_t steps;
    int32_t* actions_all;
    float* rewards_all;
    uint8_t* dones_all;
    int32_t* actions_out;
    float* reward_out;
    uint8_t* done_out;
    double* ep_stats_out;
    StepsRecord rec;
    void* stream;
};

struct DQNStepsCall {  // lb_dqn_steps' arguments (lb_dqn_step: steps = 1, no sync)
    const float* frag;
    float* obs;
    int64_t num_envs;
    int32_t num_elements;
    const uint8_t* masks;
    void* state;
    const lb_config* cfg;
    const lb_dqn_explore* ex;
    int32_t* actions_out;
    float *next_obs_out, *reward_out;
    uint8_t* done_out;
    float* terminal_obs_out;
    double* ep_stats_out;
    int64_t slots;
    const int64_t* pos_in;
    int64_t* pos_out;
    float *rb_obs, *rb_next_obs;
    int64_t* rb_actions;
    float *rb_rewards, *rb_dones;
    double *ep_sum, *ep_cnt;
    int32_t steps;
    int32_t* sync;
    void* stream;
};

// The 16-lane kernels' launches of a checked call (lbk8s_steps.hip) and k_ppo_steps64's,
// k_eval_steps64's and k_dqn_steps64's, which are lb_ppo_steps256's, lb_eval_steps256's and
// lb_dqn_steps256's at E <= 64 (lbk8s_steps64.hip; they hand the 16-lane shape on themselves)
int ppo_steps_launch(const PPOStepsCall& c);
int ppo_steps_tl_launch(const PPOStepsCall& c);
int eval_steps_launch(const EvalStepsCall& c);
int dqn_steps_launch(const DQNStepsCall& c);
int ppo_steps64_launch(const PPOStepsCall& c);
int eval_steps64_launch(const EvalStepsCall& c);
int dqn_steps64_launch(const DQNStepsCall& c);

inline int steps_fail(const char* fn, const std::string& msg) {
    g_err = std::string(fn) + msg;
    return -1;
}

// what: "rollout", "evaluation", "vector step"
inline int steps_unsupported(const char* fn, const char* what) {
    return steps_fail(fn, std::string(": the env's shape has no one-launch ") + what + " (" + fn + "_supported)");
}

inline int steps_record_check(const char* fn, const StepsRecord& rec) {
    if ((rec.ep_sum == nullptr) != (rec.ep_cnt == nullptr)) return steps_fail(fn, ": ep_sum and ep_cnt go together");
    if (rec.log && (!rec.ret32 || !rec.count || rec.cap < 0))
        return steps_fail(fn, ": a log needs ret32, count and cap >= 0");
    return 0;
}

inline int ppo_steps_check(const char* fn, const PPOStepsCall& c) {
    if (c.num_envs < 1) return steps_fail(fn, ": num_envs < 1");
    if (c.steps < 1 || c.steps > LB_PPO_STEPS_MAX) return steps_fail(fn, ": steps must be in [1, 4096]");
    if (c.store_rows != c.steps && c.store_rows != c.steps - 1)
        return steps_fail(fn, ": store_rows must be steps or steps - 1");
    if (!c.frag || !c.obs || !c.state || !c.uniforms || !c.actions_f32 || !c.logprobs || !c.values || !c.rewards ||
        !c.actions_out || !c.done_out || !c.ep_stats_out)
        return steps_fail(fn, ": frag/obs/state/uniforms/actions_f32/logprobs/values/rewards/actions_out/done_out/"
                              "ep_stats_out NULL");
    if (c.store_rows > 0 && (!c.obs_next || !c.dones_next)) return steps_fail(fn, ": obs_next / dones_next NULL");
    if (c.store_rows < c.steps && (!c.last_obs || !c.last_done))
        return steps_fail(fn, ": store_rows == steps - 1 needs last_obs and last_done");
    return steps_record_check(fn, c.rec);
}

inline void ppo_steps_params(const PPOStepsCall& c, DSParams& d, Params& e, PPOSteps& r) {
    e = make_params(c.state, c.cfg, c.num_envs);
    e.done = c.done_out;
    e.term_obs = c.terminal_obs;
    e.ep_stats = c.ep_stats_out;
    d = DSParams{nullptr, c.frag, nullptr, nullptr, c.num_envs, c.num_elements, 1, 1, nullptr, nullptr, nullptr, nullptr,
                 c.actions_out, nullptr};
    r = PPOSteps{c.steps, c.store_rows, c.obs, c.uniforms, c.actions_f32, c.logprobs, c.values, c.rewards,
                 reinterpret_cast<float4*>(c.obs_next), c.dones_next, reinterpret_cast<float4*>(c.last_obs), c.last_done,
                 c.rec};
}

inline int eval_steps_check(const char* fn, const EvalStepsCall& c) {
    if (c.num_envs < 1) return steps_fail(fn, ": num_envs < 1");
    if (c.steps < 1 || c.steps > LB_EVAL_STEPS_MAX) return steps_fail(fn, ": steps must be in [1, 4096]");
    if (!c.frag || !c.obs || !c.state || !c.actions_out || !c.reward_out || !c.done_out || !c.ep_stats_out)
        return steps_fail(fn, ": frag/obs/state/actions_out/reward_out/done_out/ep_stats_out NULL");
    return steps_record_check(fn, c.rec);
}

inline void eval_steps_params(const EvalStepsCall& c, DSParams& d, Params& e, EvalSteps& r) {
    e = make_params(c.state, c.cfg, c.num_envs);
    e.reward = c.reward_out;
    e.done = c.done_out;
    e.ep_stats = c.ep_stats_out;
    d = DSParams{nullptr, c.frag, nullptr, nullptr, c.num_envs, c.num_elements, 1, 0, nullptr, nullptr, nullptr, nullptr,
                 c.actions_out, c.masks};
    r = EvalSteps{c.steps, reinterpret_cast<float4*>(c.obs), c.actions_all, c.rewards_all, c.dones_all, c.rec};
}

// lb_dqn_steps', lb_dqn_steps64's and lb_dqn_steps256's own arguments: the period's length and the launch's counter
inline int dqn_period_check(const char* fn, const DQNStepsCall& c) {
    if (c.steps < 1 || c.steps > 32) return steps_fail(fn, ": steps must be in [1, 32]");
    if (!c.sync) return steps_fail(fn, ": sync (a device int32 that is 0) is required");
    return 0;
}

// distinct (lb_dqn_step, which has no sync): the first block writes the device words while others
// may still read them, so in and out must differ
inline int dqn_steps_check(const char* fn, const DQNStepsCall& c, bool distinct) {
    if (!c.frag || !c.obs || !c.state || !c.ex || !c.actions_out || !c.next_obs_out || !c.reward_out || !c.done_out ||
        c.num_envs < 1)
        return steps_fail(fn, ": frag/obs/state/ex/actions/next_obs/reward/done NULL or num_envs < 1");
    if (!c.ex->vstep_in || !c.ex->vstep_out || (distinct && c.ex->vstep_in == c.ex->vstep_out) || !c.ex->explore_out)
        return steps_fail(fn, std::string(": lb_dqn_explore's device words NULL") +
                                  (distinct ? " (or vstep_in == vstep_out)" : ""));
    if (c.cfg->rng_mode != LB_RNG_PHILOX) return steps_fail(fn, " draws in Philox mode only");
    const int32_t A = c.cfg->num_endpoints + (c.cfg->rejection_allowed ? 1 : 0);
    if (c.num_elements != A) return steps_fail(fn, ": num_elements must be the env's action count (R)");
    if (c.slots < 1 || !c.pos_in || !c.pos_out || (distinct && c.pos_in == c.pos_out) || !c.rb_obs || !c.rb_next_obs ||
        !c.rb_actions || !c.rb_rewards || !c.rb_dones ||
        ((c.ep_sum || c.ep_cnt) && !(c.ep_sum && c.ep_cnt && c.ep_stats_out)))
        return steps_fail(fn, std::string(": replay buffers NULL (or ") + (distinct ? "pos_in == pos_out, or " : "") +
                                  "ep_sum / ep_cnt without the other or ep_stats_out)");
    return 0;
}

inline void dqn_steps_params(const DQNStepsCall& c, DSParams& d, Params& e, DQNReplay& r) {
    e = make_params(c.state, c.cfg, c.num_envs);
    e.obs = c.next_obs_out;
    e.reward = c.reward_out;
    e.done = c.done_out;
    e.term_obs = c.terminal_obs_out;
    e.ep_stats = c.ep_stats_out;
    d = DSParams{c.obs, c.frag, nullptr, nullptr, c.num_envs, c.num_elements, 1, 0, nullptr, nullptr, nullptr, nullptr,
                 c.actions_out, c.masks};
    d.ex_on = 1;
    d.ex = *c.ex;
    d.ex_acc3 = e.acc3;
    d.ex_sc = e.sc;
    d.ex_env_offset = e.env_id_offset;
    d.ex_key0 = e.key0;
    d.ex_key1 = e.key1;
    r = DQNReplay{c.slots, c.num_elements * 2, c.pos_in, c.pos_out, reinterpret_cast<float4*>(c.obs),
                  reinterpret_cast<float4*>(c.rb_obs), reinterpret_cast<float4*>(c.rb_next_obs), c.rb_actions,
                  c.rb_rewards, c.rb_dones, c.ep_sum, c.ep_cnt};
}

}  // namespace lbk
