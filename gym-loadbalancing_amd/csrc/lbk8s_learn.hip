// lbk8s_learn.hip — the learners' small bookkeeping kernels and their entry points: the replay
// add and sample (DQN), the episode log, the PPO vector step's record and GAE.
//
// Public ABI: include/lbk8s.h; the host helpers: lbk8s_host.h.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "lbk8s.h"
#include "lbk8s_common.h"
#include "lbk8s_host.h"
#include "lbk8s_steps.h"

namespace lbk {

// lb_replay_add: the DQN vector step's bookkeeping in one launch (dqn_deepset.py:158-174
// replay add + obs <- next_obs, :147-156 episode returns).  Slot pos = *pos_in; one thread
// writes (pos + 1) % slots to *pos_out, a different word (callers alternate the two), so
// no thread of this launch can read the advanced position.
struct ReplayParams {
    int64_t B;
    int f4;  // float4s per observation
    int64_t slots;
    const int64_t* pos_in;
    int64_t* pos_out;
    float4* obs;
    const float4* next_obs;
    const int32_t* actions;
    const float* reward;
    const uint8_t* done;
    const double* ep_stats;  // [B][LB_ST_K], column 0 = the finished episode's return
    float4* rb_obs;
    float4* rb_next_obs;
    int64_t* rb_actions;
    float* rb_rewards;
    float* rb_dones;
    double* ep_sum;  // [B] per-env sums (deterministic; reduced when flushed)
    double* ep_cnt;
};

__global__ void k_replay_add(ReplayParams p) {
    const int64_t pos = *p.pos_in;
    const int64_t n4 = p.B * p.f4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4 || i < p.B;
         i += (int64_t)gridDim.x * blockDim.x) {
        if (i < n4) {
            const float4 o = p.obs[i], nx = p.next_obs[i];
            p.rb_obs[pos * n4 + i] = o;
            p.rb_next_obs[pos * n4 + i] = nx;
            p.obs[i] = nx;
        }
        if (i < p.B) {
            const float d = p.done[i] ? 1.f : 0.f;
            p.rb_actions[pos * p.B + i] = p.actions[i];
            p.rb_rewards[pos * p.B + i] = p.reward[i];
            p.rb_dones[pos * p.B + i] = d;
            if (p.ep_sum && p.done[i]) {
                p.ep_sum[i] += p.ep_stats[i * LB_ST_K];
                p.ep_cnt[i] += 1.0;
            }
        }
        if (i == 0) *p.pos_out = (pos + 1) % p.slots;
    }
}

// lb_replay_sample: SB3 ReplayBuffer.sample's (slot, env) draws and the gather; thread
// (i, part): part < f4 -> obs float4, < 2 f4 -> next_obs float4, == 2 f4 -> the scalars
struct ReplaySampleParams {
    int64_t B;
    int f4;
    int64_t slots;
    int batch;
    uint64_t seed;
    const int64_t* vstep;
    const int64_t* base_adds;
    const float4* rb_obs;
    const float4* rb_next_obs;
    const int64_t* rb_actions;
    const float* rb_rewards;
    const float* rb_dones;
    float4* obs;
    float4* next_obs;
    int64_t* actions;
    float* rewards;
    float* dones;
};
__global__ void k_replay_sample(ReplaySampleParams p) {
    const int parts = 2 * p.f4 + 1;
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (int64_t)p.batch * parts) return;
    const int i = (int)(q / parts), part = (int)(q - (int64_t)i * parts);
    const int64_t t = *p.vstep, adds = *p.base_adds + t;
    const int64_t upper = adds < p.slots ? (adds > 0 ? adds : 1) : p.slots;
    const U4 w = philox((uint32_t)t, (uint32_t)((uint64_t)t >> 32), (uint32_t)i, D_DQN_SAMPLE, (uint32_t)p.seed,
                        (uint32_t)(p.seed >> 32));
    const int64_t bi = (int64_t)(((uint64_t)w.x * (uint64_t)upper) >> 32);  // upper < 2^32
    const int64_t ei = (int64_t)bounded(w.y, (uint32_t)p.B);
    const int64_t row = bi * p.B + ei;
    if (part < p.f4) p.obs[(int64_t)i * p.f4 + part] = p.rb_obs[row * p.f4 + part];
    else if (part < 2 * p.f4) p.next_obs[(int64_t)i * p.f4 + part - p.f4] = p.rb_next_obs[row * p.f4 + part - p.f4];
    else {
        p.actions[i] = p.rb_actions[row];
        p.rewards[i] = p.rb_rewards[row];
        p.dones[i] = p.rb_dones[row];
    }
}

// lb_episode_log: VecMonitor's per-env float32 return and the finished episodes' rows,
// appended to a device log (one atomic per wave: the ballot's count)
struct EpLogParams {
    int64_t B;
    const uint8_t* done;
    const double* ep_stats;
    const float* reward;
    const double* reward64;
    const int32_t* actions;
    float* ret32;
    float* ep_r32;
    int64_t tag;
    double* log;
    int64_t cap;
    uint32_t* count;
};

// one env's part of the episode log; every lane of the wave calls it (the ballot), live or not
__device__ __forceinline__ void episode_log_env(const EpLogParams& p, int64_t env) {
    bool d = false;
    float r32 = 0.f;
    if (env < p.B) {
        // VecMonitor's float32 episode_returns += the env's float64 reward: one rounding
        r32 = p.reward64 ? (float)((double)p.ret32[env] + p.reward64[env]) : p.ret32[env] + p.reward[env];
        d = p.done[env] != 0;
        p.ret32[env] = d ? 0.f : r32;
        if (d && p.ep_r32) p.ep_r32[env] = r32;
    }
    eplog_append(d, env, p.ep_stats, r32, p.tag, p.log, p.cap, p.count,
                 [&] { return EpLogStep{p.reward[env], p.actions[env]}; });
}

__global__ __launch_bounds__(256) void k_episode_log(EpLogParams p) {
    episode_log_env(p, (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
}

// lb_ppo_record: the PPO vector step's bookkeeping in one launch (ppo_deepset.py:174-190: the
// next step's done row as float32, the finished episodes' returns) and, with a log, lb_episode_log.
// The sums are per env, as lb_replay_add's: deterministic, reduced once per rollout by the caller.
struct PPORecordParams {
    EpLogParams log;  // log.log == NULL: no episode log; B, done and ep_stats are always set
    float* next_done;
    double* ep_sum;  // [B] or NULL (then ep_cnt too)
    double* ep_cnt;
};

__global__ __launch_bounds__(256) void k_ppo_record(PPORecordParams p) {
    const int64_t env = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (env < p.log.B) {
        const bool d = p.log.done[env] != 0;
        p.next_done[env] = d ? 1.f : 0.f;
        if (d && p.ep_sum) {
            p.ep_sum[env] += p.log.ep_stats[env * LB_ST_K + LB_ST_RETURN];
            p.ep_cnt[env] += 1.0;
        }
    }
    if (p.log.log) episode_log_env(p.log, env);  // (wave-uniform: every lane takes part in its ballot)
}

// lb_gae: the GAE recurrence (ppo_deepset.py:192-205) of one env per thread, t downwards with
// values[t + 1] / dones[t + 1] carried in registers, so every input word is read once, coalesced
// across envs.  float32 op for op as torch evaluates it (the build has -ffp-contract=off).  The
// loads of GAE_UNROLL steps are issued before the chain that consumes them: their addresses do
// not depend on the recurrence.
constexpr int GAE_BLOCK = 64;  // small blocks: PPO's 4096 envs spread over 64 CUs
constexpr int GAE_UNROLL = 4;
struct GAEParams {
    const float* rewards;
    const float* values;
    const float* dones;
    const float* next_value;
    const float* next_done;
    int64_t T, B;
    float g, gl;  // (float)gamma, (float)(gamma * gae_lambda)
    float* adv;
    float* ret;
};

__device__ __forceinline__ void gae_step(const GAEParams& p, float r, float v, float& nv, float& nd, float& last,
                                         int64_t idx) {
    const float nnt = 1.f - nd;
    const float delta = (r + (p.g * nv) * nnt) - v;
    last = delta + (p.gl * nnt) * last;
    p.adv[idx] = last;
    p.ret[idx] = last + v;
    nv = v;
}

__global__ __launch_bounds__(GAE_BLOCK) void k_gae(GAEParams p) {
    const int64_t b = (int64_t)blockIdx.x * GAE_BLOCK + threadIdx.x;
    if (b >= p.B) return;
    float nv = p.next_value[b], nd = p.next_done[b], last = 0.f;
    int64_t t = p.T - 1;
    for (; t >= GAE_UNROLL - 1; t -= GAE_UNROLL) {
        float r[GAE_UNROLL], v[GAE_UNROLL], d[GAE_UNROLL];
#pragma unroll
        for (int k = 0; k < GAE_UNROLL; ++k) {
            const int64_t idx = (t - k) * p.B + b;
            r[k] = p.rewards[idx];
            v[k] = p.values[idx];
            d[k] = p.dones[idx];
        }
#pragma unroll
        for (int k = 0; k < GAE_UNROLL; ++k) {
            gae_step(p, r[k], v[k], nv, nd, last, (t - k) * p.B + b);
            nd = d[k];
        }
    }
    for (; t >= 0; --t) {
        const int64_t idx = t * p.B + b;
        const float r = p.rewards[idx], v = p.values[idx], d = p.dones[idx];
        gae_step(p, r, v, nv, nd, last, idx);
        nd = d;
    }
}

// lb_gae_tl: k_gae with the bootstrap at a time limit (include/lbk8s_abi_ppo_tl.h): where the step
// ended the episode (nd != 0) the TD error takes the terminal observation's value, term_values[t],
// in place of values[t + 1] (the next episode's first value), and the lambda-chain is cut as in
// k_gae.  g * bv in place of (g * nv) * nnt: with term_values zero, or no done set, k_gae's bits.
__device__ __forceinline__ void gae_tl_step(const GAEParams& p, float r, float v, float tv, float& nv, float& nd,
                                            float& last, int64_t idx) {
    const float bv = nd != 0.f ? tv : nv;
    const float nnt = 1.f - nd;
    const float delta = (r + p.g * bv) - v;
    last = delta + (p.gl * nnt) * last;
    p.adv[idx] = last;
    p.ret[idx] = last + v;
    nv = v;
}

__global__ __launch_bounds__(GAE_BLOCK) void k_gae_tl(GAEParams p, const float* term_values) {
    const int64_t b = (int64_t)blockIdx.x * GAE_BLOCK + threadIdx.x;
    if (b >= p.B) return;
    float nv = p.next_value[b], nd = p.next_done[b], last = 0.f;
    int64_t t = p.T - 1;
    for (; t >= GAE_UNROLL - 1; t -= GAE_UNROLL) {
        float r[GAE_UNROLL], v[GAE_UNROLL], d[GAE_UNROLL], tv[GAE_UNROLL];
#pragma unroll
        for (int k = 0; k < GAE_UNROLL; ++k) {
            const int64_t idx = (t - k) * p.B + b;
            r[k] = p.rewards[idx];
            v[k] = p.values[idx];
            d[k] = p.dones[idx];
            tv[k] = term_values[idx];
        }
#pragma unroll
        for (int k = 0; k < GAE_UNROLL; ++k) {
            gae_tl_step(p, r[k], v[k], tv[k], nv, nd, last, (t - k) * p.B + b);
            nd = d[k];
        }
    }
    for (; t >= 0; --t) {
        const int64_t idx = t * p.B + b;
        const float r = p.rewards[idx], v = p.values[idx], d = p.dones[idx], tv = term_values[idx];
        gae_tl_step(p, r, v, tv, nv, nd, last, idx);
        nd = d;
    }
}

}  // namespace lbk

using namespace lbk;

extern "C" {

int lb_replay_add(int64_t num_envs, int32_t obs_floats, int64_t slots, const int64_t* pos_in, int64_t* pos_out,
                  float* obs, const float* next_obs, const int32_t* actions, const float* reward, const uint8_t* done,
                  const double* ep_stats, float* rb_obs, float* rb_next_obs, int64_t* rb_actions, float* rb_rewards,
                  float* rb_dones, double* ep_sum, double* ep_cnt, void* stream) {
    if (num_envs < 1 || obs_floats < 4 || obs_floats % 4 || slots < 1) return fail("bad replay geometry");
    if (!pos_in || !pos_out || pos_in == pos_out || !obs || !next_obs || !actions || !reward || !done || !rb_obs ||
        !rb_next_obs || !rb_actions || !rb_rewards || !rb_dones || ((ep_sum || ep_cnt) && !(ep_sum && ep_cnt && ep_stats)))
        return fail("replay buffers NULL (or pos_in == pos_out)");
    ReplayParams p{num_envs, obs_floats / 4, slots, pos_in, pos_out, reinterpret_cast<float4*>(obs),
                   reinterpret_cast<const float4*>(next_obs), actions, reward, done, ep_stats,
                   reinterpret_cast<float4*>(rb_obs), reinterpret_cast<float4*>(rb_next_obs), rb_actions, rb_rewards,
                   rb_dones, ep_sum, ep_cnt};
    const int64_t n = std::max<int64_t>(num_envs * p.f4, num_envs);
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 65535);
    hipLaunchKernelGGL(k_replay_add, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    return check_launch();
}

int lb_replay_sample(int64_t num_envs, int32_t obs_floats, int64_t slots, int32_t batch, uint64_t seed,
                     const int64_t* vstep, const int64_t* base_adds, const float* rb_obs, const float* rb_next_obs,
                     const int64_t* rb_actions, const float* rb_rewards, const float* rb_dones, float* obs_out,
                     float* next_obs_out, int64_t* actions_out, float* rewards_out, float* dones_out, void* stream) {
    if (num_envs < 1 || obs_floats < 4 || obs_floats % 4 || slots < 1 || slots >= (1ll << 32) || batch < 1 ||
        num_envs >= (1ll << 32))
        return fail("bad replay sample geometry");
    if (!vstep || !base_adds || !rb_obs || !rb_next_obs || !rb_actions || !rb_rewards || !rb_dones || !obs_out ||
        !next_obs_out || !actions_out || !rewards_out || !dones_out)
        return fail("replay sample buffers NULL");
    ReplaySampleParams p{num_envs, obs_floats / 4, slots, batch, seed, vstep, base_adds,
                         reinterpret_cast<const float4*>(rb_obs), reinterpret_cast<const float4*>(rb_next_obs),
                         rb_actions, rb_rewards, rb_dones, reinterpret_cast<float4*>(obs_out),
                         reinterpret_cast<float4*>(next_obs_out), actions_out, rewards_out, dones_out};
    const int64_t n = (int64_t)batch * (2 * p.f4 + 1);
    hipLaunchKernelGGL(k_replay_sample, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    return check_launch();
}

int lb_episode_log(int64_t num_envs, const uint8_t* done, const double* ep_stats, const float* reward,
                   const double* reward64, const int32_t* actions, float* ret32, float* ep_r32, int64_t tag, double* log, int64_t cap,
                   uint32_t* count, void* stream) {
    if (num_envs < 1 || !done || !ep_stats || !reward || !actions || !ret32 || !log || !count || cap < 0)
        return fail("episode log: buffers NULL or num_envs < 1");
    EpLogParams p{num_envs, done, ep_stats, reward, reward64, actions, ret32, ep_r32, tag, log, cap, count};
    hipLaunchKernelGGL(k_episode_log, dim3(env_blocks(num_envs)), dim3(BLOCK), 0, (hipStream_t)stream, p);
    return check_launch();
}

int lb_ppo_record(int64_t num_envs, const uint8_t* done, const double* ep_stats, float* next_done_out,
                  double* ep_sum, double* ep_cnt, const float* reward, const double* reward64,
                  const int32_t* actions, float* ret32, float* ep_r32, int64_t tag, double* log, int64_t cap,
                  uint32_t* count, void* stream) {
    if (num_envs < 1 || !done || !ep_stats || !next_done_out)
        return fail("lb_ppo_record: done/ep_stats/next_done_out NULL or num_envs < 1");
    if ((ep_sum == nullptr) != (ep_cnt == nullptr)) return fail("lb_ppo_record: ep_sum and ep_cnt go together");
    if (log && (!reward || !actions || !ret32 || !count || cap < 0))
        return fail("lb_ppo_record: a log needs reward, actions, ret32, count and cap >= 0");
    PPORecordParams p{{num_envs, done, ep_stats, reward, reward64, actions, ret32, ep_r32, tag, log, cap, count},
                      next_done_out, ep_sum, ep_cnt};
    hipLaunchKernelGGL(k_ppo_record, dim3(env_blocks(num_envs)), dim3(BLOCK), 0, (hipStream_t)stream, p);
    return check_launch();
}

int lb_gae(const float* rewards, const float* values, const float* dones, const float* next_value,
           const float* next_done, int64_t num_steps, int64_t num_envs, double gamma, double gae_lambda,
           float* advantages_out, float* returns_out, void* stream) {
    if (num_steps < 1 || num_envs < 1) return fail("lb_gae: num_steps < 1 or num_envs < 1");
    if (!rewards || !values || !dones || !next_value || !next_done || !advantages_out || !returns_out)
        return fail("lb_gae: a buffer is NULL");
    const void* in[5] = {rewards, values, dones, next_value, next_done};
    for (const void* q : in)
        if (q == advantages_out || q == returns_out) return fail("lb_gae: an output is also an input");
    if (advantages_out == returns_out) return fail("lb_gae: advantages_out == returns_out");
    // rounded once, the product in double first (Python's gamma * gae_lambda)
    GAEParams p{rewards, values, dones, next_value, next_done, num_steps, num_envs,
                (float)gamma, (float)(gamma * gae_lambda), advantages_out, returns_out};
    const int64_t blocks = (num_envs + GAE_BLOCK - 1) / GAE_BLOCK;
    if (blocks > 0x7FFFFFFF) return fail("lb_gae: num_envs too large for one launch");
    hipLaunchKernelGGL(k_gae, dim3((unsigned)blocks), dim3(GAE_BLOCK), 0, (hipStream_t)stream, p);
    return check_launch();
}

int lb_gae_tl(const float* rewards, const float* values, const float* dones, const float* next_value,
              const float* next_done, const float* term_values, int64_t num_steps, int64_t num_envs, double gamma,
              double gae_lambda, float* advantages_out, float* returns_out, void* stream) {
    if (num_steps < 1 || num_envs < 1) return fail("lb_gae_tl: num_steps < 1 or num_envs < 1");
    if (!rewards || !values || !dones || !next_value || !next_done || !term_values || !advantages_out || !returns_out)
        return fail("lb_gae_tl: a buffer is NULL");
    const void* in[6] = {rewards, values, dones, next_value, next_done, term_values};
    for (const void* q : in)
        if (q == advantages_out || q == returns_out) return fail("lb_gae_tl: an output is also an input");
    if (advantages_out == returns_out) return fail("lb_gae_tl: advantages_out == returns_out");
    GAEParams p{rewards, values, dones, next_value, next_done, num_steps, num_envs,
                (float)gamma, (float)(gamma * gae_lambda), advantages_out, returns_out};
    const int64_t blocks = (num_envs + GAE_BLOCK - 1) / GAE_BLOCK;
    if (blocks > 0x7FFFFFFF) return fail("lb_gae_tl: num_envs too large for one launch");
    hipLaunchKernelGGL(k_gae_tl, dim3((unsigned)blocks), dim3(GAE_BLOCK), 0, (hipStream_t)stream, p, term_values);
    return check_launch();
}

}  // extern "C"

// The kernels of the policies LB_POLICY_ROUND_ROBIN .. LB_POLICY_REWARD_GREEDY are compiled with this
// unit (csrc/Makefile says why here).
#include "lbk8s_policies.hip"
