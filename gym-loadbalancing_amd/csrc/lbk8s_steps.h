// lbk8s_steps.h — what the one-launch step kernels share: k_dqn_step (lbk8s_dqn.h), k_ppo_steps
// (lbk8s_ppo.h) and k_eval_steps (lbk8s_eval.h).
//
// In each of them one wave carries a group of P envs through all the steps of the launch: lanes
// 16 s .. 16 s + 15 hold env env0 + s in registers (W = 16, one endpoint per lane: the slice
// layout of E <= 16 below 32,768 envs), the group's observations live in a two-buffer LDS image
// (step i's input and its next observations) that the forward reads and the stored rows are
// copied from, and the env's history counters and scalars go back to memory once, after the last
// step.  StepsGroup is that skeleton -- open, step, record, close -- and a kernel adds what is its
// own: the forward that chooses the action and the rows a step leaves in global memory.  Same
// functions, same order per env as lb_step and lb_ppo_record: bit for bit the separate launches.
//
// The episode log's row and VecMonitor's float32 return are written here and nowhere else
// (eplog_append is lb_episode_log's append too).
#pragma once

#include "lbk8s_common.h"
#include "lbk8s_slice.h"

namespace lbk {

constexpr int STEPS_OBS_F4 = 34;  // float4s of an observation of R <= 17 rows (dqn_step_fusable: R <= 16)
static_assert(2 * 16 <= STEPS_OBS_F4, "the LDS observation image holds R <= 16 rows");

// lb_ppo_record's buffers: the finished episodes' per-env sums and the episode log
struct StepsRecord {
    double* ep_sum;  // [B] or NULL (then ep_cnt too)
    double* ep_cnt;
    // the episode log (log == NULL: none, and ret32 / ep_r32 are not touched)
    float* ret32;
    float* ep_r32;
    int64_t tag0;  // step i of the launch logs tag0 + i
    double* log;
    int64_t cap;
    uint32_t* count;
};

struct EpLogStep {  // the reward and action words of a log row
    float reward;
    int32_t action;
};

// Appends the rows of the wave's finished episodes to the device log: one atomic per wave (the
// ballot's count), rows past cap dropped (count still advances: the host sees the overflow).
// Every lane of the wave calls it, done or not; step() is evaluated by the lanes that write a row.
template <typename Step>
__device__ __forceinline__ void eplog_append(bool done, int64_t env, const double* ep_stats, float r32, int64_t tag,
                                             double* log, int64_t cap, uint32_t* count, Step&& step) {
    const int lane = threadIdx.x & 63;
    const uint64_t m = __ballot(done);
    if (!m) return;
    const int first = __ffsll((unsigned long long)m) - 1;
    uint32_t base = 0;
    if (lane == first) base = atomicAdd(count, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, first);
    const int64_t slot = (int64_t)base + __popcll(m & ((1ull << lane) - 1));
    if (!done || slot >= cap) return;
    double* row = log + slot * LB_EPLOG_W;
    const double* st = ep_stats + env * LB_ST_K;
#pragma unroll
    for (int k = 0; k < LB_ST_K; ++k) row[k] = st[k];
    const EpLogStep w = step();
    row[LB_EPLOG_RET32] = (double)r32;
    row[LB_EPLOG_REWARD] = (double)w.reward;
    row[LB_EPLOG_ACTION] = (double)w.action;
    row[LB_EPLOG_ENV] = (double)env;
    row[LB_EPLOG_TAG] = (double)tag;
}

// One group of P envs of a wave across the launch's steps.  rec == NULL (k_dqn_step, whose sums
// stay in memory): no record registers.
template <int P>
struct StepsGroup {
    int64_t env0, env;  // the group's first env; this lane's
    bool live, head;    // the lane holds an env; it is the lane of the env's scalars
    int j1;             // the group's float4s
    int s, l16, f4;     // slice, lane in the slice, float4s per observation
    SEnv<1> v;
    double esum, ecnt;  // the env's ep_sum / ep_cnt and VecMonitor's float32 running return (head)
    float ret32;
    // the last step's results
    float rw;
    double reward, ret;  // ret: the finished episode's return (its ep_stats row's first column)
    bool dn;

    // the env loaded and observed once, as k_rollout_slice
    __device__ __forceinline__ void open(const Params& e, const StepsRecord* rec, int64_t gi, int lane, int f4_) {
        s = lane >> 4, l16 = lane & 15, f4 = f4_;
        env0 = gi * P;
        env = env0 + s;
        live = s < P && env < e.B;
        head = live && l16 == 0;
        j1 = (int)((env0 + P < e.B ? env0 + P : e.B) - env0) * f4;
        esum = 0.0, ecnt = 0.0;
        ret32 = 0.f;
        if (live) {
            slice_load<16, 1>(e, env, l16, v);
            slice_observe<1>(e, v);
        }
        if (rec && head) {
            if (rec->ep_sum) {
                esum = rec->ep_sum[env];
                ecnt = rec->ep_cnt[env];
            }
            if (rec->log) ret32 = rec->ret32[env];
        }
    }

    // lb_step with action a: lanes 16 s .. 16 s + 15 step env env0 + s (k_step_slice<16, 1>'s body,
    // the observed values kept in registers: a step changes the selected endpoint's); the next
    // observations to the LDS buffer nxt
    __device__ __forceinline__ void step(const Params& e, int a, float4* nxt) {
        rw = 0.f;
        reward = 0.0, ret = 0.0;
        dn = false;
        if (live) {
            const SPrep pr = slice_prep<16, 1>(e, v, a);
            const double tot0 = v.total;
            reward = slice_apply<16, 1, false, false>(e, env, l16, v, pr, dn);
            rw = (float)reward;
            ret = e.auto_reset ? tot0 + reward : 0.0;  // (slice_apply's v.total += reward)
            slice_obs_rows<16, 1>(e, l16, v, [&](int q, float4 o) { nxt[s * f4 + q] = o; });
        }
    }

    // lb_ppo_record of step i: the finished episode's sums, VecMonitor's float32 episode_returns +=
    // the env's float64 reward (one rounding), the log row.  rec by value: its fields are then the
    // kernel's own arguments inside the step loop, and the kernels compile to what they were with
    // this code written out in each (through a pointer k_eval_steps measured 1.5 % slower)
    __device__ __forceinline__ void record(const Params& e, const StepsRecord rec, int a, int i) {
        float r32 = 0.f;
        if (head) {
            if (rec.ep_sum && dn) {
                esum += e.auto_reset ? ret : e.ep_stats[env * LB_ST_K + LB_ST_RETURN];
                ecnt += 1.0;
            }
            if (rec.log) {
                r32 = (float)((double)ret32 + reward);
                ret32 = dn ? 0.f : r32;
                if (dn && rec.ep_r32) rec.ep_r32[env] = r32;
            }
        }
        if (rec.log)  // (wave-uniform: every lane takes part in the ballot; a done head wrote the stats row)
            eplog_append(head && dn, env, e.ep_stats, r32, rec.tag0 + i, rec.log, rec.cap, rec.count,
                         [&] { return EpLogStep{rw, a}; });
    }

    // the env's history counters and scalars, stored after the last step
    __device__ __forceinline__ void close(const Params& e, const StepsRecord* rec) {
        if (live) {
            if (l16 < e.E) e.edyn[eidx(e, env, l16)] = v.ed[0];
            if (l16 == 0) slice_store_scalars<1>(e, env, v);
        }
        if (rec && head) {
            if (rec->ep_sum) {
                rec->ep_sum[env] = esum;
                rec->ep_cnt[env] = ecnt;
            }
            if (rec->log) rec->ret32[env] = ret32;
        }
    }
};

}  // namespace lbk
