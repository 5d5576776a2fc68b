// lbk8s_eval.h — lb_eval_steps: the vector steps of a greedy evaluation (run_test_deepset.py:44-98)
// in ONE launch.
//
// A step of lbk8s/evaluate.py:run_test is the greedy forward (lb_ds_q_argmax), lb_step and, for
// the finished episodes' sums and the VecMonitor log, lb_ppo_record.  Over an evaluation the
// network and the masks are fixed and every output is per env, so -- as k_dqn_step does for a DQN
// train period and k_ppo_steps for a PPO rollout -- one wave carries its P envs through all the
// steps: the env in registers (W = 16, one endpoint per lane: the layout of E <= 16 below 32,768
// envs), the group's observations in a two-buffer LDS image that the forward reads, the float32
// running return and the episode sums in registers.  Same functions, same order per env: bit for
// bit the 3 x steps launches (tests/test_gpu_eval_steps.py).
//
// The forward is k_dqn_step's greedy one: the actor part of the VALU image (VG_ACTOR floats at
// frag + DS_FLOATS, staged once per block) under ds_group_obs / ds_group_actor<1, P, 2, true>.  Its
// arithmetic is per set column, so the bits do not depend on P (lb_ds_q_argmax itself takes P = 1
// or 2 by the batch).  LDS at P = 2: the image and scratch (39,424 + 8,192 B) plus 8 waves x 2
// buffers x P x DQN_OBS_F4 float4s (17,408 B) = 65,024 B: two blocks per CU.
//
// What a step leaves in global memory is its trace row (actions_all / rewards_all / dones_all,
// each optional) and, when an episode ends, the ep_stats row and the log row; the observations,
// the env state and the per-env words of the last lb_step are written once, after the last step.
#pragma once

#include "lbk8s_deepsets.h"
#include "lbk8s_dqn.h"
#include "lbk8s_slice.h"

namespace lbk {

struct EvalSteps {
    int steps;
    float4* obs;           // [B][2 R]: step 0's input; <- the observations after the last step
    int32_t* actions_all;  // [steps][B] or NULL
    float* rewards_all;    // [steps][B] or NULL
    uint8_t* dones_all;    // [steps][B] or NULL
    double* ep_sum;        // [B] or NULL (then ep_cnt too)
    double* ep_cnt;
    // the episode log (lb_ppo_record's; log == NULL: none, and ret32 / ep_r32 are not touched)
    float* ret32;
    float* ep_r32;
    int64_t tag0;
    double* log;
    int64_t cap;
    uint32_t* count;
};

// d: the forward (lb_ds_q_argmax's DSParams without obs or Q values: the actor-only image, masks,
// actions = the caller's int32 action buffer); e: the env (lb_step's Params: reward, done,
// ep_stats, no obs and no terminal obs).
template <int P>
__global__ __launch_bounds__(DS_BLOCK, 2) void k_eval_steps(DSParams d, Params e, EvalSteps r) {
    static_assert(P == 1 || P == 2, "envs per wave iteration (the VALU Gamma takes at most two)");
    constexpr int NWB = DS_BLOCK / 64;
    __shared__ __attribute__((aligned(16))) float W[VG_ACTOR + NWB * P * VG_SCRATCH];
    __shared__ __attribute__((aligned(16))) float4 OB[NWB][2][P * DQN_OBS_F4];
    for (int i = threadIdx.x * 4; i < VG_ACTOR; i += DS_BLOCK * 4)
        *reinterpret_cast<float4*>(W + i) = *reinterpret_cast<const float4*>(d.wfrag + DS_FLOATS + i);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* xs = W + VG_ACTOR + wv * P * VG_SCRATCH;
    // wave-major numbering, as k_deepsets_fwd: fewer groups than waves put one wave per SIMD
    const int64_t wave = (int64_t)wv * gridDim.x + blockIdx.x;
    const int64_t nwaves = (int64_t)gridDim.x * NWB;
    const int R = d.R, col = lane & 15, grp = lane >> 4;
    const int s = lane >> 4, l16 = lane & 15;
    const int f4 = 2 * R;  // float4s per observation (<= DQN_OBS_F4: host check)
    const int64_t B = e.B, groups = (B + P - 1) / P;
    float4(*ob)[P * DQN_OBS_F4] = OB[wv];
    for (int64_t gi = wave; gi < groups; gi += nwaves) {
        const int64_t env0 = gi * P;
        const int64_t env = env0 + s;
        const bool live = s < P && env < B;
        const bool head = live && l16 == 0;  // the lane of the env's scalars
        const int j1 = (int)((env0 + P < B ? env0 + P : B) - env0) * f4;  // the group's float4s
        SEnv<1> v;
        double esum = 0.0, ecnt = 0.0;
        float ret32 = 0.f;
        if (live) {
            slice_load<16, 1>(e, env, l16, v);
            slice_observe<1>(e, v);
        }
        if (head) {
            if (r.ep_sum) {
                esum = r.ep_sum[env];
                ecnt = r.ep_cnt[env];
            }
            if (r.log) ret32 = r.ret32[env];
        }
        for (int j = lane; j < j1; j += 64) ob[0][j] = r.obs[env0 * f4 + j];
        for (int i = 0; i < r.steps; ++i) {
            const float4* cur = ob[i & 1];
            float4* nxt = ob[(i + 1) & 1];
            const int64_t row = (int64_t)i * B;
            // lb_ds_q_argmax on the LDS observations (lane s holds env0 + s's action), then to the
            // lanes of the env's slice
            float h0[P][2], m0[2], xr0[2];
            ds_group_obs<1, P, 2>(d, env0, col, grp, R, h0, m0, xr0, reinterpret_cast<const float*>(cur));
            const int32_t act = ds_group_actor<1, P, 2, true>(d, W, lane, env0, col, grp, R, h0, m0, xs);
            const int32_t a = __shfl(act, s < P ? s : 0);
            // lb_step: lanes 16 s .. 16 s + 15 step env env0 + s (k_step_slice<16, 1>'s body, the
            // observed values kept in registers)
            float rw = 0.f;
            double reward = 0.0, ret = 0.0;
            bool dn = false;
            if (live) {
                const SPrep pr = slice_prep<16, 1>(e, v, a);
                const double tot0 = v.total;
                reward = slice_apply<16, 1, false, false>(e, env, l16, v, pr, dn);
                rw = (float)reward;
                ret = e.auto_reset ? tot0 + reward : 0.0;  // (the ep_stats row's return: v.total at the end)
                slice_obs_rows<16, 1>(e, l16, v, [&](int q, float4 o) { nxt[s * f4 + q] = o; });
            }
            // the step's trace row, then lb_ppo_record: the finished episode's sums, the VecMonitor
            // return
            float r32 = 0.f;
            if (head) {
                if (r.actions_all) r.actions_all[row + env] = a;
                if (r.rewards_all) r.rewards_all[row + env] = rw;
                if (r.dones_all) r.dones_all[row + env] = (uint8_t)dn;
                if (i == r.steps - 1) {  // what the last lb_step leaves
                    e.reward[env] = rw;
                    e.rew64[env] = reward;
                    e.done[env] = (uint8_t)dn;
                }
                if (r.ep_sum && dn) {
                    esum += e.auto_reset ? ret : e.ep_stats[env * LB_ST_K + LB_ST_RETURN];
                    ecnt += 1.0;
                }
                if (r.log) {
                    r32 = (float)((double)ret32 + reward);
                    ret32 = dn ? 0.f : r32;
                    if (dn && r.ep_r32) r.ep_r32[env] = r32;
                }
            }
            if (r.log) {  // (wave-uniform: every lane takes part in the ballot)
                const bool dl = head && dn;
                const uint64_t m = __ballot(dl);
                if (m) {
                    const int first = __ffsll((unsigned long long)m) - 1;
                    uint32_t base = 0;
                    if (lane == first) base = atomicAdd(r.count, (uint32_t)__popcll(m));
                    base = (uint32_t)__shfl((int)base, first);
                    const int64_t slot = (int64_t)base + __popcll(m & ((1ull << lane) - 1));
                    if (dl && slot < r.cap) {
                        double* lr = r.log + slot * LB_EPLOG_W;
                        const double* st = e.ep_stats + env * LB_ST_K;  // (this lane wrote the row)
#pragma unroll
                        for (int k = 0; k < LB_ST_K; ++k) lr[k] = st[k];
                        lr[LB_EPLOG_RET32] = (double)r32;
                        lr[LB_EPLOG_REWARD] = (double)rw;
                        lr[LB_EPLOG_ACTION] = (double)a;
                        lr[LB_EPLOG_ENV] = (double)env;
                        lr[LB_EPLOG_TAG] = (double)(r.tag0 + i);
                    }
                }
            }
        }
        // obs <- the observations after the last step, from LDS (the wave's LDS writes and reads
        // complete in order), then the env
        const float4* fin = ob[r.steps & 1];
        for (int j = lane; j < j1; j += 64) r.obs[env0 * f4 + j] = fin[j];
        if (live) {
            if (l16 < e.E) e.edyn[eidx(e, env, l16)] = v.ed[0];
            if (l16 == 0) slice_store_scalars<1>(e, env, v);
        }
        if (head) {
            if (r.ep_sum) {
                r.ep_sum[env] = esum;
                r.ep_cnt[env] = ecnt;
            }
            if (r.log) r.ret32[env] = ret32;
        }
    }
}

}  // namespace lbk
