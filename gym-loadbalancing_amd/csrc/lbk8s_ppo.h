// lbk8s_ppo.h — lb_ppo_steps: the vector steps of a PPO rollout (envs/ppo_deepset.py:160-190) in
// ONE launch.
//
// With fused_act and fused_bookkeeping a PPO vector step is three launches: lb_ds_sample (the
// deep-sets forward with the categorical draw), lb_step and lb_ppo_record (the next done row, the
// finished episodes' sums, the VecMonitor log).  Over a rollout the policy is fixed, the uniforms
// are drawn before it starts and every output is per env, so -- as k_dqn_step does for a DQN train
// period -- one wave carries its P envs through all the steps: the env in registers
// (W = 16, one endpoint per lane: the layout of E <= 16 below 32,768 envs), the group's
// observations in a two-buffer LDS image that the forward reads and the storage rows are copied
// from, the float32 running return and the episode sums in registers.  Same functions, same
// order per env: bit for bit the 3 x steps launches (tests/test_gpu_ppo_steps.py).
//
// The forward is lb_ds_sample's at R <= 16: the MFMA-fragment image (DS_FLOATS, staged once per
// block) under ds_group_obs / ds_group_actor / ds_group_critic<1, P, LB_DS_FWD_SAMPLE>.  Its
// arithmetic is per set column, so the bits do not depend on P (lb_ds_sample itself takes P = 1,
// 2 or 4 by the batch).  LDS: the image (135,440 B) plus 8 waves x 2 buffers x P x DQN_OBS_F4
// float4s = 152,848 B at P = 2 (P = 4 would pass 160 KB).
#pragma once

#include "lbk8s_deepsets.h"
#include "lbk8s_dqn.h"
#include "lbk8s_slice.h"

namespace lbk {

struct PPOSteps {
    int steps, store_rows;    // store_rows: steps or steps - 1 (the last step's rows go to last_*)
    const float* obs;         // [B][R][8]: step 0's input
    const float* uniforms;    // [steps][B]
    float* actions_f32;       // [steps][B], as logprobs, values, rewards
    float* logprobs;
    float* values;
    float* rewards;
    float4* obs_next;         // [store_rows][B][2 R]
    float* dones_next;        // [store_rows][B]
    float4* last_obs;         // [B][2 R]
    float* last_done;         // [B]
    double* ep_sum;           // [B] or NULL (then ep_cnt too)
    double* ep_cnt;
    // the episode log (lb_ppo_record's; log == NULL: none, and ret32 / ep_r32 are not touched)
    float* ret32;
    float* ep_r32;
    int64_t tag0;
    double* log;
    int64_t cap;
    uint32_t* count;
};

// d: the forward (lb_ds_sample's DSParams without masks or logits: actions = the caller's int32
// action buffer); e: the env (lb_step's Params: done, ep_stats, no terminal obs; obs / reward
// are the per-step rows of r).
template <int P>
__global__ __launch_bounds__(DS_BLOCK, 2) void k_ppo_steps(DSParams d, Params e, PPOSteps r) {
    static_assert(P == 1 || P == 2, "envs per wave iteration (the LDS budget)");
    constexpr int NWB = DS_BLOCK / 64;
    __shared__ __attribute__((aligned(16))) float W[DS_FLOATS];
    __shared__ __attribute__((aligned(16))) float4 OB[NWB][2][P * DQN_OBS_F4];
    for (int i = threadIdx.x * 4; i < DS_FLOATS; i += DS_BLOCK * 4)
        *reinterpret_cast<float4*>(W + i) = *reinterpret_cast<const float4*>(d.wfrag + i);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
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
        for (int j = lane; j < j1; j += 64) ob[0][j] = reinterpret_cast<const float4*>(r.obs)[env0 * f4 + j];
        for (int i = 0; i < r.steps; ++i) {
            const float4* cur = ob[i & 1];
            float4* nxt = ob[(i + 1) & 1];
            const int64_t row = (int64_t)i * B;
            const bool stored = i < r.store_rows;
            // lb_ds_sample on the LDS observations: the action to the lanes of the env's slice
            DSParams ds = d;
            ds.uniforms = r.uniforms + row;
            ds.actions_f32 = r.actions_f32 + row;
            ds.logprob = r.logprobs + row;
            ds.value = r.values + row;
            float h0[P][2], m0[2], xr0[2];
            ds_group_obs<1, P, LB_DS_FWD_SAMPLE>(ds, env0, col, grp, R, h0, m0, xr0, reinterpret_cast<const float*>(cur));
            const int32_t a = ds_group_actor<1, P, LB_DS_FWD_SAMPLE, false>(ds, W, lane, env0, col, grp, R, h0, m0);
            ds_group_critic<1, P, LB_DS_FWD_SAMPLE, false>(ds, W, lane, env0, col, grp, R, h0, m0);
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
            // the next observations' storage row, from LDS (the wave's LDS writes and reads complete
            // in order)
            float4* orow = stored ? r.obs_next + row * f4 : r.last_obs;
            for (int j = lane; j < j1; j += 64) st_stream(orow + env0 * f4 + j, nxt[j]);
            // lb_ppo_record: the next done row, the finished episode's sums, the VecMonitor return
            float r32 = 0.f;
            if (head) {
                r.rewards[row + env] = rw;
                (stored ? r.dones_next + row : r.last_done)[env] = dn ? 1.f : 0.f;
                if (i == r.steps - 1) {  // what the last lb_step leaves
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
