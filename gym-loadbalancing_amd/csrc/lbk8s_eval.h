// lbk8s_eval.h — lb_eval_steps: the vector steps of a greedy evaluation (run_test_deepset.py:44-98)
// in ONE launch.
//
// A step of lbk8s/evaluate.py:run_test is the greedy forward (lb_ds_q_argmax), lb_step and, for
// the finished episodes' sums and the VecMonitor log, lb_ppo_record.  Over an evaluation the
// network and the masks are fixed and every output is per env, so -- as k_dqn_step does for a DQN
// train period and k_ppo_steps for a PPO rollout -- one wave carries its P envs through all the
// steps (StepsEnv<16, 1, P>, lbk8s_steps.h: the env, the float32 running return and the episode sums in
// registers, the group's observations in the two-buffer LDS image that the forward reads).  Bit
// for bit the 3 x steps launches (tests/test_gpu_eval_steps.py).
//
// The forward is k_dqn_step's greedy one: the actor part of the VALU image (VG_ACTOR floats at
// frag + DS_FLOATS, staged once per block) under ds_group_obs / ds_group_actor<1, P, 2, true>.  Its
// arithmetic is per set column, so the bits do not depend on P (lb_ds_q_argmax itself takes P = 1
// or 2 by the batch).  LDS at P = 2: the image and scratch (39,424 + 8,192 B) plus 8 waves x 2
// buffers x P x 34 float4s (17,408 B) = 65,024 B: two blocks per CU.
//
// What a step leaves in global memory is its trace row (actions_all / rewards_all / dones_all,
// each optional) and, when an episode ends, the ep_stats row and the log row; the observations,
// the env state and the per-env words of the last lb_step are written once, after the last step.
#pragma once

#include "lbk8s_deepsets.h"
#include "lbk8s_steps.h"

namespace lbk {

struct EvalSteps {
    int steps;
    float4* obs;           // [B][2 R]: step 0's input; <- the observations after the last step
    int32_t* actions_all;  // [steps][B] or NULL
    float* rewards_all;    // [steps][B] or NULL
    uint8_t* dones_all;    // [steps][B] or NULL
    StepsRecord rec;       // lb_ppo_record's sums and episode log
};

// Step i's trace row (row: i B) and, after the last step, what the last lb_step leaves: written by
// the head lane of env (g: the env's StepsEnv after step(), a: the action it took)
template <typename G>
__device__ __forceinline__ void eval_trace_row(const Params& e, const EvalSteps& r, const G& g, int64_t row, int64_t env,
                                               int32_t a, int i) {
    if (!g.head) return;
    if (r.actions_all) r.actions_all[row + env] = a;
    if (r.rewards_all) r.rewards_all[row + env] = g.rw;
    if (r.dones_all) r.dones_all[row + env] = (uint8_t)g.dn;
    if (i == r.steps - 1) {
        e.reward[env] = g.rw;
        e.rew64[env] = g.reward;
        e.done[env] = (uint8_t)g.dn;
    }
}

// d: the forward (lb_ds_q_argmax's DSParams without obs or Q values: the actor-only image, masks,
// actions = the caller's int32 action buffer); e: the env (lb_step's Params: reward, done,
// ep_stats, no obs and no terminal obs).
template <int P>
__global__ __launch_bounds__(DS_BLOCK, 2) void k_eval_steps(DSParams d, Params e, EvalSteps r) {
    static_assert(P == 1 || P == 2, "envs per wave iteration (the VALU Gamma takes at most two)");
    constexpr int NWB = DS_BLOCK / 64;
    __shared__ __attribute__((aligned(16))) float W[VG_ACTOR + NWB * P * VG_SCRATCH];
    __shared__ __attribute__((aligned(16))) float4 OB[NWB][2][P * steps_obs_f4(16, 1)];
    static_assert(sizeof(W) + sizeof(OB) <= 80 * 1024, "k_eval_steps: two blocks per CU");
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
    const int64_t B = e.B, groups = (B + P - 1) / P;
    float4(*ob)[P * steps_obs_f4(16, 1)] = OB[wv];
    for (int64_t gi = wave; gi < groups; gi += nwaves) {
        StepsEnv<16, 1, P> g;
        g.open(e, &r.rec, gi, lane, 2 * R);  // (float4s per observation <= steps_obs_f4(16, 1): host check)
        const int64_t env0 = g.env0, env = g.env;
        for (int j = lane; j < g.j1; j += 64) ob[0][j] = r.obs[env0 * g.f4 + j];
        for (int i = 0; i < r.steps; ++i) {
            const float4* cur = ob[i & 1];
            float4* nxt = ob[(i + 1) & 1];
            const int64_t row = (int64_t)i * B;
            // lb_ds_q_argmax on the LDS observations (lane s holds env0 + s's action), then to the
            // lanes of the env's slice
            float h0[P][2], m0[2], xr0[2];
            ds_group_obs<1, P, 2>(d, env0, col, grp, R, h0, m0, xr0, reinterpret_cast<const float*>(cur));
            const int32_t act = ds_group_actor<1, P, 2, true>(d, W, lane, env0, col, grp, R, h0, m0, xs);
            const int32_t a = __shfl(act, g.s < P ? g.s : 0);
            g.step(e, a, nxt);
            // the step's trace row, then lb_ppo_record's sums and log
            eval_trace_row(e, r, g, row, env, a, i);
            g.record(e, r.rec, a, i);
        }
        // obs <- the observations after the last step, from LDS (the wave's LDS writes and reads
        // complete in order), then the env
        const float4* fin = ob[r.steps & 1];
        for (int j = lane; j < g.j1; j += 64) r.obs[env0 * g.f4 + j] = fin[j];
        g.close(e, &r.rec);
    }
}

}  // namespace lbk
