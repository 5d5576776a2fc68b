// lbk8s_ppo.h — lb_ppo_steps: the vector steps of a PPO rollout (envs/ppo_deepset.py:160-190) in
// ONE launch.
//
// With fused_act and fused_bookkeeping a PPO vector step is three launches: lb_ds_sample (the
// deep-sets forward with the categorical draw), lb_step and lb_ppo_record (the next done row, the
// finished episodes' sums, the VecMonitor log).  Over a rollout the policy is fixed, the uniforms
// are drawn before it starts and every output is per env, so -- as k_dqn_step does for a DQN train
// period -- one wave carries its P envs through all the steps (StepsEnv<16, 1, P>, lbk8s_steps.h: the
// env, the float32 running return and the episode sums in registers, the group's observations in
// the two-buffer LDS image that the forward reads and the storage rows are copied from).  Bit for
// bit the 3 x steps launches (tests/test_gpu_ppo_steps.py).
//
// The forward is lb_ds_sample's at R <= 16: the MFMA-fragment image (DS_FLOATS, staged once per
// block) under ds_group_obs / ds_group_actor / ds_group_critic<1, P, LB_DS_FWD_SAMPLE>.  Its
// arithmetic is per set column, so the bits do not depend on P (lb_ds_sample itself takes P = 1,
// 2 or 4 by the batch).  LDS: the image (135,440 B) plus 8 waves x 2 buffers x P x 34
// float4s = 152,848 B at P = 2 (P = 4 would pass 160 KB).
//
// TL (k_ppo_steps<P, true>: lb_ppo_steps_tl, include/lbk8s_abi_ppo_tl.h): lb_step writes the finished
// envs' terminal observations (e.term_obs, slice_apply) and each step leaves its term_values row:
// +0 for an env that goes on and, where an env of the group finished (a wave-uniform test: 1 step
// in episode_length), lb_ds_value_where's critic on the group's terminal observations, read back
// from e.term_obs once the wave's stores are complete (no third LDS buffer fits, and none is
// needed).  The step's own critic moves behind the env step there (its input is the six fragment
// words of ds_group_obs, nothing of the env), so both critics are ONE site of the code, run once or
// twice: two inlined copies spilled.  The flagged critic (DS_FWD_WHERE) with every flag set is the
// sampling forward's critic, and its arithmetic is per set column: lb_ds_sample's and
// lb_ds_value_where's bits.
#pragma once

#include <type_traits>

#include "lbk8s_deepsets.h"
#include "lbk8s_steps.h"

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
    StepsRecord rec;          // lb_ppo_record's sums and episode log
};

struct PPOStepsTL : PPOSteps {
    float* term_values;       // [steps][B]
};

// d: the forward (lb_ds_sample's DSParams without masks or logits: actions = the caller's int32
// action buffer); e: the env (lb_step's Params: done, ep_stats, no terminal obs -- TL: the call's
// terminal_obs; obs / reward are the per-step rows of r).
template <int P, bool TL = false>
__global__ __launch_bounds__(DS_BLOCK, 2) void k_ppo_steps(DSParams d, Params e,
                                                           std::conditional_t<TL, PPOStepsTL, PPOSteps> r) {
    static_assert(P == 1 || P == 2, "envs per wave iteration (the LDS budget)");
    constexpr int NWB = DS_BLOCK / 64;
    __shared__ __attribute__((aligned(16))) float W[DS_FLOATS];
    __shared__ __attribute__((aligned(16))) float4 OB[NWB][2][P * steps_obs_f4(16, 1)];
    for (int i = threadIdx.x * 4; i < DS_FLOATS; i += DS_BLOCK * 4)
        *reinterpret_cast<float4*>(W + i) = *reinterpret_cast<const float4*>(d.wfrag + i);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
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
        const int f4 = g.f4;
        for (int j = lane; j < g.j1; j += 64) ob[0][j] = reinterpret_cast<const float4*>(r.obs)[env0 * f4 + j];
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
            if constexpr (!TL) ds_group_critic<1, P, LB_DS_FWD_SAMPLE, false>(ds, W, lane, env0, col, grp, R, h0, m0);
            g.step(e, a, nxt);
            // the next observations' storage row, from LDS (the wave's LDS writes and reads complete
            // in order)
            float4* orow = stored ? r.obs_next + row * f4 : r.last_obs;
            for (int j = lane; j < g.j1; j += 64) st_stream(orow + env0 * f4 + j, nxt[j]);
            // the reward and next done rows, then lb_ppo_record's sums and log
            if (g.head) {
                r.rewards[row + env] = g.rw;
                (stored ? r.dones_next + row : r.last_done)[env] = g.dn ? 1.f : 0.f;
                if (i == r.steps - 1) {  // what the last lb_step leaves
                    e.rew64[env] = g.reward;
                    e.done[env] = (uint8_t)g.dn;
                }
            }
            g.record(e, r.rec, a, i);
            if constexpr (TL) {
                // the step's critic, then lb_ds_value_where(frag, terminal_obs, done_out, ..) on the
                // group where an env of it finished (fin: the finished envs' head lanes, 16 s)
                const uint64_t fin = __ballot(g.head && g.dn);
                if (g.head && !g.dn) r.term_values[row + env] = 0.f;
                uint32_t fl = ~0u;
#pragma clang loop unroll(disable)
                for (int pass = 0;; ++pass) {
                    ds_group_critic<1, P, DS_FWD_WHERE, false>(ds, W, lane, env0, col, grp, R, h0, m0, nullptr, nullptr, fl);
                    if (pass || !fin) break;
                    fl = 0;
#pragma unroll
                    for (int s = 0; s < P; ++s) fl |= (uint32_t)((fin >> (16 * s)) & 1) << s;
                    __threadfence();  // the slices' terminal rows, stored by other lanes of the wave
                    ds.obs = e.term_obs;
                    ds.value = r.term_values + row;
                    ds_group_obs<1, P, DS_FWD_WHERE>(ds, env0, col, grp, R, h0, m0, xr0, nullptr, fl);
                }
            }
        }
        g.close(e, &r.rec);
    }
}

}  // namespace lbk
