// lbk8s_dqn64.h — k_dqn_steps64 (lb_dqn_steps64): a DQN train period's vector steps in one launch
// for envs of up to 64 endpoints, the sibling of k_dqn_step (lbk8s_dqn.h), which covers the
// 16-lane slice of R <= 16 rows only.
//
// One wave carries ONE env of R = 17..65 observation rows through all nsteps vector steps
// (StepsEnv<W, 1, 1> of lbk8s_steps.h), with k_dqn_step's functions in k_dqn_step's order per
// env: the explore mask over t .. t + nsteps - 1, the env's random action or the greedy action of
// the Q forward (k_eval_steps64's: MODE 2, TS = ceil(R / 16) set tiles, the actor part of the
// image), the env step, the replay rows.  Bit for bit lb_dqn_step n times, which at these shapes
// is lb_dqn_act + lb_step + lb_replay_add (tests/test_gpu_dqn_steps64.py).
//
// LDS.  Two observation buffers per wave, cur (step i's input) and nxt (its next observations):
// the replay row needs both.  Over the greedy forward the env's registers are parked in nxt, which
// is free until StepsEnv::step writes it, and cur stays intact for the replay rows.  Bytes, 8
// waves per block:
//   TS = 2: actor fragments 45,056 + 2 x 8,448 = 61,952 (W = 32)
//   TS >= 3: VG_ACTOR 39,424 + scratch 4,096 + 2 x 16,640 = 76,800 (W = 64)
// One block per CU, as the siblings: __launch_bounds__(DS_BLOCK, 1).
#pragma once

#include "lbk8s_dqn.h"
#include "lbk8s_steps64.h"

namespace lbk {

// d, e, r, nsteps, sync: k_dqn_step's (sync is required: the device words may coincide).
template <int W, int TS>
__global__ __launch_bounds__(DS_BLOCK, 1) void k_dqn_steps64(DSParams d, Params e, DQNReplay r, int nsteps,
                                                            int32_t* sync) {
    static_assert(TS >= 2 && TS <= 5 && 16 * (TS - 1) < W + 1, "some R <= W + 1 takes TS set tiles");
    constexpr int NWB = DS_BLOCK / 64, OBF4 = steps_obs_f4(W, 1);
    constexpr bool VG = DSGeom<TS, 1, 2>::VG;
    constexpr int IMG = VG ? (int)VG_ACTOR : (int)DS_C1L;
    __shared__ __attribute__((aligned(16))) float Wt[IMG + (VG ? NWB * VG_SCRATCH : 0)];
    __shared__ __attribute__((aligned(16))) float4 OB[NWB][2][OBF4];
    static_assert(sizeof(Wt) + sizeof(OB) <= STEPS64_LDS_MAX, "k_dqn_steps64: the image, the scratch and two buffers per wave");
    const int64_t t = *d.ex.vstep_in;
    const int64_t pos = *r.pos_in;
    uint32_t exm = 0;  // step i explores: bit i (uniform over the launch)
    for (int i = 0; i < nsteps; ++i)
        if (dqn_explores(d.ex, t + i)) exm |= 1u << i;
    const uint32_t all = nsteps >= 32 ? ~0u : (1u << nsteps) - 1u;
    if (exm != all)  // (some step is greedy)
        steps_stage_weights<IMG>(Wt, d.wfrag + (VG ? DS_FLOATS : 0));
    const StepsWave w = steps_wave<VG, IMG>(Wt);
    const int lane = w.lane;
    float* xs = w.xs;
    const int R = d.R;
    const int64_t B = e.B, n4 = B * r.f4;
    float4(*ob)[OBF4] = OB[w.wv];
    for (int64_t gi = w.wave; gi < B; gi += w.nwaves) {
        StepsEnv<W, 1, 1> g;
        g.open(e, nullptr, gi, lane, r.f4);  // (float4s per observation: 2 R <= OBF4, host check)
        const int64_t env = g.env0;
        const int f4 = g.f4;
        for (int j = lane; j < f4; j += 64) ob[0][j] = r.obs[env * f4 + j];
        for (int i = 0; i < nsteps; ++i) {
            const bool explore = (exm >> i) & 1u;
            const int64_t ps = (pos + i) % r.slots;
            float4* cur = ob[i & 1];
            float4* nxt = ob[(i + 1) & 1];
            int a = 0;
            // lb_dqn_act's greedy forward on the LDS observation (lane 0 holds the action and writes
            // d.actions), the env parked in nxt over it
            if (!explore) a = steps_greedy_action<TS, VG>(d, g, Wt, xs, lane, env, R, cur, nxt);
            const int lp = steps64_lane(lane);
            g.relane(lp);
            if (explore && g.live) {  // (lb_dqn_act's random action of every env)
                a = random_action(e, env, g.v.acc3, g.v.s.step);
                if (g.head) d.actions[env] = a;
            }
            g.step(e, a, nxt);
            if (g.head) {
                e.reward[env] = g.rw;
                if (e.rew64) e.rew64[env] = g.reward;
                e.done[env] = (uint8_t)g.dn;
            }
            // the env's replay rows (lb_replay_add's) and obs <- next obs, from LDS (the wave's LDS
            // writes and reads complete in order)
            for (int j = lp; j < f4; j += 64) {
                const float4 o = cur[j], nx = nxt[j];
                const int64_t q = env * f4 + j;
                r.rb_obs[ps * n4 + q] = o;
                r.rb_next_obs[ps * n4 + q] = nx;
                r.obs[q] = nx;
                st_stream(reinterpret_cast<float4*>(e.obs) + q, nx);
            }
            if (g.head) {  // (the lane that wrote the env's reward, done and stats row)
                r.rb_actions[ps * B + env] = a;
                r.rb_rewards[ps * B + env] = g.rw;
                r.rb_dones[ps * B + env] = g.dn ? 1.f : 0.f;
                if (r.ep_sum && g.dn) {
                    r.ep_sum[env] += e.auto_reset ? g.ret : e.ep_stats[env * LB_ST_K];
                    r.ep_cnt[env] += 1.0;
                }
            }
        }
        g.close(e, nullptr);
    }
    // the last block to finish writes the device words (every block has read them); the counter
    // wraps itself to 0 (k_dqn_step)
    __shared__ int last;
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        last = atomicInc(reinterpret_cast<unsigned*>(sync), gridDim.x - 1u) == gridDim.x - 1u;
    }
    __syncthreads();
    if (last && threadIdx.x == 0) {
        *d.ex.explore_out = (int32_t)((exm >> (nsteps - 1)) & 1u);
        *d.ex.vstep_out = t + nsteps;
        *r.pos_out = (pos + nsteps) % r.slots;
    }
}

}  // namespace lbk
