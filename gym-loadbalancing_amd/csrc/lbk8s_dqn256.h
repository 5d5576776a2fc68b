// lbk8s_dqn256.h — k_dqn_steps256 (lb_dqn_steps256): a DQN train period's vector steps in one
// launch for envs of 65 to 256 endpoints, the sibling of k_dqn_steps64 (lbk8s_dqn64.h), which
// covers one endpoint per lane (E <= 64, R <= 65) only.
//
// One wave carries ONE env of R = 66..257 observation rows through all nsteps vector steps: the
// 64 lanes of a wave with EPL = 2 or 4 endpoints per lane (StepsEnv<64, EPL, 1> of lbk8s_steps.h),
// with k_dqn_step's functions in k_dqn_step's order per env: the explore mask over
// t .. t + nsteps - 1, the env's random action or the greedy action of the Q forward
// (k_eval_steps256's at that R: the TS = 5 VALU image up to R = 80, the chunked forward on the
// actor fragments above), the env step, the replay rows.  Bit for bit lb_dqn_step n times, which
// at these shapes is lb_dqn_act + lb_step + lb_replay_add (tests/test_gpu_dqn_steps256.py).
//
//   instance     R          E          forward
//   <2, false>   66..80     65..80     steps_greedy_action<5, true>, the env parked over it
//   <2, true>    81..129    80..128    ds_chunked_set<2, DSRowsLds> (lbk8s_ds_chunked.h): the function
//   <4, true>    130..257   129..256   k_deepsets_fwd_big<2> runs per set, the rows read from the LDS image
//
// LDS.  ONE observation buffer per wave in all three instances, as k_eval_steps256, where
// k_dqn_steps64 keeps two (cur and nxt): two buffers of 514 float4s for 8 waves are 131,584 bytes,
// with the actor fragments 176,640, over the CU's 163,840.  The replay row's rb_obs half is
// therefore stored from the image at the top of the step, before the forward (which without
// chunks parks the env over that image) and before StepsEnv::step writes the next rows into it;
// rb_next_obs, obs and the streamed next observations are stored from the same buffer after the
// step.  The addresses are distinct, and where the ring wraps inside a launch the same lane
// rewrites the same address in program order, so the bytes left are those of the two-buffer
// scheme.  Bytes, 8 waves per block (k_eval_steps256's):
//   <2, false>  VG_ACTOR 39,424 + scratch 4,096 + 8 x 258 x 16 = 33,024:  76,544
//   <2, true>   actor fragments 45,056 + 33,024:                          78,080
//   <4, true>   actor fragments 45,056 + 8 x 514 x 16 = 65,792:          110,848
// One block per CU, as the siblings: __launch_bounds__(DS_BLOCK, 1).
#pragma once

#include "lbk8s_dqn.h"
#include "lbk8s_steps256.h"

namespace lbk {

// d, e, r, nsteps, sync: k_dqn_step's (sync is required: the device words may coincide).
template <int EPL, bool CHUNK>
__global__ __launch_bounds__(DS_BLOCK, 1) void k_dqn_steps256(DSParams d, Params e, DQNReplay r, int nsteps,
                                                             int32_t* sync) {
    static_assert(CHUNK || EPL == 2, "R <= LB_DS_MAX_ELEMENTS rows are E <= 128 endpoints");
    constexpr int NWB = DS_BLOCK / 64, OBF4 = steps_obs_f4(64, EPL), TS = (LB_DS_MAX_ELEMENTS + 15) / 16;
    constexpr bool VG = !CHUNK;
    static_assert(CHUNK || DSGeom<TS, 1, 2>::VG, "the forward of TS = 5 set tiles reads the VALU image");
    constexpr int IMG = VG ? (int)VG_ACTOR : (int)DS_C1L;
    __shared__ __attribute__((aligned(16))) float Wt[IMG + (VG ? NWB * VG_SCRATCH : 0)];
    __shared__ __attribute__((aligned(16))) float4 OB[NWB][OBF4];
    static_assert(sizeof(Wt) + sizeof(OB) <= STEPS64_LDS_MAX, "k_dqn_steps256: the image, the scratch and one buffer per wave");
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
    float4* ob = OB[w.wv];
    for (int64_t gi = w.wave; gi < B; gi += w.nwaves) {
        StepsEnv<64, EPL, 1> g;
        g.open(e, nullptr, gi, lane, r.f4);  // (float4s per observation: 2 R <= OBF4, host check)
        const int64_t env = g.env0;
        const int f4 = g.f4;
        for (int j = lane; j < f4; j += 64) ob[j] = r.obs[env * f4 + j];
        for (int i = 0; i < nsteps; ++i) {
            const bool explore = (exm >> i) & 1u;
            const int64_t ps = (pos + i) % r.slots;
            // the replay row's observation half (lb_replay_add's), from the one buffer while it still
            // holds step i's input (the wave's LDS writes and reads complete in order)
            {
                const int l0 = steps64_lane(lane);
                for (int j = l0; j < f4; j += 64) r.rb_obs[ps * n4 + env * f4 + j] = ob[j];
            }
            int a = 0;
            // lb_dqn_act's greedy forward on the LDS observation (lane 0 holds the action and writes
            // d.actions): chunked, the env in registers next to it; else the env parked in the image
            if (!explore) {
                if constexpr (CHUNK) {
                    const int ln = steps64_lane(lane);
                    g.relane(ln);
                    const int32_t act = ds_chunked_set<2>(d, Wt, Wt, DSRowsLds{ob}, env, ln, R);
                    a = __shfl(act, 0);
                } else {
                    a = steps_greedy_action<TS, VG>(d, g, Wt, xs, lane, env, R, ob, ob);
                }
            }
            const int lp = steps64_lane(lane);
            g.relane(lp);
            if (explore && g.live) {  // (lb_dqn_act's random action of every env)
                a = random_action(e, env, g.v.acc3, g.v.s.step);
                if (g.head) d.actions[env] = a;
            }
            g.step(e, a, ob);
            if (g.head) {
                e.reward[env] = g.rw;
                if (e.rew64) e.rew64[env] = g.reward;
                e.done[env] = (uint8_t)g.dn;
            }
            // the row's next observations and obs <- next obs, from the same buffer
            for (int j = lp; j < f4; j += 64) {
                const float4 nx = ob[j];
                const int64_t q = env * f4 + j;
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
