// lbk8s_ppo256.h — k_ppo_steps256 (lb_ppo_steps256): the vector steps of a PPO rollout in one launch
// for envs of 65 to 256 endpoints, the sibling of k_ppo_steps64 (lbk8s_steps64.h), which covers one
// endpoint per lane (E <= 64, R <= 65) only.
//
// One wave carries ONE env of R = 65..257 observation rows through all the steps of the launch: the
// 64 lanes of a wave with EPL = 2 or 4 endpoints per lane (StepsEnv<64, EPL, 1> of lbk8s_steps.h),
// with k_ppo_steps64's loop body per env: the sampling forward on the LDS observation, the env
// step, the next observations' storage row streamed out from LDS, the head lane's reward, done and
// last-step words, lb_ppo_record's sums and log.  The forward is lb_ds_sample's at that R, per set
// column and per row, so the bits are its (tests/test_gpu_ppo_steps256.py):
//
//   instance     R          E          forward
//   <2, false>   65..80     65..80     ds_group_obs / ds_group_actor / ds_group_critic<5, 1, SAMPLE, VG>
//                                      on the VALU image (k_ppo_steps64<64, 5>'s), the env parked over it
//   <2, true>    81..129    80..128    ds_chunked_set<LB_DS_FWD_SAMPLE, DSRowsLds> (lbk8s_ds_chunked.h): the
//   <4, true>    130..257   129..256   function k_deepsets_fwd_big<SAMPLE> runs per set (actor passes,
//                                      ds_sample_wave, critic), here with the rows read from the wave's
//                                      LDS image and the epilogue's fragments from global memory (below);
//                                      the env in registers next to it
//
// LDS.  Neither weight image fits next to the observation buffers the siblings keep (the CU has
// STEPS64_LDS_MAX = 163,840 bytes; 8 waves per block, one buffer per wave):
//   chunked   the fragment image with the critic is DS_FLOATS = 33,860 floats = 135,440 B; with
//             buffers of 2 (64 EPL + 1) float4s, 33,024 / 65,792 B, that is 168,464 / 201,232 B.
//             The chunk loops read only the fragments below DS_C3L (both networks' layers 1 and 2,
//             the actor's layer 3: 20,480 floats = 81,920 B).  The rest -- the critic's layer 3 on
//             the set's mean and max and rho, 13,380 floats -- is read once per set and step, after
//             the last chunk, as whole 64-float rows (We[.. + lane]): those reads go to the image in
//             global memory (d.wfrag; it stays in L2), the same values in the same operations:
//             ds_chunked_set's second weight pointer.
//               <2, true>   81,920 + 33,024 = 114,944 B
//               <4, true>   81,920 + 65,792 = 147,712 B
//   <2, false> the VALU image VG_RHO = 32,772 floats = 131,088 B and the waves' scratch 4,096 B
//             leave 28,656 B.  The forward holds the observation in its fragments, so a buffer
//             needs the larger of an R = 80 observation (160 float4s) and the parked env
//             (StepsEnv::PARK_WORDS = 6 x 64 x 2 + 32 = 800 words = 200 float4s), not the 258
//             float4s of E = 128: 8 x 200 x 16 = 25,600 B, 160,784 B in all.
// One block per CU, as the siblings: __launch_bounds__(DS_BLOCK, 1).
#pragma once

#include "lbk8s_ppo.h"
#include "lbk8s_steps256.h"

namespace lbk {

// lb_ppo_steps256: k_ppo_steps' arguments; one env of 64 lanes with EPL endpoints each per wave.
template <int EPL, bool CHUNK>
__global__ __launch_bounds__(DS_BLOCK, 1) void k_ppo_steps256(DSParams d, Params e, PPOSteps r) {
    static_assert(CHUNK || EPL == 2, "R <= LB_DS_MAX_ELEMENTS rows are E <= 128 endpoints");
    constexpr int NWB = DS_BLOCK / 64, TS = (LB_DS_MAX_ELEMENTS + 15) / 16;
    constexpr bool VG = !CHUNK;
    static_assert(CHUNK || DSGeom<TS, 1, LB_DS_FWD_SAMPLE>::VG, "the forward of TS = 5 set tiles reads the VALU image");
    using Env = StepsEnv<64, EPL, 1>;
    // the buffer of a wave: the whole observation image where the chunked forward reads it; else the
    // parked env or an observation of LB_DS_MAX_ELEMENTS rows, whichever is larger
    constexpr int PARK_F4 = (Env::PARK_WORDS + 3) / 4;
    constexpr int OBF4 = CHUNK ? steps_obs_f4(64, EPL) : (PARK_F4 > 2 * LB_DS_MAX_ELEMENTS ? PARK_F4 : 2 * LB_DS_MAX_ELEMENTS);
    static_assert(CHUNK ? 2 * STEPS256_MAX_R <= steps_obs_f4(64, 4) : (4 * OBF4 >= Env::PARK_WORDS && OBF4 >= 2 * 16 * TS),
                  "the buffer holds the observation's rows and, without chunks, the parked env");
    constexpr int IMG = VG ? (int)VG_RHO : (int)DS_C3L;
    __shared__ __attribute__((aligned(16))) float Wt[IMG + (VG ? NWB * VG_SCRATCH : 0)];
    __shared__ __attribute__((aligned(16))) float4 OB[NWB][OBF4];
    static_assert(sizeof(Wt) + sizeof(OB) <= STEPS64_LDS_MAX, "k_ppo_steps256: the image, the scratch and one buffer per wave");
    steps_stage_weights<IMG>(Wt, d.wfrag + (VG ? DS_FLOATS : 0));
    const StepsWave w = steps_wave<VG, IMG>(Wt);
    const int lane = w.lane;
    float* xs = w.xs;
    const int R = d.R;
    const int64_t B = e.B;
    float4* ob = OB[w.wv];
    for (int64_t gi = w.wave; gi < B; gi += w.nwaves) {
        Env g;
        g.open(e, &r.rec, gi, lane, 2 * R);  // (float4s per observation <= OBF4: host check)
        const int64_t env = g.env0;
        const int f4 = g.f4;
        for (int j = lane; j < f4; j += 64) ob[j] = reinterpret_cast<const float4*>(r.obs)[env * f4 + j];
        for (int i = 0; i < r.steps; ++i) {
            const int64_t row = (int64_t)i * B;
            const bool stored = i < r.store_rows;
            const int ln = steps64_lane(lane);
            g.relane(ln);
            // lb_ds_sample on the LDS observation
            DSParams ds = d;
            ds.uniforms = r.uniforms + row;
            ds.actions_f32 = r.actions_f32 + row;
            ds.logprob = r.logprobs + row;
            ds.value = r.values + row;
            int32_t a;
            if constexpr (CHUNK) {
                // Wt holds the fragments below DS_C3L, the critic's epilogue reads the image in global
                // memory (every lane holds the action: a scalar)
                a = __builtin_amdgcn_readfirstlane(
                    ds_chunked_set<LB_DS_FWD_SAMPLE>(ds, Wt, d.wfrag, DSRowsLds{ob}, env, ln, R));
            } else {
                // into the fragments h0 (the image is free after it), the env parked over the forward
                // as in k_ppo_steps64
                const int col = ln & 15, grp = ln >> 4;
                float h0[TS][2], m0[2], xr0[2];
                ds_group_obs<TS, 1, LB_DS_FWD_SAMPLE>(ds, env, col, grp, R, h0, m0, xr0, reinterpret_cast<const float*>(ob));
                g.park(ob);
                uint32_t wo = 0;
                asm volatile("" : "+s"(wo));
                const float* Wc = Wt + wo;
                const int32_t act = ds_group_actor<TS, 1, LB_DS_FWD_SAMPLE, VG>(ds, Wc, ln, env, col, grp, R, h0, m0, xs);
                ds_group_critic<TS, 1, LB_DS_FWD_SAMPLE, VG>(ds, Wc, ln, env, col, grp, R, h0, m0, xs);
                a = __shfl(act, 0);  // (row group 0 holds it) to the lanes of the env's slice
            }
            const int lp = steps64_lane(lane);
            g.relane(lp);
            if constexpr (!CHUNK) g.unpark(ob);
            g.step(e, a, ob);
            // the next observations' storage row, from LDS (the wave's LDS writes and reads complete
            // in order)
            float4* orow = stored ? r.obs_next + row * f4 : r.last_obs;
            for (int j = lp; j < f4; j += 64) st_stream(orow + env * f4 + j, ob[j]);
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
        }
        g.close(e, &r.rec);
    }
}

}  // namespace lbk
