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
//   <2, true>    81..129    80..128    ds_chunked_sample_lds: k_deepsets_fwd_big<SAMPLE>'s actor
//   <4, true>    130..257   129..256   passes, ds_sample_wave and critic, the set read from the wave's
//                                      LDS image, the env in registers next to it
//
// The chunked forward's loop is written out here a second time on purpose, as
// ds_chunked_argmax_lds repeats the greedy one: k_deepsets_fwd_big keeps its code.
//
// LDS.  Neither weight image fits next to the observation buffers the siblings keep (the CU has
// STEPS64_LDS_MAX = 163,840 bytes; 8 waves per block, one buffer per wave):
//   chunked   the fragment image with the critic is DS_FLOATS = 33,860 floats = 135,440 B; with
//             buffers of 2 (64 EPL + 1) float4s, 33,024 / 65,792 B, that is 168,464 / 201,232 B.
//             The chunk loops read only the fragments below DS_C3L (both networks' layers 1 and 2,
//             the actor's layer 3: 20,480 floats = 81,920 B).  The rest -- the critic's layer 3 on
//             the set's mean and max and rho, 13,380 floats -- is read once per set and step, after
//             the last chunk, as whole 64-float rows (W[.. + lane]): those reads go to the image in
//             global memory (d.wfrag; it stays in L2), the same values in the same operations.
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

// k_deepsets_fwd_big<LB_DS_FWD_SAMPLE> for one set (actor and critic on, no logits row: the
// DSParams of ppo_steps_params), statement for statement, on the R rows of the LDS image ob.
// W: the fragments below DS_C3L in LDS; Wg: the whole fragment image in global memory, read
// from DS_C3L on.  The lane of the action's row writes p.actions / actions_f32 / logprob [env],
// lane 0 p.value[env]; every lane returns the action.
__device__ __forceinline__ int32_t ds_chunked_sample_lds(const DSParams& p, const float* W, const float* Wg,
                                                         const float4* ob, int64_t env, int lane, int R) {
    const int col = lane & 15, grp = lane >> 4;
    const int nch = (R + 16 * DS_CT - 1) / (16 * DS_CT);
    float h0[DS_CT][2], h1[DS_CT][16], h2[DS_CT][16];
    float m0[2] = {-INFINITY, -INFINITY};
    for (int c = 0; c < nch; ++c) {
        load_obs_chunk_lds(ob, 16 * DS_CT * c, R, col, grp, h0);
        chunk_max_acc<2>(h0, m0, 16 * DS_CT * c, col, R);
    }
    row_reduce<true>(m0);
    int32_t act;
    {
        float m1[16], m2[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) m1[k] = m2[k] = -INFINITY;
        // (an opaque offset per chunk: the weight fragments are re-read from LDS in every chunk)
        for (int c = 0; c < nch; ++c) {
            uint32_t wo = 0;
            asm volatile("" : "+s"(wo));
            const float* Wc = W + wo;
            load_obs_chunk_lds(ob, 16 * DS_CT * c, R, col, grp, h0);
            eq_layer<DS_CT, 1, 2, 1>(Wc + DS_A1L, Wc + DS_A1G, h0, m0, h1, lane);
            chunk_max_acc<16>(h1, m1, 16 * DS_CT * c, col, R);
        }
        row_reduce<true>(m1);
        for (int c = 0; c < nch; ++c) {
            uint32_t wo = 0;
            asm volatile("" : "+s"(wo));
            const float* Wc = W + wo;
            load_obs_chunk_lds(ob, 16 * DS_CT * c, R, col, grp, h0);
            eq_layer<DS_CT, 1, 2, 1>(Wc + DS_A1L, Wc + DS_A1G, h0, m0, h1, lane);
            eq_layer<DS_CT, 1, 16, 2>(Wc + DS_A2L, Wc + DS_A2G, h1, m1, h2, lane);
            chunk_max_acc<16>(h2, m2, 16 * DS_CT * c, col, R);
        }
        row_reduce<true>(m2);
        const float* G = W + DS_A3G + 16 * grp;
        float gl = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) gl += G[k * 64] * m2[k];
        gl += __shfl_xor(gl, 16);
        gl += __shfl_xor(gl, 32);
        // the set's masked logits stay in registers for the draw, lane l keeps rows l, 64 + l, ..
        // (row 32 c + 16 t + col is lane (col, 2 (c & 1) + t)'s slot c >> 1)
        float lgr[DS_SLOTS];
#pragma unroll
        for (int j = 0; j < DS_SLOTS; ++j) lgr[j] = -INFINITY;
        for (int c = 0; c < nch; ++c) {
            uint32_t wo = 0;
            asm volatile("" : "+s"(wo));
            const float* Wc = W + wo;
            load_obs_chunk_lds(ob, 16 * DS_CT * c, R, col, grp, h0);
            eq_layer<DS_CT, 1, 2, 1>(Wc + DS_A1L, Wc + DS_A1G, h0, m0, h1, lane);
            eq_layer<DS_CT, 1, 16, 2>(Wc + DS_A2L, Wc + DS_A2G, h1, m1, h2, lane);
#pragma unroll
            for (int t = 0; t < DS_CT; ++t) {
                float v = 0.f;
#pragma unroll
                for (int k = 0; k < 16; ++k) v += Wc[DS_A3L + 16 * grp + k * 64] * h2[t][k];
                v += __shfl_xor(v, 16);
                v += __shfl_xor(v, 32);
                const int row = 16 * DS_CT * c + 16 * t + col;
                if (row >= R) continue;
                if (grp == 2 * (c & 1) + t) {
                    const float q = (!p.masks || p.masks[env * R + row]) ? gl + v : -1e8f;
#pragma unroll
                    for (int j = 0; j < DS_SLOTS; ++j) lgr[j] = j == (c >> 1) ? q : lgr[j];
                }
            }
        }
        act = ds_sample_wave(p, lgr, env, lane);
    }
    // critic: the max of c1, then the max and the sum of c2, then layer 3 / rho
    float mc1[16], mc2[16], sm[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        mc1[k] = mc2[k] = -INFINITY;
        sm[k] = 0.f;
    }
    for (int c = 0; c < nch; ++c) {
        uint32_t wo = 0;
        asm volatile("" : "+s"(wo));
        const float* Wc = W + wo;
        load_obs_chunk_lds(ob, 16 * DS_CT * c, R, col, grp, h0);
        eq_layer<DS_CT, 1, 2, 2>(Wc + DS_C1L, Wc + DS_C1G, h0, m0, h1, lane);
        chunk_max_acc<16>(h1, mc1, 16 * DS_CT * c, col, R);
    }
    row_reduce<true>(mc1);
    for (int c = 0; c < nch; ++c) {
        uint32_t wo = 0;
        asm volatile("" : "+s"(wo));
        const float* Wc = W + wo;
        load_obs_chunk_lds(ob, 16 * DS_CT * c, R, col, grp, h0);
        eq_layer<DS_CT, 1, 2, 2>(Wc + DS_C1L, Wc + DS_C1G, h0, m0, h1, lane);
        eq_layer<DS_CT, 1, 16, 2>(Wc + DS_C2L, Wc + DS_C2G, h1, mc1, h2, lane);
        chunk_max_acc<16>(h2, mc2, 16 * DS_CT * c, col, R);
#pragma unroll
        for (int t = 0; t < DS_CT; ++t)
            if (16 * DS_CT * c + 16 * t + col < R)
#pragma unroll
                for (int k = 0; k < 16; ++k) sm[k] += h2[t][k];
    }
    row_reduce<true>(mc2);
    row_reduce<false>(sm);
    // (from here on the fragments are read from global memory, whole rows of 64 lanes)
    const float invR = 1.0f / (float)R;
    float mean[16];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        dsf4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 16; ++k) acc = mfma4(Wg[DS_C3G + (nt * 16 + k) * 64 + lane], mc2[k], acc);
#pragma unroll
        for (int k = 0; k < 16; ++k) acc = mfma4(Wg[DS_C3L + (nt * 16 + k) * 64 + lane], sm[k] * invR, acc);
#pragma unroll
        for (int i = 0; i < 4; ++i) mean[4 * nt + i] = acc[i];
    }
    float r1[16];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        dsf4 acc;
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = Wg[DS_R1B + 16 * nt + 4 * grp + i];
#pragma unroll
        for (int k = 0; k < 16; ++k) acc = mfma4(Wg[DS_R1W + (nt * 16 + k) * 64 + lane], mean[k], acc);
#pragma unroll
        for (int i = 0; i < 4; ++i) r1[4 * nt + i] = act_elu(acc[i]);
    }
    dsf4 v = {Wg[DS_R2B], 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 16; ++k) v = mfma4(Wg[DS_R2W + k * 64 + lane], r1[k], v);
    if (lane == 0) p.value[env] = v[0];
    return act;
}

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
                // (every lane holds the action: a scalar)
                a = __builtin_amdgcn_readfirstlane(ds_chunked_sample_lds(ds, Wt, d.wfrag, ob, env, ln, R));
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
