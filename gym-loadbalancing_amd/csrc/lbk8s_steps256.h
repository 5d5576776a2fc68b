// lbk8s_steps256.h — the one-launch greedy evaluation for envs of 65 to 256 endpoints:
// k_eval_steps256 (lb_eval_steps256), the sibling of k_eval_steps64 (lbk8s_steps64.h), which
// covers one endpoint per lane (E <= 64, R <= 65) only.
//
// One wave carries ONE env of R = 66..257 observation rows through all the steps of the launch.
// The env sits in the slice layout of its geometry below 32,768 envs: the 64 lanes of a wave with
// EPL = 2 or 4 endpoints per lane (StepsEnv<64, EPL, 1> of lbk8s_steps.h).
// The forward is lb_ds_q_argmax's at that R, per set column and per row, so the bits are its:
//
//   CHUNK  R          EPL   forward
//   no     66..80     2     ds_group_obs / ds_group_actor<5, 1, 2, VG> on the VALU actor image
//                           (k_eval_steps64<64, 5>'s), the env parked in the image over it
//   yes    81..257    2, 4  k_deepsets_fwd_big<2>'s chunked greedy forward (the max pass over obs,
//                           three passes over the 32-row chunks, first maximum wins, masked rows at
//                           -1e8) on the actor fragments, the set's rows read from the wave's LDS
//                           observation image (ds_reads: load_obs_chunk_lds)
//
// The chunked forward's loop is written out here a second time on purpose, as k_rollout_slice_k8s
// repeats k_rollout_slice's: k_deepsets_fwd_big keeps its code.
//
// LDS.  The observation image is one buffer of 2 (64 EPL + 1) float4s per wave (258 / 514: the
// chunked forward reads it in every pass, StepsEnv::step then writes the next rows into it; a
// wave's LDS operations complete in order).  Without chunks the forward holds the observation in
// its fragments and the image holds the parked env over it: 6 x 64 x 2 + 32 = 800 words, more
// than the 640 of an R = 80 image and fewer than the buffer's 1,032.  Bytes, 8 waves per block:
//   <2, false>  VG_ACTOR 39,424 + scratch 4,096 + 8 x 258 x 16 = 33,024:  76,544
//   <2, true>   actor fragments 45,056 + 33,024:                          78,080
//   <4, true>   actor fragments 45,056 + 8 x 514 x 16 = 65,792:          110,848
// One block per CU (ds_grid_spread), so a lane has 256 registers: __launch_bounds__(DS_BLOCK, 1).
// The chunked forward is built for 128 of them, so the env stays in registers next to it.
#pragma once

#include "lbk8s_deepsets.h"
#include "lbk8s_eval.h"
#include "lbk8s_slice.h"
#include "lbk8s_steps.h"
#include "lbk8s_steps64.h"

namespace lbk {

constexpr int STEPS256_MAX_R = LB_DS_MAX_ELEMENTS_FWD;
static_assert(2 * STEPS256_MAX_R <= steps_obs_f4(64, 4), "the LDS observation image holds R <= 257 rows");

// load_obs_chunk (lbk8s_deepsets.h) from an LDS image: the same words, read by ds_reads (a generic
// pointer to LDS compiles to flat loads)
typedef __attribute__((address_space(3))) const float lds_cfloat;
__device__ __forceinline__ void load_obs_chunk_lds(const float4* img, int row0, int R, int col, int grp,
                                                   float (&h0)[DS_CT][2]) {
    lds_cfloat* x = (lds_cfloat*)(img);
#pragma unroll
    for (int t = 0; t < DS_CT; ++t) {
        const int row = row0 + 16 * t + col;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) h0[t][kk] = row < R ? x[row * 8 + 4 * kk + grp] : 0.f;
    }
}

// k_deepsets_fwd_big<2>'s actor (its ARGMAX path, statement for statement) on the set of R rows in
// the LDS image ob; W: the actor fragments (DS_C1L floats of wfrag) in LDS.  Lane 0 returns the
// action and writes it to p.actions[env], as the forward does.
__device__ __forceinline__ int32_t ds_chunked_argmax_lds(const DSParams& p, const float* W, const float4* ob, int64_t env,
                                                         int lane, int R) {
    const int col = lane & 15, grp = lane >> 4;
    const int nch = (R + 16 * DS_CT - 1) / (16 * DS_CT);
    float h0[DS_CT][2], h1[DS_CT][16], h2[DS_CT][16];
    float m0[2] = {-INFINITY, -INFINITY};
    for (int c = 0; c < nch; ++c) {
        load_obs_chunk_lds(ob, 16 * DS_CT * c, R, col, grp, h0);
        chunk_max_acc<2>(h0, m0, 16 * DS_CT * c, col, R);
    }
    row_reduce<true>(m0);
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
    float best = -INFINITY, brow = 1e9f;
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
            const float q = (!p.masks || p.masks[env * R + row]) ? gl + v : -1e8f;
            if (q > best) {  // rows ascend: the first maximum of this lane wins
                best = q;
                brow = (float)row;
            }
        }
    }
    float m[1] = {best};
    row_reduce<true>(m);
    float cc[1] = {best == m[0] ? -brow : -1e9f};
    row_reduce<true>(cc);
    const int32_t act = (int32_t)(-cc[0]);
    if (lane == 0) p.actions[env] = act;
    return act;
}

// lb_eval_steps256: k_eval_steps' arguments; one env of 64 lanes with EPL endpoints each per wave
// (eval_steps_wide of lbk8s_steps64.h).
template <int EPL, bool CHUNK>
__global__ __launch_bounds__(DS_BLOCK, 1) void k_eval_steps256(DSParams d, Params e, EvalSteps r) {
    static_assert(CHUNK || EPL == 2, "R <= LB_DS_MAX_ELEMENTS rows are E <= 128 endpoints");
    constexpr int NWB = DS_BLOCK / 64, OBF4 = steps_obs_f4(64, EPL), TS = (LB_DS_MAX_ELEMENTS + 15) / 16;
    constexpr bool VG = !CHUNK;
    static_assert(CHUNK || DSGeom<TS, 1, 2>::VG, "the forward of TS = 5 set tiles reads the VALU image");
    constexpr int IMG = VG ? (int)VG_ACTOR : (int)DS_C1L;
    __shared__ __attribute__((aligned(16))) float Wt[IMG + (VG ? NWB * VG_SCRATCH : 0)];
    __shared__ __attribute__((aligned(16))) float4 OB[NWB][OBF4];
    static_assert(sizeof(Wt) + sizeof(OB) <= STEPS64_LDS_MAX, "k_eval_steps256: the image, the scratch and one buffer per wave");
    eval_steps_wide<64, EPL, TS, CHUNK>(d, e, r, Wt, OB);
}

}  // namespace lbk
