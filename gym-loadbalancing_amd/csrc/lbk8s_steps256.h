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
//   yes    81..257    2, 4  ds_chunked_set<2, DSRowsLds> (lbk8s_ds_chunked.h), the function that
//                           k_deepsets_fwd_big<2> runs per set (the max pass over obs, three passes
//                           over the 32-row chunks, first maximum wins, masked rows at -1e8), on the
//                           actor fragments in LDS (both weight pointers: no critic runs), the set's
//                           rows read from the wave's LDS observation image (ds_reads)
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
