// lbk8s_steps64.h — the one-launch step kernels for envs of up to 64 endpoints: k_ppo_steps64
// (lb_ppo_steps64) and k_eval_steps64 (lb_eval_steps64), the siblings of k_ppo_steps (lbk8s_ppo.h)
// and k_eval_steps (lbk8s_eval.h), which cover the 16-lane slice of R <= 16 rows only.
//
// One wave carries ONE env of R = 17..65 observation rows through all the steps of the launch.
// The env sits in the slice layout of its geometry (W = 16, 32 or 64 lanes, one endpoint per
// lane: EPL = 1, fewer than 32,768 envs) on lanes 0 .. W - 1 (StepsEnv<W, 1, 1> of
// lbk8s_steps.h), the forward is the deep-sets forward of TS = ceil(R / 16) set tiles with one env
// per wave iteration:
//
//   W   E        R        TS
//   16  16       17       2         (the reject row is the one live row of tile 2)
//   32  17..32   17..33   2, 3 at R = 33
//   64  33..64   33..65   3, 4, 5
//
// At TS = 2 the forward reads the MFMA fragment image, at TS >= 3 the VALU image with the wave's
// scratch (DSGeom<TS, 1, MODE>::VG) -- the images and the arithmetic of lb_ds_sample /
// lb_ds_q_argmax at that R, per set column, so the bits are theirs whichever P they take.
//
// LDS.  The observation image is ONE buffer of 2 (W + 1) float4s per wave: ds_group_obs moves the
// observation into the layer-1 fragments before anything else runs and nothing reads the image
// again before StepsEnv::step writes the next rows, which are then copied out (PPO) or read by
// the next forward (a wave's LDS operations complete in order).  In between, over the forward,
// the image holds the env's registers (StepsEnv::park).  Bytes, 8 waves per block:
//   k_ppo_steps64   TS = 2: DS_FLOATS image 135,440 + 8 x 66 x 16 = 143,888 (W = 32)
//                   TS >= 3: VG_RHO image 131,088 + scratch 8 x 128 x 4 = 4,096 + 8 x 130 x 16 =
//                   16,640: 151,824 (W = 64; two buffers would be 168,464, over the CU's 163,840)
//   k_eval_steps64  TS = 2: actor fragments 45,056 + 8,448 = 53,504; TS >= 3: VG_ACTOR 39,424 +
//                   4,096 + 16,640 = 60,160
// One block per CU (the grid is ds_grid_spread's: at most one block per CU), so a lane has 256
// registers: __launch_bounds__(DS_BLOCK, 1).
#pragma once

#include "lbk8s_deepsets.h"
#include "lbk8s_eval.h"
#include "lbk8s_ppo.h"
#include "lbk8s_slice.h"
#include "lbk8s_steps.h"

namespace lbk {

constexpr int STEPS64_MAX_R = 65;
static_assert(2 * STEPS64_MAX_R <= steps_obs_f4(64, 1), "the LDS observation image holds R <= 65 rows");
constexpr int STEPS64_LDS_MAX = 160 * 1024;

// The lane index as a value the compiler cannot see through.  Taken anew before the forward and
// after it in every step, it keeps what derives from the lane (column and row group, the slice's
// addresses of the step's and the restart's stores) from being computed once before the step loop
// and held in registers across the forward, where there are none to spare.
__device__ __forceinline__ int steps64_lane(int lane) {
    asm volatile("" : "+v"(lane));
    return lane;
}

// The block's weight image staged into LDS once (every thread of the block calls it)
template <int IMG>
__device__ __forceinline__ void steps_stage_weights(float* Wt, const float* src) {
    for (int i = threadIdx.x * 4; i < IMG; i += DS_BLOCK * 4)
        *reinterpret_cast<float4*>(Wt + i) = *reinterpret_cast<const float4*>(src + i);
    __syncthreads();
}

// A wave of a wide step kernel, one env at a time: its scratch behind the weight image Wt of IMG
// floats (VG: the VALU image's forward has one) and the wave-major numbering of k_deepsets_fwd
// (fewer envs than waves put one wave per SIMD)
struct StepsWave {
    int lane, wv;
    float* xs;
    int64_t wave, nwaves;
};
template <bool VG, int IMG>
__device__ __forceinline__ StepsWave steps_wave(float* Wt) {
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* xs = VG ? Wt + IMG + wv * VG_SCRATCH : nullptr;
    const int64_t wave = (int64_t)wv * gridDim.x + blockIdx.x;
    const int64_t nwaves = (int64_t)gridDim.x * (DS_BLOCK / 64);
    return {lane, wv, xs, wave, nwaves};
}

// lb_ds_q_argmax of env's observation in the LDS image cur, to every lane of the wave: the forward
// of TS set tiles (MODE 2, the actor part of the image Wt), the env g parked in the image pk over
// it (cur itself, or a second buffer where cur is still needed: k_dqn_steps64).  Lane 0 writes
// d.actions[env], as the forward does.
template <int TS, bool VG, typename G>
__device__ __forceinline__ int32_t steps_greedy_action(const DSParams& d, G& g, const float* Wt, float* xs, int lane,
                                                       int64_t env, int R, const float4* cur, float4* pk) {
    const int ln = steps64_lane(lane), col = ln & 15, grp = ln >> 4;
    g.relane(ln);
    float h0[TS][2], m0[2], xr0[2];
    ds_group_obs<TS, 1, 2>(d, env, col, grp, R, h0, m0, xr0, reinterpret_cast<const float*>(cur));
    g.park(pk);
    // (an opaque offset per step, as k_deepsets_fwd_big's per chunk: the weights are read from LDS
    // in every step, not hoisted out of the loop into registers that then spill)
    uint32_t wo = 0;
    asm volatile("" : "+s"(wo));
    const float* Wc = Wt + wo;
    const int32_t act = ds_group_actor<TS, 1, 2, VG>(d, Wc, ln, env, col, grp, R, h0, m0, xs);
    g.relane(steps64_lane(lane));
    g.unpark(pk);
    return __shfl(act, 0);  // (lane 0 holds it)
}

// lb_ppo_steps64: k_ppo_steps' arguments; one env of W lanes and TS set tiles per wave.
template <int W, int TS>
__global__ __launch_bounds__(DS_BLOCK, 1) void k_ppo_steps64(DSParams d, Params e, PPOSteps r) {
    static_assert(TS >= 2 && TS <= 5 && 16 * (TS - 1) < W + 1, "some R <= W + 1 takes TS set tiles");
    constexpr int NWB = DS_BLOCK / 64, OBF4 = steps_obs_f4(W, 1);
    constexpr bool VG = DSGeom<TS, 1, LB_DS_FWD_SAMPLE>::VG;
    constexpr int IMG = VG ? (int)VG_RHO : (int)DS_FLOATS;
    __shared__ __attribute__((aligned(16))) float Wt[IMG + (VG ? NWB * VG_SCRATCH : 0)];
    __shared__ __attribute__((aligned(16))) float4 OB[NWB][OBF4];
    static_assert(sizeof(Wt) + sizeof(OB) <= STEPS64_LDS_MAX, "k_ppo_steps64: the image, the scratch and one buffer per wave");
    steps_stage_weights<IMG>(Wt, d.wfrag + (VG ? DS_FLOATS : 0));
    const StepsWave w = steps_wave<VG, IMG>(Wt);
    const int lane = w.lane;
    float* xs = w.xs;
    const int R = d.R;
    const int64_t B = e.B;
    float4* ob = OB[w.wv];
    for (int64_t gi = w.wave; gi < B; gi += w.nwaves) {
        StepsEnv<W, 1, 1> g;
        g.open(e, &r.rec, gi, lane, 2 * R);  // (float4s per observation <= OBF4: host check)
        const int64_t env = g.env0;
        const int f4 = g.f4;
        for (int j = lane; j < f4; j += 64) ob[j] = reinterpret_cast<const float4*>(r.obs)[env * f4 + j];
        for (int i = 0; i < r.steps; ++i) {
            const int64_t row = (int64_t)i * B;
            const bool stored = i < r.store_rows;
            const int ln = steps64_lane(lane), col = ln & 15, grp = ln >> 4;
            g.relane(ln);
            // lb_ds_sample on the LDS observation (into the fragments h0: the image is free after it),
            // the env parked over the forward as in steps_greedy_action
            DSParams ds = d;
            ds.uniforms = r.uniforms + row;
            ds.actions_f32 = r.actions_f32 + row;
            ds.logprob = r.logprobs + row;
            ds.value = r.values + row;
            float h0[TS][2], m0[2], xr0[2];
            ds_group_obs<TS, 1, LB_DS_FWD_SAMPLE>(ds, env, col, grp, R, h0, m0, xr0, reinterpret_cast<const float*>(ob));
            g.park(ob);
            uint32_t wo = 0;
            asm volatile("" : "+s"(wo));
            const float* Wc = Wt + wo;
            const int32_t act = ds_group_actor<TS, 1, LB_DS_FWD_SAMPLE, VG>(ds, Wc, ln, env, col, grp, R, h0, m0, xs);
            ds_group_critic<TS, 1, LB_DS_FWD_SAMPLE, VG>(ds, Wc, ln, env, col, grp, R, h0, m0, xs);
            const int lp = steps64_lane(lane);
            g.relane(lp);
            g.unpark(ob);
            const int32_t a = __shfl(act, 0);  // (row group 0 holds it) to the lanes of the env's slice
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

// The body of k_eval_steps64<W, TS> (EPL = 1, CHUNK = false) and of k_eval_steps256<EPL, CHUNK>
// (W = 64): k_eval_steps' arguments; one env of W lanes with EPL endpoints each per wave.  Wt: the
// actor part of the forward's image (and the waves' scratch), OB: one observation buffer per wave.
// CHUNK: the chunked forward reads the observation from the image in every pass, and the env
// stays in registers next to it.
template <int W, int EPL, int TS, bool CHUNK>
__device__ __forceinline__ void eval_steps_wide(const DSParams& d, const Params& e, const EvalSteps& r, float* Wt,
                                                float4 (*OB)[steps_obs_f4(W, EPL)]) {
    constexpr bool VG = !CHUNK && DSGeom<TS, 1, 2>::VG;
    constexpr int IMG = VG ? (int)VG_ACTOR : (int)DS_C1L;
    steps_stage_weights<IMG>(Wt, d.wfrag + (VG ? DS_FLOATS : 0));
    const StepsWave w = steps_wave<VG, IMG>(Wt);
    const int lane = w.lane;
    float* xs = w.xs;
    const int R = d.R;
    const int64_t B = e.B;
    float4* ob = OB[w.wv];
    for (int64_t gi = w.wave; gi < B; gi += w.nwaves) {
        StepsEnv<W, EPL, 1> g;
        g.open(e, &r.rec, gi, lane, 2 * R);  // (float4s per observation <= steps_obs_f4: host check)
        const int64_t env = g.env0;
        const int f4 = g.f4;
        for (int j = lane; j < f4; j += 64) ob[j] = r.obs[env * f4 + j];
        for (int i = 0; i < r.steps; ++i) {
            const int64_t row = (int64_t)i * B;
            // lb_ds_q_argmax on the LDS observation, to the lanes of the env's slice
            int32_t a;
            if constexpr (CHUNK) {
                const int ln = steps64_lane(lane);
                g.relane(ln);
                const int32_t act = ds_chunked_set<2>(d, Wt, Wt, DSRowsLds{ob}, env, ln, R);
                g.relane(steps64_lane(lane));
                a = __shfl(act, 0);
            } else {
                a = steps_greedy_action<TS, VG>(d, g, Wt, xs, lane, env, R, ob, ob);
            }
            g.step(e, a, ob);
            // the step's trace row, then lb_ppo_record's sums and log
            eval_trace_row(e, r, g, row, env, a, i);
            g.record(e, r.rec, a, i);
        }
        // obs <- the observations after the last step, from LDS, then the env
        for (int j = lane; j < f4; j += 64) r.obs[env * f4 + j] = ob[j];
        g.close(e, &r.rec);
    }
}

// lb_eval_steps64: one env of W lanes and TS set tiles per wave.  The greedy forward reads the
// actor part of its image only.
template <int W, int TS>
__global__ __launch_bounds__(DS_BLOCK, 1) void k_eval_steps64(DSParams d, Params e, EvalSteps r) {
    static_assert(TS >= 2 && TS <= 5 && 16 * (TS - 1) < W + 1, "some R <= W + 1 takes TS set tiles");
    constexpr int NWB = DS_BLOCK / 64, OBF4 = steps_obs_f4(W, 1);
    constexpr bool VG = DSGeom<TS, 1, 2>::VG;
    constexpr int IMG = VG ? (int)VG_ACTOR : (int)DS_C1L;
    __shared__ __attribute__((aligned(16))) float Wt[IMG + (VG ? NWB * VG_SCRATCH : 0)];
    __shared__ __attribute__((aligned(16))) float4 OB[NWB][OBF4];
    static_assert(sizeof(Wt) + sizeof(OB) <= STEPS64_LDS_MAX, "k_eval_steps64: the image, the scratch and one buffer per wave");
    eval_steps_wide<W, 1, TS, false>(d, e, r, Wt, OB);
}

}  // namespace lbk
