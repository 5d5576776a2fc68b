// lbk8s_steps64.h — the one-launch step kernels for envs of up to 64 endpoints: k_ppo_steps64
// (lb_ppo_steps64) and k_eval_steps64 (lb_eval_steps64), the siblings of k_ppo_steps (lbk8s_ppo.h)
// and k_eval_steps (lbk8s_eval.h), which cover the 16-lane slice of R <= 16 rows only.
//
// One wave carries ONE env of R = 17..65 observation rows through all the steps of the launch.
// The env sits in the slice layout of its geometry (W = 16, 32 or 64 lanes, one endpoint per
// lane: EPL = 1, fewer than 32,768 envs) on lanes 0 .. W - 1 (StepsGroupW, the W-lane sibling of
// StepsGroup), the forward is the deep-sets forward of TS = ceil(R / 16) set tiles with one env
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
// again before StepsGroupW::step writes the next rows, which are then copied out (PPO) or read by
// the next forward (a wave's LDS operations complete in order).  In between, over the forward,
// the image holds the env's registers (StepsGroupW::park).  Bytes, 8 waves per block:
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
constexpr int steps64_obs_f4(int W) { return 2 * (W + 1); }  // float4s of an observation of R <= W + 1 rows
static_assert(2 * STEPS64_MAX_R <= steps64_obs_f4(64), "the LDS observation image holds R <= 65 rows");
constexpr int STEPS64_LDS_MAX = 160 * 1024;

// The lane index as a value the compiler cannot see through.  Taken anew before the forward and
// after it in every step, it keeps what derives from the lane (column and row group, the slice's
// addresses of the step's and the restart's stores) from being computed once before the step loop
// and held in registers across the forward, where there are none to spare.
__device__ __forceinline__ int steps64_lane(int lane) {
    asm volatile("" : "+v"(lane));
    return lane;
}

// StepsGroup (lbk8s_steps.h) for W-lane slices: a group of P envs of a wave, W P <= 64, one
// endpoint per lane (EPL = 1).  Lanes W s .. W s + W - 1 hold env env0 + s.  Same functions, same
// order per env as lb_step and lb_ppo_record.
template <int W, int P>
struct StepsGroupW {
    static_assert((W == 16 || W == 32 || W == 64) && P >= 1 && W * P <= 64, "P slices of W lanes in a wave");
    int64_t env0, env;  // the group's first env; this lane's
    bool live, head;    // the lane holds an env; it is the lane of the env's scalars
    int j1;             // the group's float4s
    int s, lw, f4;      // slice, lane in the slice, float4s per observation
    SEnv<1> v;
    double esum, ecnt;  // the env's ep_sum / ep_cnt and VecMonitor's float32 running return (head)
    float ret32;
    // the last step's results
    float rw;
    double reward, ret;  // ret: the finished episode's return (its ep_stats row's first column)
    bool dn;

    __device__ __forceinline__ void open(const Params& e, const StepsRecord* rec, int64_t gi, int lane, int f4_) {
        s = lane / W, lw = lane % W, f4 = f4_;
        env0 = gi * P;
        env = env0 + s;
        live = s < P && env < e.B;
        head = live && lw == 0;
        j1 = (int)((env0 + P < e.B ? env0 + P : e.B) - env0) * f4;
        esum = 0.0, ecnt = 0.0;
        ret32 = 0.f;
        if (live) {
            slice_load<W, 1>(e, env, lw, v);
            slice_observe<1>(e, v);
        }
        if (rec && head) {
            if (rec->ep_sum) {
                esum = rec->ep_sum[env];
                ecnt = rec->ep_cnt[env];
            }
            if (rec->log) ret32 = rec->ret32[env];
        }
    }

    // lb_step with action a (k_step_slice<W, 1>'s body, the observed values kept in registers);
    // the next observations to the LDS image nxt
    __device__ __forceinline__ void step(const Params& e, int a, float4* nxt) {
        rw = 0.f;
        reward = 0.0, ret = 0.0;
        dn = false;
        if (live) {
            const SPrep pr = slice_prep<W, 1>(e, v, a);
            const double tot0 = v.total;
            reward = slice_apply<W, 1, false, false>(e, env, lw, v, pr, dn);
            rw = (float)reward;
            ret = e.auto_reset ? tot0 + reward : 0.0;  // (slice_apply's v.total += reward)
            slice_obs_rows<W, 1>(e, lw, v, [&](int q, float4 o) { nxt[s * f4 + q] = o; });
        }
    }

    // The env's registers parked in the wave's LDS observation image over the forward (P = 1: the
    // whole image is the env's), and taken back before step().  The image is free then (the
    // forward holds the observation in its fragments), and the forward of TS = 5 set tiles takes
    // 210 to 226 of the lane's 256 registers on its own: with the env held next to it the kernels
    // spilled to scratch.  Words (all moved as float, the image's element type): lane lw's lat0
    // at 2 lw, em / ed / olat / ocpu at (2..5) W + lw; from 6 W the env's scalars, written by
    // the head lane and read back by every lane of the slice.
    static constexpr int PARK_WORDS = 6 * W + 32;
    static_assert(PARK_WORDS <= 4 * steps64_obs_f4(W), "the parked env fits the observation image");
    static __device__ __forceinline__ void pk_put(float* w, uint64_t x) {
        w[0] = __uint_as_float((uint32_t)x);
        w[1] = __uint_as_float((uint32_t)(x >> 32));
    }
    static __device__ __forceinline__ uint64_t pk_get(const float* w) {
        return (uint64_t)__float_as_uint(w[0]) | ((uint64_t)__float_as_uint(w[1]) << 32);
    }
    static __device__ __forceinline__ void pk_put(float* w, double x) { pk_put(w, (uint64_t)__double_as_longlong(x)); }
    static __device__ __forceinline__ double pk_getd(const float* w) { return __longlong_as_double((long long)pk_get(w)); }
    __device__ __forceinline__ void park(float4* img) {
        static_assert(P == 1, "one env per wave: the image is its own");
        if (!live) return;
        float* w = reinterpret_cast<float*>(img);
        pk_put(w + 2 * lw, v.lat0[0]);
        w[2 * W + lw] = __uint_as_float(v.em[0]);
        w[3 * W + lw] = __uint_as_float(v.ed[0]);
        w[4 * W + lw] = v.olat[0];
        w[5 * W + lw] = v.ocpu[0];
        if (!head) return;
        float* u = w + 6 * W;
        pk_put(u, v.t), pk_put(u + 2, v.dt), pk_put(u + 4, v.total), pk_put(u + 6, v.last_r);
        pk_put(u + 8, v.sum_lat), pk_put(u + 10, v.sum_cpu), pk_put(u + 12, v.topo), pk_put(u + 14, v.zcap);
        pk_put(u + 16, v.acc2), pk_put(u + 18, v.acc3), pk_put(u + 20, v.nz0), pk_put(u + 22, v.nz1);
        pk_put(u + 24, sc_pack(v.s)), pk_put(u + 26, esum), pk_put(u + 28, ecnt);
        u[30] = __uint_as_float(v.sum_hi);
        u[31] = ret32;
    }
    __device__ __forceinline__ void unpark(const float4* img) {
        if (!live) return;
        const float* w = reinterpret_cast<const float*>(img);
        v.lat0[0] = pk_getd(w + 2 * lw);
        v.em[0] = __float_as_uint(w[2 * W + lw]);
        v.ed[0] = __float_as_uint(w[3 * W + lw]);
        v.olat[0] = w[4 * W + lw];
        v.ocpu[0] = w[5 * W + lw];
        const float* u = w + 6 * W;
        v.t = pk_getd(u), v.dt = pk_getd(u + 2), v.total = pk_getd(u + 4), v.last_r = pk_getd(u + 6);
        v.sum_lat = pk_get(u + 8), v.sum_cpu = pk_get(u + 10), v.topo = pk_get(u + 12), v.zcap = pk_get(u + 14);
        v.acc2 = pk_get(u + 16), v.acc3 = pk_get(u + 18), v.nz0 = pk_get(u + 20), v.nz1 = pk_get(u + 22);
        v.s = sc_unpack(pk_get(u + 24)), esum = pk_getd(u + 26), ecnt = pk_getd(u + 28);
        v.sum_hi = __float_as_uint(u[30]);
        ret32 = u[31];
    }

    // lb_ppo_record of step i (StepsGroup::record)
    __device__ __forceinline__ void record(const Params& e, const StepsRecord rec, int a, int i) {
        float r32 = 0.f;
        if (head) {
            if (rec.ep_sum && dn) {
                esum += e.auto_reset ? ret : e.ep_stats[env * LB_ST_K + LB_ST_RETURN];
                ecnt += 1.0;
            }
            if (rec.log) {
                r32 = (float)((double)ret32 + reward);
                ret32 = dn ? 0.f : r32;
                if (dn && rec.ep_r32) rec.ep_r32[env] = r32;
            }
        }
        if (rec.log)  // (wave-uniform: every lane takes part in the ballot; a done head wrote the stats row)
            eplog_append(head && dn, env, e.ep_stats, r32, rec.tag0 + i, rec.log, rec.cap, rec.count,
                         [&] { return EpLogStep{rw, a}; });
    }

    // the env's history counters and scalars, stored after the last step
    __device__ __forceinline__ void close(const Params& e, const StepsRecord* rec) {
        if (live) {
            if (lw < e.E) e.edyn[eidx(e, env, lw)] = v.ed[0];
            if (lw == 0) slice_store_scalars<1>(e, env, v);
        }
        if (rec && head) {
            if (rec->ep_sum) {
                rec->ep_sum[env] = esum;
                rec->ep_cnt[env] = ecnt;
            }
            if (rec->log) rec->ret32[env] = ret32;
        }
    }
};

// lb_ppo_steps64: k_ppo_steps' arguments; one env of W lanes and TS set tiles per wave.
template <int W, int TS>
__global__ __launch_bounds__(DS_BLOCK, 1) void k_ppo_steps64(DSParams d, Params e, PPOSteps r) {
    static_assert(TS >= 2 && TS <= 5 && 16 * (TS - 1) < W + 1, "some R <= W + 1 takes TS set tiles");
    constexpr int NWB = DS_BLOCK / 64, OBF4 = steps64_obs_f4(W);
    constexpr bool VG = DSGeom<TS, 1, LB_DS_FWD_SAMPLE>::VG;
    constexpr int IMG = VG ? (int)VG_RHO : (int)DS_FLOATS;
    __shared__ __attribute__((aligned(16))) float Wt[IMG + (VG ? NWB * VG_SCRATCH : 0)];
    __shared__ __attribute__((aligned(16))) float4 OB[NWB][OBF4];
    static_assert(sizeof(Wt) + sizeof(OB) <= STEPS64_LDS_MAX, "k_ppo_steps64: the image, the scratch and one buffer per wave");
    const float* src = d.wfrag + (VG ? DS_FLOATS : 0);
    for (int i = threadIdx.x * 4; i < IMG; i += DS_BLOCK * 4)
        *reinterpret_cast<float4*>(Wt + i) = *reinterpret_cast<const float4*>(src + i);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* xs = VG ? Wt + IMG + wv * VG_SCRATCH : nullptr;
    // wave-major numbering, as k_deepsets_fwd: fewer envs than waves put one wave per SIMD
    const int64_t wave = (int64_t)wv * gridDim.x + blockIdx.x;
    const int64_t nwaves = (int64_t)gridDim.x * NWB;
    const int R = d.R;
    const int64_t B = e.B;
    float4* ob = OB[wv];
    for (int64_t gi = wave; gi < B; gi += nwaves) {
        StepsGroupW<W, 1> g;
        g.open(e, &r.rec, gi, lane, 2 * R);  // (float4s per observation <= OBF4: host check)
        const int64_t env = g.env0;
        const int f4 = g.f4;
        for (int j = lane; j < f4; j += 64) ob[j] = reinterpret_cast<const float4*>(r.obs)[env * f4 + j];
        for (int i = 0; i < r.steps; ++i) {
            const int64_t row = (int64_t)i * B;
            const bool stored = i < r.store_rows;
            const int ln = steps64_lane(lane), col = ln & 15, grp = ln >> 4;
            g.lw = ln % W;
            // lb_ds_sample on the LDS observation (into the fragments h0: the image is free after it)
            DSParams ds = d;
            ds.uniforms = r.uniforms + row;
            ds.actions_f32 = r.actions_f32 + row;
            ds.logprob = r.logprobs + row;
            ds.value = r.values + row;
            float h0[TS][2], m0[2], xr0[2];
            ds_group_obs<TS, 1, LB_DS_FWD_SAMPLE>(ds, env, col, grp, R, h0, m0, xr0, reinterpret_cast<const float*>(ob));
            g.park(ob);
            // (an opaque offset per step, as k_deepsets_fwd_big's per chunk: the weights are read from
            // LDS in every step, not hoisted out of the loop into registers that then spill)
            uint32_t wo = 0;
            asm volatile("" : "+s"(wo));
            const float* Wc = Wt + wo;
            const int32_t act = ds_group_actor<TS, 1, LB_DS_FWD_SAMPLE, VG>(ds, Wc, ln, env, col, grp, R, h0, m0, xs);
            ds_group_critic<TS, 1, LB_DS_FWD_SAMPLE, VG>(ds, Wc, ln, env, col, grp, R, h0, m0, xs);
            const int lp = steps64_lane(lane);
            g.lw = lp % W;
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

// lb_eval_steps64: k_eval_steps' arguments; one env of W lanes and TS set tiles per wave.  The
// greedy forward reads the actor part of its image only.
template <int W, int TS>
__global__ __launch_bounds__(DS_BLOCK, 1) void k_eval_steps64(DSParams d, Params e, EvalSteps r) {
    static_assert(TS >= 2 && TS <= 5 && 16 * (TS - 1) < W + 1, "some R <= W + 1 takes TS set tiles");
    constexpr int NWB = DS_BLOCK / 64, OBF4 = steps64_obs_f4(W);
    constexpr bool VG = DSGeom<TS, 1, 2>::VG;
    constexpr int IMG = VG ? (int)VG_ACTOR : (int)DS_C1L;
    __shared__ __attribute__((aligned(16))) float Wt[IMG + (VG ? NWB * VG_SCRATCH : 0)];
    __shared__ __attribute__((aligned(16))) float4 OB[NWB][OBF4];
    static_assert(sizeof(Wt) + sizeof(OB) <= STEPS64_LDS_MAX, "k_eval_steps64: the image, the scratch and one buffer per wave");
    const float* src = d.wfrag + (VG ? DS_FLOATS : 0);
    for (int i = threadIdx.x * 4; i < IMG; i += DS_BLOCK * 4)
        *reinterpret_cast<float4*>(Wt + i) = *reinterpret_cast<const float4*>(src + i);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* xs = VG ? Wt + IMG + wv * VG_SCRATCH : nullptr;
    // wave-major numbering, as k_deepsets_fwd: fewer envs than waves put one wave per SIMD
    const int64_t wave = (int64_t)wv * gridDim.x + blockIdx.x;
    const int64_t nwaves = (int64_t)gridDim.x * NWB;
    const int R = d.R;
    const int64_t B = e.B;
    float4* ob = OB[wv];
    for (int64_t gi = wave; gi < B; gi += nwaves) {
        StepsGroupW<W, 1> g;
        g.open(e, &r.rec, gi, lane, 2 * R);  // (float4s per observation <= OBF4: host check)
        const int64_t env = g.env0;
        const int f4 = g.f4;
        for (int j = lane; j < f4; j += 64) ob[j] = r.obs[env * f4 + j];
        for (int i = 0; i < r.steps; ++i) {
            const int64_t row = (int64_t)i * B;
            const int ln = steps64_lane(lane), col = ln & 15, grp = ln >> 4;
            g.lw = ln % W;
            // lb_ds_q_argmax on the LDS observation (lane 0 holds the action), then to the lanes of
            // the env's slice
            float h0[TS][2], m0[2], xr0[2];
            ds_group_obs<TS, 1, 2>(d, env, col, grp, R, h0, m0, xr0, reinterpret_cast<const float*>(ob));
            g.park(ob);
            uint32_t wo = 0;  // (the weights read from LDS in every step: k_ppo_steps64)
            asm volatile("" : "+s"(wo));
            const float* Wc = Wt + wo;
            const int32_t act = ds_group_actor<TS, 1, 2, VG>(d, Wc, ln, env, col, grp, R, h0, m0, xs);
            g.lw = steps64_lane(lane) % W;
            g.unpark(ob);
            const int32_t a = __shfl(act, 0);
            g.step(e, a, ob);
            // the step's trace row, then lb_ppo_record's sums and log
            if (g.head) {
                if (r.actions_all) r.actions_all[row + env] = a;
                if (r.rewards_all) r.rewards_all[row + env] = g.rw;
                if (r.dones_all) r.dones_all[row + env] = (uint8_t)g.dn;
                if (i == r.steps - 1) {  // what the last lb_step leaves
                    e.reward[env] = g.rw;
                    e.rew64[env] = g.reward;
                    e.done[env] = (uint8_t)g.dn;
                }
            }
            g.record(e, r.rec, a, i);
        }
        // obs <- the observations after the last step, from LDS, then the env
        for (int j = lane; j < f4; j += 64) r.obs[env * f4 + j] = ob[j];
        g.close(e, &r.rec);
    }
}

}  // namespace lbk
