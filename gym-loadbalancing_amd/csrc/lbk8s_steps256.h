// lbk8s_steps256.h — the one-launch greedy evaluation for envs of 65 to 256 endpoints:
// k_eval_steps256 (lb_eval_steps256), the sibling of k_eval_steps64 (lbk8s_steps64.h), which
// covers one endpoint per lane (E <= 64, R <= 65) only.
//
// One wave carries ONE env of R = 66..257 observation rows through all the steps of the launch.
// The env sits in the slice layout of its geometry below 32,768 envs: the 64 lanes of a wave with
// EPL = 2 or 4 endpoints per lane (StepsEnvW64, the EPL-general sibling of StepsGroupW<64, 1>).
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
// chunked forward reads it in every pass, StepsEnvW64::step then writes the next rows into it; a
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
constexpr int steps256_obs_f4(int EPL) { return 2 * (64 * EPL + 1); }  // float4s of an observation of R <= 64 EPL + 1 rows
static_assert(2 * STEPS256_MAX_R <= steps256_obs_f4(4), "the LDS observation image holds R <= 257 rows");

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

// StepsGroupW<64, 1> (lbk8s_steps64.h) for EPL endpoints per lane: one env on the 64 lanes of a
// wave.  Same functions, same order as lb_step and lb_ppo_record.
template <int EPL>
struct StepsEnvW64 {
    static_assert(EPL == 2 || EPL == 4, "the 64-lane slices of E = 65..256");
    static constexpr int W = 64;
    int64_t env;
    bool live, head;  // the wave holds an env; this is the lane of the env's scalars
    int lw;           // the lane
    SEnv<EPL> v;
    double esum, ecnt;  // the env's ep_sum / ep_cnt and VecMonitor's float32 running return (head)
    float ret32;
    // the last step's results
    float rw;
    double reward, ret;  // ret: the finished episode's return (its ep_stats row's first column)
    bool dn;

    __device__ __forceinline__ void open(const Params& e, const StepsRecord* rec, int64_t gi, int lane) {
        lw = lane;
        env = gi;
        live = env < e.B;
        head = live && lw == 0;
        esum = 0.0, ecnt = 0.0;
        ret32 = 0.f;
        if (live) {
            slice_load<W, EPL>(e, env, lw, v);
            slice_observe<EPL>(e, v);
        }
        if (rec && head) {
            if (rec->ep_sum) {
                esum = rec->ep_sum[env];
                ecnt = rec->ep_cnt[env];
            }
            if (rec->log) ret32 = rec->ret32[env];
        }
    }

    // lb_step with action a (k_step_slice<64, EPL>'s body, the observed values kept in registers);
    // the next observations to the LDS image nxt (slice_obs_rows' q: the float4 of the env's block)
    __device__ __forceinline__ void step(const Params& e, int a, float4* nxt) {
        rw = 0.f;
        reward = 0.0, ret = 0.0;
        dn = false;
        if (live) {
            const SPrep pr = slice_prep<W, EPL>(e, v, a);
            const double tot0 = v.total;
            reward = slice_apply<W, EPL, false, false>(e, env, lw, v, pr, dn);
            rw = (float)reward;
            ret = e.auto_reset ? tot0 + reward : 0.0;  // (slice_apply's v.total += reward)
            slice_obs_rows<W, EPL>(e, lw, v, [&](int q, float4 o) { nxt[q] = o; });
        }
    }

    // The env's registers parked in LDS over a forward that leaves none to spare (StepsGroupW's
    // park / unpark).  Words: lane lw's lat0[k] at 2 (64 k + lw); em / ed / olat / ocpu [k] at
    // (2..5) 64 EPL + 64 k + lw; from 6 x 64 EPL the env's scalars, written by the head lane and
    // read back by every lane.
    static constexpr int PARK_WORDS = 6 * W * EPL + 32;
    static_assert(PARK_WORDS <= 4 * steps256_obs_f4(EPL), "the parked env fits the observation image");
    using G1 = StepsGroupW<64, 1>;  // (its word packing)
    __device__ __forceinline__ void park(float4* img) {
        if (!live) return;
        float* w = reinterpret_cast<float*>(img);
#pragma unroll
        for (int k = 0; k < EPL; ++k) {
            G1::pk_put(w + 2 * (W * k + lw), v.lat0[k]);
            w[(2 * EPL + k) * W + lw] = __uint_as_float(v.em[k]);
            w[(3 * EPL + k) * W + lw] = __uint_as_float(v.ed[k]);
            w[(4 * EPL + k) * W + lw] = v.olat[k];
            w[(5 * EPL + k) * W + lw] = v.ocpu[k];
        }
        if (!head) return;
        float* u = w + 6 * W * EPL;
        G1::pk_put(u, v.t), G1::pk_put(u + 2, v.dt), G1::pk_put(u + 4, v.total), G1::pk_put(u + 6, v.last_r);
        G1::pk_put(u + 8, v.sum_lat), G1::pk_put(u + 10, v.sum_cpu), G1::pk_put(u + 12, v.topo), G1::pk_put(u + 14, v.zcap);
        G1::pk_put(u + 16, v.acc2), G1::pk_put(u + 18, v.acc3), G1::pk_put(u + 20, v.nz0), G1::pk_put(u + 22, v.nz1);
        G1::pk_put(u + 24, sc_pack(v.s)), G1::pk_put(u + 26, esum), G1::pk_put(u + 28, ecnt);
        u[30] = __uint_as_float(v.sum_hi);
        u[31] = ret32;
    }
    __device__ __forceinline__ void unpark(const float4* img) {
        if (!live) return;
        const float* w = reinterpret_cast<const float*>(img);
#pragma unroll
        for (int k = 0; k < EPL; ++k) {
            v.lat0[k] = G1::pk_getd(w + 2 * (W * k + lw));
            v.em[k] = __float_as_uint(w[(2 * EPL + k) * W + lw]);
            v.ed[k] = __float_as_uint(w[(3 * EPL + k) * W + lw]);
            v.olat[k] = w[(4 * EPL + k) * W + lw];
            v.ocpu[k] = w[(5 * EPL + k) * W + lw];
        }
        const float* u = w + 6 * W * EPL;
        v.t = G1::pk_getd(u), v.dt = G1::pk_getd(u + 2), v.total = G1::pk_getd(u + 4), v.last_r = G1::pk_getd(u + 6);
        v.sum_lat = G1::pk_get(u + 8), v.sum_cpu = G1::pk_get(u + 10), v.topo = G1::pk_get(u + 12), v.zcap = G1::pk_get(u + 14);
        v.acc2 = G1::pk_get(u + 16), v.acc3 = G1::pk_get(u + 18), v.nz0 = G1::pk_get(u + 20), v.nz1 = G1::pk_get(u + 22);
        v.s = sc_unpack(G1::pk_get(u + 24)), esum = G1::pk_getd(u + 26), ecnt = G1::pk_getd(u + 28);
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

    // the env's history counters (the slice layout's end-of-launch stores: k_rollout_slice's) and
    // scalars, stored after the last step
    __device__ __forceinline__ void close(const Params& e, const StepsRecord* rec) {
        if (live) {
#pragma unroll
            for (int k = 0; k < EPL; ++k) {
                const int ep = lw + k * W;
                if (ep < e.E) e.edyn[eidx(e, env, ep)] = v.ed[k];
            }
            if (lw == 0) slice_store_scalars<EPL>(e, env, v);
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

// lb_eval_steps256: k_eval_steps' arguments; one env of 64 lanes with EPL endpoints each per wave.
template <int EPL, bool CHUNK>
__global__ __launch_bounds__(DS_BLOCK, 1) void k_eval_steps256(DSParams d, Params e, EvalSteps r) {
    static_assert(CHUNK || EPL == 2, "R <= LB_DS_MAX_ELEMENTS rows are E <= 128 endpoints");
    constexpr int NWB = DS_BLOCK / 64, OBF4 = steps256_obs_f4(EPL), TS = (LB_DS_MAX_ELEMENTS + 15) / 16;
    constexpr bool VG = !CHUNK;
    static_assert(CHUNK || DSGeom<TS, 1, 2>::VG, "the forward of TS = 5 set tiles reads the VALU image");
    constexpr int IMG = VG ? (int)VG_ACTOR : (int)DS_C1L;
    __shared__ __attribute__((aligned(16))) float Wt[IMG + (VG ? NWB * VG_SCRATCH : 0)];
    __shared__ __attribute__((aligned(16))) float4 OB[NWB][OBF4];
    static_assert(sizeof(Wt) + sizeof(OB) <= STEPS64_LDS_MAX, "k_eval_steps256: the image, the scratch and one buffer per wave");
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
    const int R = d.R, f4 = 2 * R;  // (float4s per observation <= OBF4: host check)
    const int64_t B = e.B;
    float4* ob = OB[wv];
    for (int64_t env = wave; env < B; env += nwaves) {
        StepsEnvW64<EPL> g;
        g.open(e, &r.rec, env, lane);
        for (int j = lane; j < f4; j += 64) ob[j] = r.obs[env * f4 + j];
        for (int i = 0; i < r.steps; ++i) {
            const int64_t row = (int64_t)i * B;
            const int ln = steps64_lane(lane);
            g.lw = ln;
            // lb_ds_q_argmax on the LDS observation (lane 0 holds the action), then to the lanes of
            // the env's slice
            int32_t act;
            if constexpr (CHUNK) {
                act = ds_chunked_argmax_lds(d, Wt, ob, env, ln, R);
            } else {
                const int col = ln & 15, grp = ln >> 4;
                float h0[TS][2], m0[2], xr0[2];
                ds_group_obs<TS, 1, 2>(d, env, col, grp, R, h0, m0, xr0, reinterpret_cast<const float*>(ob));
                g.park(ob);
                uint32_t wo = 0;  // (the weights read from LDS in every step: k_ppo_steps64)
                asm volatile("" : "+s"(wo));
                const float* Wc = Wt + wo;
                act = ds_group_actor<TS, 1, 2, VG>(d, Wc, ln, env, col, grp, R, h0, m0, xs);
            }
            g.lw = steps64_lane(lane);
            if constexpr (!CHUNK) g.unpark(ob);
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
