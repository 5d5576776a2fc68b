// lbk8s_steps.h — what every one-launch step kernel shares: k_dqn_step (lbk8s_dqn.h), k_ppo_steps
// (lbk8s_ppo.h) and k_eval_steps (lbk8s_eval.h) at W = 16, their siblings for up to 64 endpoints
// (lbk8s_steps64.h, lbk8s_dqn64.h) and k_eval_steps256 (lbk8s_steps256.h).
//
// In each of them one wave carries a group of P envs through all the steps of the launch: lanes
// W s .. W s + W - 1 hold env env0 + s in registers (the slice layout below 32,768 envs: W lanes
// with EPL endpoints each), the group's observations live in an LDS image that the forward reads
// and the stored rows are copied from, and the env's history counters and scalars go back to
// memory once, after the last step.  StepsEnv<W, EPL, P> is that skeleton -- open, step, record,
// close, and park / unpark for the forwards that leave the env no registers -- and a kernel adds
// what is its own: the forward that chooses the action and the rows a step leaves in global
// memory.  Same functions, same order per env as lb_step and lb_ppo_record: bit for bit the
// separate launches.
//
// The episode log's row and VecMonitor's float32 return are written here and nowhere else
// (eplog_append is lb_episode_log's append too).
#pragma once

#include "lbk8s_common.h"
#include "lbk8s_slice.h"

namespace lbk {

// float4s of the LDS image of an observation of R <= W EPL + 1 rows (34 at W = 16, EPL = 1)
constexpr int steps_obs_f4(int W, int EPL) { return 2 * (W * EPL + 1); }
static_assert(2 * 16 <= steps_obs_f4(16, 1), "the LDS observation image holds R <= 16 rows (dqn_step_fusable)");

// lb_ppo_record's buffers: the finished episodes' per-env sums and the episode log
struct StepsRecord {
    double* ep_sum;  // [B] or NULL (then ep_cnt too)
    double* ep_cnt;
    // the episode log (log == NULL: none, and ret32 / ep_r32 are not touched)
    float* ret32;
    float* ep_r32;
    int64_t tag0;  // step i of the launch logs tag0 + i
    double* log;
    int64_t cap;
    uint32_t* count;
};

struct EpLogStep {  // the reward and action words of a log row
    float reward;
    int32_t action;
};

// Appends the rows of the wave's finished episodes to the device log: one atomic per wave (the
// ballot's count), rows past cap dropped (count still advances: the host sees the overflow).
// Every lane of the wave calls it, done or not; step() is evaluated by the lanes that write a row.
template <typename Step>
__device__ __forceinline__ void eplog_append(bool done, int64_t env, const double* ep_stats, float r32, int64_t tag,
                                             double* log, int64_t cap, uint32_t* count, Step&& step) {
    const int lane = threadIdx.x & 63;
    const uint64_t m = __ballot(done);
    if (!m) return;
    const int first = __ffsll((unsigned long long)m) - 1;
    uint32_t base = 0;
    if (lane == first) base = atomicAdd(count, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, first);
    const int64_t slot = (int64_t)base + __popcll(m & ((1ull << lane) - 1));
    if (!done || slot >= cap) return;
    double* row = log + slot * LB_EPLOG_W;
    const double* st = ep_stats + env * LB_ST_K;
#pragma unroll
    for (int k = 0; k < LB_ST_K; ++k) row[k] = st[k];
    const EpLogStep w = step();
    row[LB_EPLOG_RET32] = (double)r32;
    row[LB_EPLOG_REWARD] = (double)w.reward;
    row[LB_EPLOG_ACTION] = (double)w.action;
    row[LB_EPLOG_ENV] = (double)env;
    row[LB_EPLOG_TAG] = (double)tag;
}

// The env's registers as words of an LDS image (StepsEnv::park), all moved as float, the image's
// element type
__device__ __forceinline__ void pk_put(float* w, uint64_t x) {
    w[0] = __uint_as_float((uint32_t)x);
    w[1] = __uint_as_float((uint32_t)(x >> 32));
}
__device__ __forceinline__ uint64_t pk_get(const float* w) {
    return (uint64_t)__float_as_uint(w[0]) | ((uint64_t)__float_as_uint(w[1]) << 32);
}
__device__ __forceinline__ void pk_put(float* w, double x) { pk_put(w, (uint64_t)__double_as_longlong(x)); }
__device__ __forceinline__ double pk_getd(const float* w) { return __longlong_as_double((long long)pk_get(w)); }

// One group of P envs of a wave across the launch's steps, in the slice layout of W lanes with EPL
// endpoints each: lanes W s .. W s + W - 1 hold env env0 + s.  rec == NULL (k_dqn_step, whose sums
// stay in memory): no record registers.
template <int W, int EPL, int P>
struct StepsEnv {
    static_assert(W == 16 || W == 32 || W == 64, "the slice layout's widths");
    static_assert(EPL == 1 || EPL == 2 || EPL == 4, "endpoints per lane");
    static_assert(P >= 1 && W * P <= 64, "P slices of W lanes in a wave");
    static_assert(EPL == 1 || (W == 64 && P == 1), "more than one endpoint per lane: the 64-lane slices of E = 65..256");
    int64_t env0, env;  // the group's first env; this lane's
    bool live, head;    // the lane holds an env; it is the lane of the env's scalars
    int j1;             // the group's float4s
    int s, lw, f4;      // slice, lane in the slice, float4s per observation
    SEnv<EPL> v;
    double esum, ecnt;  // the env's ep_sum / ep_cnt and VecMonitor's float32 running return (head)
    float ret32;
    // the last step's results
    float rw;
    double reward, ret;  // ret: the finished episode's return (its ep_stats row's first column)
    bool dn;

    // the env loaded and observed once, as k_rollout_slice
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

    // lw from a lane index taken anew inside the step loop (steps64_lane of lbk8s_steps64.h)
    __device__ __forceinline__ void relane(int ln) { lw = ln % W; }

    // lb_step with action a: lanes W s .. W s + W - 1 step env env0 + s (k_step_slice<W, EPL>'s
    // body, the observed values kept in registers: a step changes the selected endpoint's); the next
    // observations to the LDS buffer nxt (slice_obs_rows' q: the float4 of the env's block)
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
            slice_obs_rows<W, EPL>(e, lw, v, [&](int q, float4 o) { nxt[s * f4 + q] = o; });
        }
    }

    // lb_ppo_record of step i: the finished episode's sums, VecMonitor's float32 episode_returns +=
    // the env's float64 reward (one rounding), the log row.  rec by value: its fields are then the
    // kernel's own arguments inside the step loop, and the kernels compile to what they were with
    // this code written out in each (through a pointer k_eval_steps measured 1.5 % slower)
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

    // The env's registers parked in the wave's LDS observation image over a forward that leaves
    // none to spare (P = 1: the whole image is the env's), and taken back before step().  The image
    // is free then (the forward holds the observation in its fragments), and the forward of TS = 5
    // set tiles takes 210 to 226 of the lane's 256 registers on its own: with the env held next to
    // it the kernels spilled to scratch.  Words: lane lw's lat0[k] at 2 (W k + lw); em / ed / olat /
    // ocpu [k] at ((2..5) EPL + k) W + lw; from 6 W EPL the env's scalars, written by the head
    // lane and read back by every lane of the slice.
    static constexpr int PARK_WORDS = 6 * W * EPL + 32;
    static_assert(PARK_WORDS <= 4 * steps_obs_f4(W, EPL), "the parked env fits the observation image");
    __device__ __forceinline__ void park(float4* img) {
        static_assert(P == 1, "one env per wave: the image is its own");
        if (!live) return;
        float* w = reinterpret_cast<float*>(img);
#pragma unroll
        for (int k = 0; k < EPL; ++k) {
            pk_put(w + 2 * (W * k + lw), v.lat0[k]);
            w[(2 * EPL + k) * W + lw] = __uint_as_float(v.em[k]);
            w[(3 * EPL + k) * W + lw] = __uint_as_float(v.ed[k]);
            w[(4 * EPL + k) * W + lw] = v.olat[k];
            w[(5 * EPL + k) * W + lw] = v.ocpu[k];
        }
        if (!head) return;
        float* u = w + 6 * W * EPL;
        pk_put(u, v.t), pk_put(u + 2, v.dt), pk_put(u + 4, v.total), pk_put(u + 6, v.last_r);
        pk_put(u + 8, v.sum_lat), pk_put(u + 10, v.sum_cpu), pk_put(u + 12, v.topo), pk_put(u + 14, v.zcap);
        pk_put(u + 16, v.acc2), pk_put(u + 18, v.acc3), pk_put(u + 20, v.nz0), pk_put(u + 22, v.nz1);
        pk_put(u + 24, sc_pack(v.s)), pk_put(u + 26, esum), pk_put(u + 28, ecnt);
        u[30] = __uint_as_float(v.sum_hi);
        u[31] = ret32;
    }
    __device__ __forceinline__ void unpark(const float4* img) {
        static_assert(P == 1, "one env per wave: the image is its own");
        if (!live) return;
        const float* w = reinterpret_cast<const float*>(img);
#pragma unroll
        for (int k = 0; k < EPL; ++k) {
            v.lat0[k] = pk_getd(w + 2 * (W * k + lw));
            v.em[k] = __float_as_uint(w[(2 * EPL + k) * W + lw]);
            v.ed[k] = __float_as_uint(w[(3 * EPL + k) * W + lw]);
            v.olat[k] = w[(4 * EPL + k) * W + lw];
            v.ocpu[k] = w[(5 * EPL + k) * W + lw];
        }
        const float* u = w + 6 * W * EPL;
        v.t = pk_getd(u), v.dt = pk_getd(u + 2), v.total = pk_getd(u + 4), v.last_r = pk_getd(u + 6);
        v.sum_lat = pk_get(u + 8), v.sum_cpu = pk_get(u + 10), v.topo = pk_get(u + 12), v.zcap = pk_get(u + 14);
        v.acc2 = pk_get(u + 16), v.acc3 = pk_get(u + 18), v.nz0 = pk_get(u + 20), v.nz1 = pk_get(u + 22);
        v.s = sc_unpack(pk_get(u + 24)), esum = pk_getd(u + 26), ecnt = pk_getd(u + 28);
        v.sum_hi = __float_as_uint(u[30]);
        ret32 = u[31];
    }
};

}  // namespace lbk
