// lbk8s_env.hip — the vectorized LoadBalancerK8sEnv on MI355X (gfx950): the state layout and
// config validation, the env's kernels and their C ABI (init, reset, step, rollout, policies,
// accessors), and the host helpers every unit of the library shares (lbk8s_host.h).
//
// Reference hot path: /root/reference/envs/loadbalancer_k8s_env.py (reset :290-400,
// step :403-513, take_action :578-686, get_reward :516-567, get_state :688-758,
// next_request :1131-1163), envs/utils.py (gini :132-143, endpoint list :33-64) and
// envs/baselines.py (greedy policies :6-35).  Public ABI: include/lbk8s.h; design
// notes: DESIGN.md.
//
// Two state layouts / kernel shapes share one state representation (lbk8s_common.h):
//   * E <= 8 : k_step_tpe    — one lane per env, LDS-staged coalesced obs (lbk8s_tpe.h);
//              k_rollout_tpe — K steps per launch, the env in registers (lb_rollout)
//   * E >  8 : k_step_slice  — one W-lane slice per env (4 envs per wave up to E = 64),
//                              lanes over endpoints; k_rollout_slice (lbk8s_slice.h)
//
// Compiled together with lbk8s_steps.hip (the one-launch step kernels) as lbk8s_env_steps.hip.
// The library's other units: lbk8s_ds.hip (deep-sets forwards), lbk8s_ds_train.hip (their
// training side), lbk8s_learn.hip (replay, episode log, GAE), lbk8s_lean_inst.hip (the lean
// rollout, one unit per policy).  lbk8s_policies.hip (the policies LB_POLICY_ROUND_ROBIN ..
// LB_POLICY_REWARD_GREEDY: the reward-greedy lb_policy kernels and their lb_rollout kernels) is
// compiled with lbk8s_learn.hip.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <string>
#include <type_traits>

#include "lbk8s.h"
#include "lbk8s_common.h"
#include "lbk8s_host.h"
#include "lbk8s_slice.h"
#include "lbk8s_tpe.h"
#include "lbk8s_rollout.h"
#include "lbk8s_lean_launch.h"

namespace lbk {

// LAT[k][j]: endpoint latency after j selections from trunc(initial) = k
// (increase_endpoint_latency :1013-1023 then decrease_endpoint_latency :1052-1060 in the
// same step); CPU[c][M]: node cpu after M selections (:861-887 then :937-960).
__global__ void k_luts(double* lat_lut, double* cpu_lut) {
    int row = blockIdx.x * blockDim.x + threadIdx.x;
    // column-major ([j][k]): envs stepping in lockstep hold similar counters, so one
    // step's lookups touch a few columns (L1/L2-resident) rather than scattered rows
    if (row < LAT_ROWS) {
        double v = (double)row;
        lat_lut[row] = v;
        for (int j = 1; j < JCAP; ++j) {
            double inc = clamp_lat(trunc(v) * 1.5);
            v = clamp_lat(trunc(inc) / 1.15);
            lat_lut[(int64_t)j * LAT_ROWS + row] = v;
        }
    } else if (row < LAT_ROWS + CPU_ROWS) {
        int c = row - LAT_ROWS;
        double w = (double)c;
        cpu_lut[c] = w;
        for (int m = 1; m < JCAP; ++m) {
            w = clamp_cpu(clamp_cpu(w * 1.15) / 1.15);
            cpu_lut[(int64_t)m * CPU_ROWS + c] = w;
        }
    }
}

// __init__ (:86-287): the only state that reaches reset() is current_time, advanced by
// __init__'s own next_request() (:267).
__global__ void k_init(Params p, int trace) {
    int64_t env = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= p.B) return;
    for (int e = 0; e < p.EP; ++e) {
        int64_t i = eidx(p, env, e);
        p.lat0[i] = 0.0;
        p.emeta[i] = 0;
        p.edyn[i] = 0;
    }
    double t;
    if (trace) {
        t = p.tr.t0[env];
    } else {
        U4 w = draw(p, env, 0, 0, D_INIT);
        t = 0.0 + p.inv_rate * std_exp(w.x, w.y);
    }
    p.t[env] = t;
    p.sc[env] = 0;
    p.topo[env] = 0;
    p.zcap[env] = 0;
    for (int w = 0; w < p.NZW; ++w) p.nzone[w * p.B + env] = 0;
    p.acc2[env] = 0;
    p.acc3[env] = 0;
    p.sum_lat[env] = 0;
    p.sum_cpu[env] = 0;
    p.sum_hi[env] = 0;
    p.total[env] = 0.0;
    p.last_r[env] = p.init_last_r;
}

// envs/baselines.py (:6-35): argmin topology latency / argmax zone cpu capacity / argmin
// endpoint cpu over feasible = mask[:-1] (masks are all True, :808-821), first index on
// ties (numpy); or a uniform random action keyed by (env, episode, step).  One lane/env.
// Also round robin, least loaded and least latency (LB_POLICY_* 4..6, include/lbk8s.h), over all
// E endpoints; reward greedy has kernels of its own (lbk8s_policies.hip).
__global__ void k_policy(Params p, int kind, int32_t* out) {
    int64_t env = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= p.B) return;
    const Scal s = sc_unpack(p.sc[env]);
    if (kind == LB_POLICY_RANDOM) {
        out[env] = random_action(p, env, p.acc3[env], s.step);
        return;
    }
    if (kind == LB_POLICY_ROUND_ROBIN) {
        out[env] = s.step % p.E;
        return;
    }
    // the baselines.py kinds: e < A - 1; the others (least loaded, least latency): every endpoint
    const int nf = kind > LB_POLICY_RANDOM ? p.E : p.A - 1;
    if (nf <= 0) { out[env] = p.A - 1; return; }
    const uint64_t topo = p.topo[env], zc = p.zcap[env];
    double best = 0.0;
    int bi = 0;
    for (int e = 0; e < nf; ++e) {
        const int64_t i = eidx(p, env, e);
        const uint32_t em = p.emeta[i];
        double val;
        if (kind == LB_POLICY_TOPOLOGY_GREEDY) val = (double)topo_val(topo, em_zone(em), s.rz);
        else if (kind == LB_POLICY_ZONE_CPU_GREEDY) val = -(double)zcap_val(zc, em_zone(em));
        else if (kind == LB_POLICY_LEAST_LOADED) val = (double)ed_j(p.edyn[i]);
        else if (kind == LB_POLICY_LEAST_LATENCY)
            val = lat_of(p, p.lat0[i], p.edyn[i]) + (double)topo_val(topo, em_zone(em), s.rz);
        else val = cpu_of(p, em, p.edyn[i]);
        if (e == 0 || val < best) { best = val; bi = e; }
    }
    out[env] = bi;
}

__global__ void k_field(Params p, int field, double* out) {
    int64_t env = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= p.B) return;
    const Scal s = sc_unpack(p.sc[env]);
    switch (field) {
    case LB_FIELD_CURRENT_TIME: out[env] = p.t[env]; return;
    case LB_FIELD_CURRENT_STEP: out[env] = (double)s.step; return;
    case LB_FIELD_REQUEST_ZONE: out[env] = (double)s.rz; return;
    case LB_FIELD_REQUEST_THRESHOLD: out[env] = (double)threshold(s.thr_idx); return;
    default: break;
    }
    const uint64_t topo = p.topo[env], zc = p.zcap[env];
    for (int e = 0; e < p.E; ++e) {
        const int64_t i = eidx(p, env, e);
        const uint32_t em = p.emeta[i], ed = p.edyn[i];
        double v;
        switch (field) {
        case LB_FIELD_ENDPOINT_LATENCY: v = lat_of(p, p.lat0[i], ed); break;
        case LB_FIELD_ENDPOINT_CPU: v = cpu_of(p, em, ed); break;
        case LB_FIELD_ENDPOINT_TOPOLOGY_LATENCY: v = (double)topo_val(topo, em_zone(em), s.rz); break;
        case LB_FIELD_ENDPOINT_ZONE_CPU_CAPACITY: v = (double)zcap_val(zc, em_zone(em)); break;
        case LB_FIELD_ENDPOINT_ZONE: v = (double)em_zone(em); break;
        case LB_FIELD_ENDPOINT_NODE: v = (double)em_node(em); break;
        default: v = (double)ed_j(ed); break;  // LB_FIELD_LOAD_SERVED
        }
        out[env * p.E + e] = v;
    }
}

__global__ void k_stats(Params p, double* out) {
    int64_t env = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= p.B) return;
    write_stats_row(p, out + env * LB_ST_K, sc_unpack(p.sc[env]), p.acc2[env], p.acc3[env], p.total[env],
                    p.sum_lat[env], p.sum_cpu[env], p.sum_hi[env]);
}

__global__ void k_status(Params p, uint32_t* flags) {
    int64_t env = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t f = 0;
    if (env < p.B) {
        Scal s = sc_unpack(p.sc[env]);
        if (s.bad) f |= LB_STATUS_BAD_ACTION;
        if (!s.reset_done) f |= LB_STATUS_NOT_RESET;
    }
    if (f) atomicOr(flags, f);
}

// ---- host side ---------------------------------------------------------------------------
thread_local std::string g_err;
#ifdef LB_EXPERIMENTS
// experiment switch of a diagnostic build (-DLB_EXPERIMENTS; lbx_set_rollout_variant,
// tools/roll_variants.py): 1 = k_rollout_img where k_rollout_lean would run, 3 = k_rollout_tpe
// for every L >= K launch (A/B references)
int g_rollout_variant = 0;
#else
constexpr int g_rollout_variant = 0;
#endif

int fail(const char* msg) {
    g_err = msg;
    return -1;
}

Geo geometry(const lb_config* c, int64_t B) {
    Geo g;
    const int E = c->num_endpoints;
    // E <= 8: one lane per env, except few envs (B < 32768, config 2), where lanes over
    // endpoints (the wide slice shape) cut each wave's serial chain: 4096 default envs
    // 10.8 -> 7.4 us per lb_step (A/B builds, profiles/r01_ablation.jsonl).
    // cfg->geometry pins the choice for E <= 8 (the state layout follows it).
    g.tpe = E <= TPE_E;
    if (g.tpe && B > 0 && B < WIDE_SLICE_MAX_B) g.tpe = false;
    if (E <= TPE_E && c->geometry == LB_GEOMETRY_TPE) g.tpe = true;
    if (c->geometry == LB_GEOMETRY_SLICE) g.tpe = false;
    if (g.tpe) {
        g.W = 1;
        g.EPL = 1;
        g.EP = E;
    } else {
        const bool wide = B < WIDE_SLICE_MAX_B;
        if (wide) {
            g.W = E <= 16 ? 16 : E <= 32 ? 32 : 64;
            g.EPL = E <= 64 ? 1 : E <= 128 ? 2 : 4;
        } else {
            g.W = E <= 64 ? 16 : E <= 128 ? 32 : 64;
            g.EPL = E <= 16 ? 1 : E <= 32 ? 2 : 4;
        }
        g.EP = g.W * g.EPL;
    }
    g.NZW = (c->num_nodes + 31) / 32;
    return g;
}

uint64_t align_up(uint64_t x) { return (x + 255) & ~(uint64_t)255; }

Offsets offsets(const lb_config* c, int64_t B) {
    Geo g = geometry(c, B);
    Offsets o;
    uint64_t x = 0;
    auto take = [&](uint64_t bytes) { uint64_t r = x; x = align_up(x + bytes); return r; };
    o.lat_lut = take((uint64_t)LAT_ROWS * JCAP * 8);
    o.cpu_lut = take((uint64_t)CPU_ROWS * JCAP * 8);
    const uint64_t BE = (uint64_t)B * g.EP;
    o.lat0 = take(BE * 8);
    o.emeta = take(BE * 4);
    o.edyn = take(BE * 4);
    o.t = take(B * 8);
    o.sc = take(B * 8);
    o.topo = take(B * 8);
    o.zcap = take(B * 8);
    o.nzone = take((uint64_t)B * g.NZW * 8);
    o.acc2 = take(B * 8);
    o.acc3 = take(B * 8);
    o.sum_lat = take(B * 8);
    o.sum_cpu = take(B * 8);
    o.sum_hi = take(B * 4);
    o.total = take(B * 8);
    o.last_r = take(B * 8);
    o.rew64 = take(B * 8);
    // thread-per-env layout: k_rollout_tpe's next-episode records (scratch, per launch)
    o.rec = take(g.tpe ? (uint64_t)B * RO_REC_BYTES : 0);
    o.end = x;
    return o;
}

double initial_last_reward(const lb_config* c) {
    // get_reward() right after reset(): penalty False, selected latency 0.0, topology 0.0,
    // cpu 1.0, all loads 0 (:297-327) — what an unrecognised first action returns.
    switch (c->reward_fn) {
    case LB_REWARD_NAIVE: return 1.0;
    case LB_REWARD_LATENCY: return -(0.0 + 0.0);
    case LB_REWARD_FAIRNESS: return 1.0 - 0.0;
    default: {
        volatile double cur = ((0.0 + 0.0) - 2.0) / 998.0;
        volatile double cpu = (1.0 - 1.0) / 99.0;
        volatile double a = c->latency_weight * (1.0 - cur);
        volatile double b = c->cpu_weight * (1.0 - cpu);
        volatile double g = c->gini_weight * (1.0 - 0.0);
        volatile double ab = a + b;
        return ab + g;
    }
    }
}

int validate(const lb_config* c) {
    if (!c) return fail("lb_config is NULL");
    if (c->num_endpoints < 1 || c->num_endpoints > EMAX) return fail("num_endpoints must be in [1, 256]");
    if (c->num_zones < 4)
        return fail("IndexError: num_zones < 4 (zone ids are drawn in [0,4), loadbalancer_k8s_env.py:354)");
    if (c->num_nodes < 24)
        return fail("IndexError: num_nodes < 24 (endpoint hosts are drawn in [0,24), loadbalancer_k8s_env.py:380)");
    if (c->num_nodes > 32 * NZW_MAX) return fail("num_nodes must be <= 256");
    if (c->episode_length < 1 || c->episode_length > CMAX) return fail("episode_length must be in [1, 1023]");
    if (c->reward_fn < 0 || c->reward_fn > 3) return fail("unknown reward_fn");
    if (c->rng_mode != LB_RNG_PHILOX && c->rng_mode != LB_RNG_TRACE) return fail("unknown rng_mode");
    if (c->geometry < LB_GEOMETRY_AUTO || c->geometry > LB_GEOMETRY_SLICE) return fail("unknown geometry");
    if (!(c->arrival_rate > 0.0)) return fail("arrival_rate must be > 0");
    return 0;
}

Params make_params(void* state, const lb_config* c, int64_t B) {
    Geo g = geometry(c, B);
    Offsets o = offsets(c, B);
    char* base = (char*)state;
    Params p;
    memset(&p, 0, sizeof(p));
    p.lat_lut = (double*)(base + o.lat_lut);
    p.cpu_lut = (double*)(base + o.cpu_lut);
    p.lat0 = (double*)(base + o.lat0);
    p.emeta = (uint32_t*)(base + o.emeta);
    p.edyn = (uint32_t*)(base + o.edyn);
    p.t = (double*)(base + o.t);
    p.sc = (uint64_t*)(base + o.sc);
    p.topo = (uint64_t*)(base + o.topo);
    p.zcap = (uint64_t*)(base + o.zcap);
    p.nzone = (uint64_t*)(base + o.nzone);
    p.acc2 = (uint64_t*)(base + o.acc2);
    p.acc3 = (uint64_t*)(base + o.acc3);
    p.sum_lat = (uint64_t*)(base + o.sum_lat);
    p.sum_cpu = (uint64_t*)(base + o.sum_cpu);
    p.sum_hi = (uint32_t*)(base + o.sum_hi);
    p.total = (double*)(base + o.total);
    p.last_r = (double*)(base + o.last_r);
    p.rew64 = (double*)(base + o.rew64);
    p.rec = g.tpe ? (uint4*)(base + o.rec) : nullptr;
    p.B = B;
    p.env_id_offset = c->env_id_offset;
    p.es = g.tpe ? B : 1;
    p.ee = g.tpe ? 1 : g.EP;
    p.E = c->num_endpoints;
    p.Z = c->num_zones;
    p.N = c->num_nodes;
    p.L = c->episode_length;
    p.R = c->num_endpoints + (c->rejection_allowed ? 1 : 0);
    p.A = p.R;
    p.EP = g.EP;
    p.NZW = g.NZW;
    p.reward_fn = c->reward_fn;
    p.rejection = c->rejection_allowed ? 1 : 0;
    p.auto_reset = c->auto_reset ? 1 : 0;
    p.inv_rate = 1.0 / c->arrival_rate;
    p.call = c->call_duration;
    p.lw = c->latency_weight;
    p.cw = c->cpu_weight;
    p.gw = c->gini_weight;
    p.init_last_r = initial_last_reward(c);
    p.key0 = (uint32_t)c->seed;
    p.key1 = (uint32_t)(c->seed >> 32);
    return p;
}

int check_launch() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        g_err = std::string("HIP launch failed: ") + hipGetErrorString(e);
        return -2;
    }
    return 0;
}

unsigned slice_blocks(int64_t B, int W) {
    int64_t per = BLOCK / W;
    return (unsigned)((B + per - 1) / per);
}
unsigned env_blocks(int64_t B) { return (unsigned)((B + BLOCK - 1) / BLOCK); }

int device_cus() {
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
            cus = 256;
    }
    return cus;
}

// Which kernel lb_rollout launches (lb_rollout_kernel reports it, LB_ROLLOUT_*).
// Per-lane addresses of the thread-per-env rollouts are 32-bit byte offsets from scalar bases
// (k_rollout_img: the state blob and the ep_stats rows; k_rollout_lean also the obs slot and
// the terminal observations), so they run only while every such offset fits in 32 bits; larger
// launches take k_rollout_tpe, which indexes in 64 bits.
int rollout_kernel(const lb_config* c, int64_t B, int32_t steps, bool outputs_all) {
    const Geo g = geometry(c, B);
    if (!g.tpe) return LB_ROLLOUT_SLICE;
    if (g.NZW > 2) return LB_ROLLOUT_STEPS;
    const bool pre = c->auto_reset && c->episode_length >= steps;
    if (!pre) return LB_ROLLOUT_TPE;
    const uint64_t lim = 0xFFFFFFFFull;
    const int R = c->num_endpoints + (c->rejection_allowed ? 1 : 0);
    const bool img_fits = offsets(c, B).end <= lim && (uint64_t)B * LB_ST_K * 8 <= lim;
    const bool lean_fits = img_fits && (uint64_t)B * R * 32 <= lim;
    const bool lean_shape = (c->num_endpoints == 8 && R == 9 && c->num_nodes <= 32) ||
                            (c->num_endpoints == 6 && R == 7 && c->num_nodes <= 64);
    if (lean_fits && lean_shape && B % 64 == 0 && B > SMALL_TPE_MAX_B && outputs_all &&
        g_rollout_variant == 0)
        return steps <= LEAN_SPLIT_MAX_K ? LB_ROLLOUT_LEAN_SPLIT : LB_ROLLOUT_LEAN;
    if (img_fits && g_rollout_variant != 3) return LB_ROLLOUT_IMG;
    return LB_ROLLOUT_TPE;
}

// lb_rollout's policy (LB_POLICY_*, validated by the caller) and one two-way choice of the
// launch as compile-time constants: f(std::integral_constant<int, policy>, std::bool_constant<flag>)
template <typename F>
void with_policy(int policy, bool flag, F f) {
    auto two = [&](auto kind) {
        if (flag) f(kind, std::true_type{});
        else f(kind, std::false_type{});
    };
    switch (policy) {
    case LB_POLICY_TOPOLOGY_GREEDY: two(std::integral_constant<int, LB_POLICY_TOPOLOGY_GREEDY>{}); break;
    case LB_POLICY_ZONE_CPU_GREEDY: two(std::integral_constant<int, LB_POLICY_ZONE_CPU_GREEDY>{}); break;
    case LB_POLICY_ENDPOINT_CPU_GREEDY: two(std::integral_constant<int, LB_POLICY_ENDPOINT_CPU_GREEDY>{}); break;
    default: two(std::integral_constant<int, LB_POLICY_RANDOM>{}); break;
    }
}

}  // namespace lbk

using namespace lbk;

extern "C" {

int lb_abi_version(void) { return LBK8S_ABI_VERSION; }

// (lb_source_hash, lb_build_flags, lb_build_compiler: lbk8s_build.cpp, rebuilt with every source change)

#ifdef LB_EXPERIMENTS
int lbx_set_rollout_variant(int v) { g_rollout_variant = v; return 0; }
#endif
#ifdef LB_TIMELINE
int lbx_set_timeline(uint64_t* buf) {  // k_rollout_img's (this unit) and k_rollout_lean's (one per policy unit)
    int r = hipMemcpyToSymbol(HIP_SYMBOL(g_timeline), &buf, sizeof(buf)) == hipSuccess ? 0 : -1;
    r |= lbx_set_timeline_lean_0(buf) | lbx_set_timeline_lean_1(buf) | lbx_set_timeline_lean_2(buf) |
         lbx_set_timeline_lean_3(buf);
    return r;
}
#endif

const char* lb_last_error(void) { return g_err.c_str(); }

int lb_validate_config(const lb_config* cfg) { return validate(cfg); }

int lb_state_bytes(const lb_config* cfg, int64_t num_envs, uint64_t* out_bytes) {
    if (int r = validate(cfg)) return r;
    if (num_envs < 1 || !out_bytes) return fail("num_envs must be >= 1 and out_bytes non-NULL");
    *out_bytes = offsets(cfg, num_envs).end;
    return 0;
}

int lb_init(void* state, const lb_config* cfg, int64_t num_envs, const lb_trace* trace, void* stream) {
    if (int r = validate(cfg)) return r;
    if (!state || num_envs < 1) return fail("state NULL or num_envs < 1");
    const bool tr = cfg->rng_mode == LB_RNG_TRACE;
    if (tr && (!trace || !trace->t0)) return fail("trace mode: lb_init needs trace->t0");
    Params p = make_params(state, cfg, num_envs);
    if (tr) p.tr = *trace;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_luts, dim3((LAT_ROWS + CPU_ROWS + 127) / 128), dim3(128), 0, s, p.lat_lut, p.cpu_lut);
    if (int r = check_launch()) return r;
    hipLaunchKernelGGL(k_init, dim3(env_blocks(num_envs)), dim3(BLOCK), 0, s, p, tr ? 1 : 0);
    return check_launch();
}

int lb_reset(void* state, const lb_config* cfg, int64_t num_envs, const uint8_t* reset_mask,
             float* obs_out, const lb_trace* trace, void* stream) {
    if (int r = validate(cfg)) return r;
    if (!state || num_envs < 1) return fail("state NULL or num_envs < 1");
    const bool tr = cfg->rng_mode == LB_RNG_TRACE;
    if (tr && (!trace || !trace->reset_lat0 || !trace->reset_topo || !trace->reset_ntype ||
               !trace->reset_nzone || !trace->reset_ncpu || !trace->reset_enode || !trace->reset_x1 ||
               !trace->reset_x2 || !trace->reset_r || !trace->reset_n))
        return fail("trace mode: lb_reset needs every reset_* trace array");
    Params p = make_params(state, cfg, num_envs);
    if (tr) p.tr = *trace;
    p.obs = obs_out;
    p.reset_mask = reset_mask;
    Geo g = geometry(cfg, num_envs);
    hipStream_t s = (hipStream_t)stream;
    if (g.tpe) {
        if (num_envs <= SMALL_TPE_MAX_B) {
            const unsigned nb = (unsigned)((num_envs + 63) / 64);
            if (tr) hipLaunchKernelGGL((k_reset_tpe<true, 64>), dim3(nb), dim3(64), 0, s, p);
            else hipLaunchKernelGGL((k_reset_tpe<false, 64>), dim3(nb), dim3(64), 0, s, p);
            return check_launch();
        }
        if (tr) hipLaunchKernelGGL(k_reset_tpe<true>, dim3(env_blocks(num_envs)), dim3(BLOCK), 0, s, p);
        else hipLaunchKernelGGL(k_reset_tpe<false>, dim3(env_blocks(num_envs)), dim3(BLOCK), 0, s, p);
        return check_launch();
    }
    LB_DISPATCH_SLICE(g.W, g.EPL, {
        if (tr) hipLaunchKernelGGL((k_reset_slice<W, EPL, true>), dim3(slice_blocks(num_envs, W)), dim3(BLOCK), 0, s, p);
        else hipLaunchKernelGGL((k_reset_slice<W, EPL, false>), dim3(slice_blocks(num_envs, W)), dim3(BLOCK), 0, s, p);
    });
    return check_launch();
}

int lb_step(void* state, const lb_config* cfg, int64_t num_envs, const int32_t* actions,
            float* obs_out, float* reward_out, uint8_t* done_out, float* terminal_obs_out,
            double* ep_stats_out, const lb_trace* trace, void* stream) {
    if (int r = validate(cfg)) return r;
    if (!state || num_envs < 1) return fail("state NULL or num_envs < 1");
    const bool tr = cfg->rng_mode == LB_RNG_TRACE;
    if (!actions && tr) return fail("actions NULL (the fused random policy) needs Philox mode");
    if (tr && (!trace || !trace->step_x1 || !trace->step_x2 || !trace->step_r || !trace->step_n))
        return fail("trace mode: lb_step needs trace->step_* arrays");
    if (tr && cfg->auto_reset &&
        (!trace->reset_lat0 || !trace->reset_topo || !trace->reset_ntype || !trace->reset_nzone ||
         !trace->reset_ncpu || !trace->reset_enode || !trace->reset_x1 || !trace->reset_x2 ||
         !trace->reset_r || !trace->reset_n))
        return fail("trace mode with auto_reset: lb_step needs the reset_* arrays (any step may end an episode)");
    Params p = make_params(state, cfg, num_envs);
    if (tr) p.tr = *trace;
    p.actions = actions;
    p.obs = obs_out;
    p.reward = reward_out;
    p.done = done_out;
    p.term_obs = terminal_obs_out;
    p.ep_stats = ep_stats_out;
    Geo g = geometry(cfg, num_envs);
    hipStream_t s = (hipStream_t)stream;
    if (g.tpe) {
        // auto-reset (the finishing envs' reset()) runs inside k_step_tpe
        const bool recompute = !tr && num_envs >= SCEN_RECOMPUTE_MIN_B;
        if (num_envs <= SMALL_TPE_MAX_B && !recompute) {
            const unsigned nb = (unsigned)((num_envs + 63) / 64);
            if (tr) hipLaunchKernelGGL((k_step_tpe<true, false, 64>), dim3(nb), dim3(64), 0, s, p);
            else hipLaunchKernelGGL((k_step_tpe<false, false, 64>), dim3(nb), dim3(64), 0, s, p);
        } else if (tr) {
            hipLaunchKernelGGL((k_step_tpe<true, false>), dim3(env_blocks(num_envs)), dim3(BLOCK), 0, s, p);
        } else if (recompute) {
            hipLaunchKernelGGL((k_step_tpe<false, true>), dim3(env_blocks(num_envs)), dim3(BLOCK), 0, s, p);
        } else {
            hipLaunchKernelGGL((k_step_tpe<false, false>), dim3(env_blocks(num_envs)), dim3(BLOCK), 0, s, p);
        }
        return check_launch();
    }
    LB_DISPATCH_SLICE(g.W, g.EPL, {
        const unsigned nb = slice_blocks(num_envs, W);
        if (tr) hipLaunchKernelGGL((k_step_slice<W, EPL, true>), dim3(nb), dim3(BLOCK), 0, s, p);
        else hipLaunchKernelGGL((k_step_slice<W, EPL, false>), dim3(nb), dim3(BLOCK), 0, s, p);
    });
    return check_launch();
}

int lb_reward64(void* state, const lb_config* cfg, int64_t num_envs, double** out) {
    if (int r = validate(cfg)) return r;
    if (!state || num_envs < 1 || !out) return fail("state/out NULL or num_envs < 1");
    *out = make_params(state, cfg, num_envs).rew64;
    return 0;
}

int lb_rollout_kernel(const lb_config* cfg, int64_t num_envs, int32_t steps, int32_t outputs_all,
                      int32_t* kernel_out) {
    if (int r = validate(cfg)) return r;
    if (num_envs < 1 || steps < 0 || !kernel_out) return fail("num_envs < 1, steps < 0 or kernel_out NULL");
    // (lb_rollout's own preconditions: a launch it would reject has no kernel to name)
    if (cfg->rng_mode != LB_RNG_PHILOX) return fail("lb_rollout draws in Philox mode only");
    *kernel_out = rollout_kernel(cfg, num_envs, steps, outputs_all != 0);
    return 0;
}

int lb_rollout(void* state, const lb_config* cfg, int64_t num_envs, int32_t policy, int32_t steps,
               float* obs_out, float* reward_out, uint8_t* done_out, int32_t* actions_out,
               float* terminal_obs_out, double* ep_stats_out, void* stream) {
    if (int r = validate(cfg)) return r;
    if (!state || num_envs < 1) return fail("state NULL or num_envs < 1");
    if (cfg->rng_mode != LB_RNG_PHILOX) return fail("lb_rollout draws in Philox mode only");
    if (policy < 0 || policy > LB_POLICY_REWARD_GREEDY) return fail("unknown policy kind");
    if (steps < 0) return fail("steps must be >= 0");
    const bool k8s = policy > LB_POLICY_RANDOM;  // kinds 4..7: kernels of lbk8s_policies.hip
    Geo g = geometry(cfg, num_envs);
    hipStream_t s = (hipStream_t)stream;
    if (g.tpe && g.NZW <= 2) {  // thread-per-env layout, N <= 64: K steps in one launch
        Params p = make_params(state, cfg, num_envs);
        p.obs = obs_out;
        p.reward = reward_out;
        p.done = done_out;
        p.term_obs = terminal_obs_out;
        p.ep_stats = ep_stats_out;
        const bool small = num_envs <= SMALL_TPE_MAX_B;
        const dim3 grid(small ? (unsigned)((num_envs + 63) / 64) : env_blocks(num_envs)), block(small ? 64 : BLOCK);
        // episodes at least as long as the launch (an env ends at most once in it): next
        // episodes drawn before the first step
        const bool pre = cfg->auto_reset && cfg->episode_length >= steps;
        // (no lean / image kernels for them: k_rollout_tpe at every shape)
        if (k8s) return launch_rollout_k8s(p, g, policy, (int)steps, pre, actions_out, s);
        const int rk = rollout_kernel(cfg, num_envs, steps, obs_out && reward_out && done_out && terminal_obs_out &&
                                                                ep_stats_out);
        if (rk == LB_ROLLOUT_LEAN || rk == LB_ROLLOUT_LEAN_SPLIT) {  // k_rollout_lean(_split) (lbk8s_lean.h), B % 64 == 0
            const bool naive = p.reward_fn == LB_REWARD_NAIVE, act = actions_out != nullptr;
            with_policy(policy, p.E == 8, [&](auto kind, auto e8) {
                constexpr int KIND = decltype(kind)::value, ET = decltype(e8)::value ? 8 : 6, RT = ET + 1,
                              NZW = decltype(e8)::value ? 1 : 2;
                if (naive && act) launch_lean<KIND, ET, RT, NZW, true, true>(p, num_envs, (int)steps, actions_out, s);
                else if (naive) launch_lean<KIND, ET, RT, NZW, true, false>(p, num_envs, (int)steps, actions_out, s);
                else if (act) launch_lean<KIND, ET, RT, NZW, false, true>(p, num_envs, (int)steps, actions_out, s);
                else launch_lean<KIND, ET, RT, NZW, false, false>(p, num_envs, (int)steps, actions_out, s);
            });
            return check_launch();
        }
        if (rk == LB_ROLLOUT_IMG) {  // k_rollout_img (lbk8s_rollout.h)
            const bool e8 = p.E == 8 && p.R == 9;
            with_policy(policy, small, [&](auto kind, auto sm) {
                constexpr int KIND = decltype(kind)::value, NB = decltype(sm)::value ? 64 : BLOCK;
                if (e8) hipLaunchKernelGGL((k_rollout_img<NB, KIND, 8, 9, 4>), grid, block, 0, s, p, (int)steps, actions_out);
                else hipLaunchKernelGGL((k_rollout_img<NB, KIND, 0, 0, 4>), grid, block, 0, s, p, (int)steps, actions_out);
            });
            return check_launch();
        }
        with_policy(policy, small, [&](auto kind, auto sm) {
            constexpr int KIND = decltype(kind)::value, NB = decltype(sm)::value ? 64 : BLOCK;
            if (pre) hipLaunchKernelGGL((k_rollout_tpe<NB, KIND, true>), grid, block, 0, s, p, (int)steps, actions_out);
            else hipLaunchKernelGGL((k_rollout_tpe<NB, KIND, false>), grid, block, 0, s, p, (int)steps, actions_out);
        });
        return check_launch();
    }
    if (g.tpe) {  // thread-per-env layout, N > 64: K policy + step launches
        if (policy != LB_POLICY_RANDOM && !actions_out)
            return fail("lb_rollout on the thread-per-env layout needs actions_out for a greedy policy");
        const int64_t R = cfg->num_endpoints + (cfg->rejection_allowed ? 1 : 0);
        for (int k = 0; k < steps; ++k) {
            int32_t* act = actions_out ? actions_out + k * num_envs : nullptr;
            if (act)
                if (int r = lb_policy(state, cfg, num_envs, policy, act, stream)) return r;
            if (int r = lb_step(state, cfg, num_envs, act, obs_out ? obs_out + k * num_envs * R * 8 : nullptr,
                                reward_out ? reward_out + k * num_envs : nullptr,
                                done_out ? done_out + k * num_envs : nullptr, terminal_obs_out, ep_stats_out,
                                nullptr, stream))
                return r;
        }
        return 0;
    }
    Params p = make_params(state, cfg, num_envs);
    p.obs = obs_out;
    p.reward = reward_out;
    p.done = done_out;
    p.term_obs = terminal_obs_out;
    p.ep_stats = ep_stats_out;
    if (k8s) return launch_rollout_k8s(p, g, policy, (int)steps, false, actions_out, s);
    if (g.W == 16 && g.EPL == 4 && p.E == 64 && p.R == 65 && g.NZW == 1) {  // config 4's shape, compile-time
        const dim3 grid(slice_blocks(num_envs, 16));
#define LB_SL64(RF_) hipLaunchKernelGGL((k_rollout_slice<16, 4, 64, 65, 1, RF_>), grid, dim3(BLOCK), 0, s, p, \
                                        (int)policy, (int)steps, actions_out)
        switch (p.reward_fn) {
        case LB_REWARD_NAIVE: LB_SL64(LB_REWARD_NAIVE); break;
        case LB_REWARD_LATENCY: LB_SL64(LB_REWARD_LATENCY); break;
        case LB_REWARD_FAIRNESS: LB_SL64(LB_REWARD_FAIRNESS); break;
        default: LB_SL64(LB_REWARD_MULTI); break;
        }
#undef LB_SL64
        return check_launch();
    }
    LB_DISPATCH_SLICE(g.W, g.EPL, {
        hipLaunchKernelGGL((k_rollout_slice<W, EPL>), dim3(slice_blocks(num_envs, W)), dim3(BLOCK), 0, s, p,
                           (int)policy, (int)steps, actions_out);
    });
    return check_launch();
}

int lb_policy(const void* state, const lb_config* cfg, int64_t num_envs, int32_t kind,
              int32_t* actions_out, void* stream) {
    if (int r = validate(cfg)) return r;
    if (!state || !actions_out || num_envs < 1) return fail("state/actions_out NULL");
    if (kind < 0 || kind > LB_POLICY_REWARD_GREEDY) return fail("unknown policy kind");
    Params p = make_params(const_cast<void*>(state), cfg, num_envs);
    if (kind == LB_POLICY_REWARD_GREEDY)
        return launch_policy_reward_greedy(p, geometry(cfg, num_envs), actions_out, (hipStream_t)stream);
    hipLaunchKernelGGL(k_policy, dim3(env_blocks(num_envs)), dim3(BLOCK), 0, (hipStream_t)stream, p, (int)kind,
                       actions_out);
    return check_launch();
}

int lb_get_field(const void* state, const lb_config* cfg, int64_t num_envs, int32_t field, double* out,
                 void* stream) {
    if (int r = validate(cfg)) return r;
    if (!state || !out || num_envs < 1) return fail("state/out NULL");
    if (field < 0 || field >= LB_FIELD_COUNT) return fail("unknown field");
    if (field == LB_FIELD_DT) return fail("dt is not stored (it only feeds obs column 7)");
    Params p = make_params(const_cast<void*>(state), cfg, num_envs);
    hipLaunchKernelGGL(k_field, dim3(env_blocks(num_envs)), dim3(BLOCK), 0, (hipStream_t)stream, p, (int)field, out);
    return check_launch();
}

int lb_get_stats(const void* state, const lb_config* cfg, int64_t num_envs, double* stats_out, void* stream) {
    if (int r = validate(cfg)) return r;
    if (!state || !stats_out || num_envs < 1) return fail("state/stats_out NULL");
    Params p = make_params(const_cast<void*>(state), cfg, num_envs);
    hipLaunchKernelGGL(k_stats, dim3(env_blocks(num_envs)), dim3(BLOCK), 0, (hipStream_t)stream, p, stats_out);
    return check_launch();
}

int lb_status(const void* state, const lb_config* cfg, int64_t num_envs, uint32_t* flags_out, void* stream) {
    if (int r = validate(cfg)) return r;
    if (!state || !flags_out || num_envs < 1) return fail("state/flags_out NULL");
    Params p = make_params(const_cast<void*>(state), cfg, num_envs);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(flags_out, 0, sizeof(uint32_t), s) != hipSuccess) return fail("hipMemsetAsync failed");
    hipLaunchKernelGGL(k_status, dim3(env_blocks(num_envs)), dim3(BLOCK), 0, s, p, flags_out);
    return check_launch();
}

}  // extern "C"
