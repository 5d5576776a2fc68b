// lbk8s_host.h — the host helpers the library's units share: error reporting, config
// validation, the state layout and the launch geometry.  Declarations only: each helper is
// defined in exactly one unit (lbk8s_env.hip unless noted).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "lbk8s.h"
#include "lbk8s_common.h"

namespace lbk {

extern thread_local std::string g_err;  // lb_last_error's message
int fail(const char* msg);              // sets g_err, returns -1
int check_launch();                     // hipGetLastError() -> 0 / -2 (and g_err)
int validate(const lb_config* c);

struct Geo {
    bool tpe;       // thread-per-env path (E <= 8)
    int W, EPL, EP, NZW;
};

// E > 8: W-lane slices.  Few envs (B < 32768): one env per wave (W = 16/32/64 by E), so
// the launch still has thousands of waves; many envs: 4 envs per wave up to E = 64, so
// the per-env scalar chain (Philox, logs, reward) is issued once per 4 envs and 4x more
// envs are in flight per CU.  Measured at E = 64 (A/B builds, profiles/r01_ablation.jsonl): 2^20 envs 1.45 ->
// 1.00 ms per step, 4096 envs 8.9 vs 20.7 us.  Both shapes give the same EP = W * EPL
// (the next power of two >= max(E, 16)), so the state layout does not depend on B.
constexpr int64_t WIDE_SLICE_MAX_B = 32768;
// E <= 8, few envs (config 2: 4096): 64-thread blocks, so the batch spreads over 4x more
// CUs (every TPE kernel works per wave).
constexpr int64_t SMALL_TPE_MAX_B = 65536;

Geo geometry(const lb_config* c, int64_t B = 0);

struct Offsets {
    uint64_t lat_lut, cpu_lut, lat0, emeta, edyn, t, sc, topo, zcap, nzone, acc2, acc3, sum_lat,
        sum_cpu, sum_hi, total, last_r, rew64, rec, end;
};

Offsets offsets(const lb_config* c, int64_t B);
Params make_params(void* state, const lb_config* c, int64_t B);

// BODY with the slice geometry (Geo::W, Geo::EPL) as the constants W and EPL
#define LB_DISPATCH_SLICE(W_, EPL_, BODY)                                         \
    do {                                                                          \
        if (W_ == 16 && EPL_ == 1) { constexpr int W = 16, EPL = 1; BODY; }       \
        else if (W_ == 16 && EPL_ == 2) { constexpr int W = 16, EPL = 2; BODY; }  \
        else if (W_ == 16 && EPL_ == 4) { constexpr int W = 16, EPL = 4; BODY; }  \
        else if (W_ == 32 && EPL_ == 4) { constexpr int W = 32, EPL = 4; BODY; }  \
        else if (W_ == 32 && EPL_ == 1) { constexpr int W = 32, EPL = 1; BODY; }  \
        else if (W_ == 64 && EPL_ == 1) { constexpr int W = 64, EPL = 1; BODY; }  \
        else if (W_ == 64 && EPL_ == 2) { constexpr int W = 64, EPL = 2; BODY; }  \
        else if (W_ == 64 && EPL_ == 4) { constexpr int W = 64, EPL = 4; BODY; }  \
        else return fail("unsupported geometry");                                 \
    } while (0)

unsigned slice_blocks(int64_t B, int W);
unsigned env_blocks(int64_t B);
int device_cus();

// lbk8s_policies.hip: the launches of LB_POLICY_ROUND_ROBIN .. LB_POLICY_REWARD_GREEDY that have
// kernels of their own (p, g: make_params / geometry of the call)
//   lb_policy(LB_POLICY_REWARD_GREEDY): lanes over the endpoints in the slice layout with
//   E > 8, else one lane per env
int launch_policy_reward_greedy(const Params& p, const Geo& g, int32_t* actions_out, hipStream_t s);
//   lb_rollout: k_rollout_slice_k8s (slice layout) / k_rollout_tpe<NB, KIND, PRE> (thread-per-env, N <= 64)
int launch_rollout_k8s(const Params& p, const Geo& g, int policy, int steps, bool pre, int32_t* actions_out,
                       hipStream_t s);

// k_deepsets_fwd numbers its waves wave-major (wave w of block b = w * grid + b): every CU
// gets a block as soon as there are as many groups as CUs (lbk8s_ds.hip)
unsigned ds_grid_spread(int64_t groups);

}  // namespace lbk
