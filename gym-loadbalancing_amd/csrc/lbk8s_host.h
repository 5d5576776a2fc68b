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

unsigned slice_blocks(int64_t B, int W);
unsigned env_blocks(int64_t B);
int device_cus();

// k_deepsets_fwd numbers its waves wave-major (wave w of block b = w * grid + b): every CU
// gets a block as soon as there are as many groups as CUs (lbk8s_ds.hip)
unsigned ds_grid_spread(int64_t groups);

}  // namespace lbk
