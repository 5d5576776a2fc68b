// lbk8s_ds.hip — the deep-sets forwards (lbk8s_deepsets.h) and their entry points: the weight
// pack, the inference, greedy-action, sampling and training forwards, the DQN act, the forward
// pair, and the one rule that picks a forward's kernel variant.
//
// Public ABI: include/lbk8s.h; the host helpers: lbk8s_host.h.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "lbk8s.h"
#include "lbk8s_common.h"
#include "lbk8s_deepsets.h"
#include "lbk8s_host.h"

#ifndef LB_DS_WAVES_PER_SIMD
#define LB_DS_WAVES_PER_SIMD 1
#endif

namespace lbk {

__global__ void k_ds_pack(lb_ds_weights w, float* out) { ds_pack_one(w, out, blockIdx.x * blockDim.x + threadIdx.x); }

unsigned ds_grid_spread(int64_t groups) { return (unsigned)std::min<int64_t>(groups, device_cus()); }

}  // namespace lbk

using namespace lbk;

namespace {
// persistent grid for the deep-sets kernels (the weight image is staged once per block)
unsigned ds_grid(int64_t groups) {
    const int64_t want = (groups + DS_BLOCK / 64 - 1) / (DS_BLOCK / 64);
    return (unsigned)std::min<int64_t>(want, device_cus());
}

// Which k_deepsets_fwd<TS, P, MODE, XR> (or k_ds_fwd_pair<1, P>) a forward takes: the one rule,
// shared by ds_forward_launch, lb_ds_forward_pair and lb_ds_forward_kernel (which reports it).
// ts == 0 is the chunked kernel (k_deepsets_fwd_big).
struct DSVariant {
    int ts, P, xr;
};
DSVariant ds_forward_variant(int which, int64_t B, int R) {
    if (R > LB_DS_MAX_ELEMENTS) return {0, 1, 0};  // large sets: streamed in chunks, one env per wave
    // a wave takes P envs per iteration: P = 4 for R <= 16, 2 for R <= 32, else 1 -- fewer
    // when the batch would leave SIMDs of the chip idle (the DQN vector step's 4096 envs:
    // 1,024 groups of four, one per SIMD; its 128-set train step)
    const int ts = (R + 15) / 16;
    // (the greedy-action forward of small sets takes at most two envs per iteration: its Gamma
    // terms on the VALU, the arithmetic of k_dqn_step's Q forward)
    // (the sampling forward is LB_DS_FWD's code up to the logits and the value: its variant too)
    int P = ts == 1 ? (which == LB_DS_FWD_ARGMAX ? 2 : 4) : (ts == 2 ? 2 : 1);
    const int64_t simds = (int64_t)device_cus() * 4 * LB_DS_WAVES_PER_SIMD;
    while (P > 1 && (B + P - 1) / P < simds) P /= 2;
    // the training forward at R = 16 TS + 1 (config 4's 65): TS tiles and the extra row (XR)
    if (which == LB_DS_FWD_TRAIN && (R == 49 || R == 65)) return {ts - 1, 1, 1};
    return {ts, P, 0};
}

template <int MODE>
void ds_forward_launch(const DSParams& p, hipStream_t s) {
    static_assert(MODE == LB_DS_FWD || MODE == LB_DS_FWD_TRAIN || MODE == LB_DS_FWD_ARGMAX ||
                      MODE == LB_DS_FWD_SAMPLE || MODE == DS_FWD_WHERE,
                  "k_deepsets_fwd's MODE is lb_ds_forward_kernel's `which` (or the flagged LB_DS_FWD)");
    // (the flagged forward is LB_DS_FWD's code on the flagged sets: its variant at the same shape)
    const DSVariant v = ds_forward_variant(MODE == DS_FWD_WHERE ? (int)LB_DS_FWD : MODE, p.B, p.R);
    if (v.ts == 0) {
        hipLaunchKernelGGL((k_deepsets_fwd_big<MODE>), dim3(ds_grid(p.B)), dim3(DS_BLOCK), 0, s, p);
        return;
    }
    const int ts = v.ts, P = v.P;
    const unsigned grid = ds_grid_spread((p.B + P - 1) / P);
    if constexpr (MODE == 1) {
        if (v.xr) {
            if (ts == 3) hipLaunchKernelGGL((k_deepsets_fwd<3, 1, 1, true>), dim3(grid), dim3(DS_BLOCK), 0, s, p);
            else hipLaunchKernelGGL((k_deepsets_fwd<4, 1, 1, true>), dim3(grid), dim3(DS_BLOCK), 0, s, p);
            return;
        }
    }
    switch (ts) {
        case 1:
            if (P == 4) hipLaunchKernelGGL((k_deepsets_fwd<1, 4, MODE>), dim3(grid), dim3(DS_BLOCK), 0, s, p);
            else if (P == 2) hipLaunchKernelGGL((k_deepsets_fwd<1, 2, MODE>), dim3(grid), dim3(DS_BLOCK), 0, s, p);
            else hipLaunchKernelGGL((k_deepsets_fwd<1, 1, MODE>), dim3(grid), dim3(DS_BLOCK), 0, s, p);
            break;
        case 2:
            if (P == 2) hipLaunchKernelGGL((k_deepsets_fwd<2, 2, MODE>), dim3(grid), dim3(DS_BLOCK), 0, s, p);
            else hipLaunchKernelGGL((k_deepsets_fwd<2, 1, MODE>), dim3(grid), dim3(DS_BLOCK), 0, s, p);
            break;
        case 3: hipLaunchKernelGGL((k_deepsets_fwd<3, 1, MODE>), dim3(grid), dim3(DS_BLOCK), 0, s, p); break;
        case 4: hipLaunchKernelGGL((k_deepsets_fwd<4, 1, MODE>), dim3(grid), dim3(DS_BLOCK), 0, s, p); break;
        default: hipLaunchKernelGGL((k_deepsets_fwd<5, 1, MODE>), dim3(grid), dim3(DS_BLOCK), 0, s, p); break;
    }
}
}  // namespace

extern "C" {

int lb_ds_pack(const lb_ds_weights* w, float* frag_out, void* stream) {
    if (!w || !frag_out) return fail("weights/frag_out NULL");
    for (int i = 0; i < 3; ++i)
        if (!w->actor_lambda[i] || !w->actor_gamma[i]) return fail("actor weights are required");
    hipLaunchKernelGGL(k_ds_pack, dim3((DS_IMG_FLOATS + 255) / 256), dim3(256), 0, (hipStream_t)stream, *w, frag_out);
    return check_launch();
}

int lb_ds_forward(const float* frag, const float* obs, int64_t num_envs, int32_t num_elements, float* logits_out,
                  float* value_out, void* stream) {
    static_assert(DS_IMG_FLOATS == LB_DS_FRAG_FLOATS, "weight image layout and header disagree");
    if (!frag || !obs || num_envs < 1) return fail("frag/obs NULL or num_envs < 1");
    if (num_elements < 1 || num_elements > LB_DS_MAX_ELEMENTS_FWD)
        return fail("num_elements must be in [1, 257] (LB_DS_MAX_ELEMENTS_FWD)");
    if (!logits_out && !value_out) return 0;
    DSParams p{obs, frag, logits_out, value_out, num_envs, num_elements, logits_out != nullptr, value_out != nullptr,
               nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ds_forward_launch<0>(p, (hipStream_t)stream);
    return check_launch();
}

int lb_ds_value_where(const float* frag, const float* obs, const uint8_t* flags, int64_t num_envs,
                      int32_t num_elements, float* value_out, void* stream) {
    if (!frag || !obs || !flags || !value_out || num_envs < 1)
        return fail("lb_ds_value_where: frag/obs/flags/value_out NULL or num_envs < 1");
    if (num_elements < 1 || num_elements > LB_DS_MAX_ELEMENTS_FWD)
        return fail("lb_ds_value_where: num_elements must be in [1, 257] (LB_DS_MAX_ELEMENTS_FWD)");
    // lb_ds_forward's parameters with logits_out NULL (the critic alone); the flags ride in masks
    DSParams p{obs, frag, nullptr, value_out, num_envs, num_elements, 0, 1,
               nullptr, nullptr, nullptr, nullptr, nullptr, flags};
    ds_forward_launch<DS_FWD_WHERE>(p, (hipStream_t)stream);
    return check_launch();
}

int lb_ds_q_argmax(const float* frag, const float* obs, int64_t num_envs, int32_t num_elements, const uint8_t* masks,
                   float* q_out, int32_t* actions_out, void* stream) {
    if (!frag || !obs || !actions_out || num_envs < 1) return fail("frag/obs/actions_out NULL or num_envs < 1");
    if (num_elements < 1 || num_elements > LB_DS_MAX_ELEMENTS_FWD)
        return fail("num_elements must be in [1, 257] (LB_DS_MAX_ELEMENTS_FWD)");
    DSParams p{obs, frag, q_out, nullptr, num_envs, num_elements, 1, 0, nullptr, nullptr, nullptr, nullptr, actions_out,
               masks};
    ds_forward_launch<2>(p, (hipStream_t)stream);
    return check_launch();
}

int lb_ds_sample(const float* frag, const float* obs, int64_t num_envs, int32_t num_elements, const uint8_t* masks,
                 const float* uniforms, float* logits_out, int32_t* actions_out, float* actions_f32_out,
                 float* logprob_out, float* value_out, void* stream) {
    if (!frag || !obs || !uniforms || !actions_out || !logprob_out || num_envs < 1)
        return fail("lb_ds_sample: frag/obs/uniforms/actions_out/logprob_out NULL or num_envs < 1");
    if (num_elements < 1 || num_elements > LB_DS_MAX_ELEMENTS_FWD)
        return fail("num_elements must be in [1, 257] (LB_DS_MAX_ELEMENTS_FWD)");
    DSParams p{obs, frag, logits_out, value_out, num_envs, num_elements, 1, value_out != nullptr,
               nullptr, nullptr, nullptr, nullptr, actions_out, masks};
    p.uniforms = uniforms;
    p.actions_f32 = actions_f32_out;
    p.logprob = logprob_out;
    ds_forward_launch<LB_DS_FWD_SAMPLE>(p, (hipStream_t)stream);
    return check_launch();
}

int lb_dqn_act(const float* frag, const float* obs, int64_t num_envs, int32_t num_elements, const uint8_t* masks,
               const void* state, const lb_config* cfg, const lb_dqn_explore* ex, int32_t* actions_out,
               void* stream) {
    if (int r = validate(cfg)) return r;
    if (!frag || !obs || !state || !ex || !actions_out || num_envs < 1)
        return fail("frag/obs/state/ex/actions_out NULL or num_envs < 1");
    if (!ex->vstep_in || !ex->vstep_out || ex->vstep_in == ex->vstep_out || !ex->explore_out)
        return fail("lb_dqn_explore: device words NULL (or vstep_in == vstep_out)");
    if (cfg->rng_mode != LB_RNG_PHILOX) return fail("lb_dqn_act draws in Philox mode only");
    const int32_t A = cfg->num_endpoints + (cfg->rejection_allowed ? 1 : 0);
    if (num_elements != A) return fail("lb_dqn_act: num_elements must be the env's action count (R)");
    if (num_elements < 1 || num_elements > LB_DS_MAX_ELEMENTS_FWD)
        return fail("num_elements must be in [1, 257] (LB_DS_MAX_ELEMENTS_FWD)");
    const Params e = make_params(const_cast<void*>(state), cfg, num_envs);
    DSParams p{obs, frag, nullptr, nullptr, num_envs, num_elements, 1, 0, nullptr, nullptr, nullptr, nullptr,
               actions_out, masks};
    p.ex_on = 1;
    p.ex = *ex;
    p.ex_acc3 = e.acc3;
    p.ex_sc = e.sc;
    p.ex_env_offset = e.env_id_offset;
    p.ex_key0 = e.key0;
    p.ex_key1 = e.key1;
    ds_forward_launch<2>(p, (hipStream_t)stream);
    return check_launch();
}

int lb_ds_train_forward(const float* frag, const float* obs, int64_t num_envs, int32_t num_elements,
                        float* logits_out, float* psi_mean_out, float* save_actor, float* save_critic,
                        float* setvec_out, void* stream) {
    if (!frag || !obs || !setvec_out || num_envs < 1) return fail("frag/obs/setvec_out NULL or num_envs < 1");
    if (num_elements < 1 || num_elements > LB_DS_MAX_ELEMENTS_TRAIN)
        return fail("num_elements must be in [1, 257] (LB_DS_MAX_ELEMENTS_TRAIN)");
    if (!logits_out && !psi_mean_out) return 0;
    if ((logits_out && !save_actor) || (psi_mean_out && !save_critic))
        return fail("a head's activation buffer is NULL");
    DSParams p{obs, frag, logits_out, nullptr, num_envs, num_elements, logits_out != nullptr, psi_mean_out != nullptr,
               save_actor, save_critic, psi_mean_out, setvec_out, nullptr, nullptr};
    ds_forward_launch<1>(p, (hipStream_t)stream);
    return check_launch();
}

int lb_ds_forward_kernel(int32_t which, int64_t num_envs, int32_t num_elements, int32_t* tiles_out,
                         int32_t* sets_per_wave_out, int32_t* extra_row_out) {
    // (4 names no forward: the kinds of ABI 15 end at LB_DS_FWD_PAIR = 3, and 4 was refused there)
    if (which < LB_DS_FWD || which > LB_DS_FWD_SAMPLE || which == LB_DS_FWD_PAIR + 1)
        return fail("lb_ds_forward_kernel: unknown forward kind");
    if (num_envs < 1 || !tiles_out || !sets_per_wave_out || !extra_row_out)
        return fail("lb_ds_forward_kernel: num_envs < 1 or an output NULL");
    // (each forward's own bound: a call it would reject has no kernel to name)
    const int32_t max_r = which == LB_DS_FWD_PAIR ? 16 : which == LB_DS_FWD_TRAIN ? LB_DS_MAX_ELEMENTS_TRAIN
                                                                                    : LB_DS_MAX_ELEMENTS_FWD;
    if (num_elements < 1 || num_elements > max_r)
        return fail("lb_ds_forward_kernel: num_elements out of the forward's range");
    const DSVariant v = ds_forward_variant(which, num_envs, num_elements);
    *tiles_out = v.ts;
    *sets_per_wave_out = v.P;
    *extra_row_out = v.xr;
    return 0;
}

int lb_ds_forward_pair(const float* frag_a, const float* obs_a, float* logits_a, const float* frag_b,
                       const float* obs_b, float* logits_b, float* save_actor_b, float* setvec_b, int64_t num_envs,
                       int32_t num_elements, void* stream) {
    if (!frag_a || !obs_a || !logits_a || !frag_b || !obs_b || !logits_b || !save_actor_b || !setvec_b || num_envs < 1)
        return fail("lb_ds_forward_pair: NULL buffer or num_envs < 1");
    if (num_elements < 1 || num_elements > 16) return fail("lb_ds_forward_pair: num_elements must be in [1, 16]");
    DSParams a{obs_a, frag_a, logits_a, nullptr, num_envs, num_elements, 1, 0,
               nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    DSParams b{obs_b, frag_b, logits_b, nullptr, num_envs, num_elements, 1, 0,
               save_actor_b, nullptr, nullptr, setvec_b, nullptr, nullptr};
    // P as ds_forward_launch picks it for one of the two (the batch against the chip's SIMDs)
    const int P = ds_forward_variant(LB_DS_FWD_PAIR, num_envs, num_elements).P;
    const int ga = (int)ds_grid_spread((num_envs + P - 1) / P);
    const dim3 grid(2 * ga);
    if (P == 4) hipLaunchKernelGGL((k_ds_fwd_pair<1, 4>), grid, dim3(DS_BLOCK), 0, (hipStream_t)stream, a, b, ga);
    else if (P == 2) hipLaunchKernelGGL((k_ds_fwd_pair<1, 2>), grid, dim3(DS_BLOCK), 0, (hipStream_t)stream, a, b, ga);
    else hipLaunchKernelGGL((k_ds_fwd_pair<1, 1>), grid, dim3(DS_BLOCK), 0, (hipStream_t)stream, a, b, ga);
    return check_launch();
}

}  // extern "C"
