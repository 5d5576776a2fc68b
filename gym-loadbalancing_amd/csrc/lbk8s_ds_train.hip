// lbk8s_ds_train.hip — the deep-sets training side (lbk8s_ds_train.h) and its entry points: the
// backward and its weight-gradient reductions, the set gradients, the sums over sets, the
// backward weight pack, and the PPO and DQN loss heads.
//
// Public ABI: include/lbk8s.h; the host helpers: lbk8s_host.h.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "lbk8s.h"
#include "lbk8s_common.h"
#include "lbk8s_deepsets.h"
#include "lbk8s_ds_train.h"
#include "lbk8s_host.h"

using namespace lbk;

namespace {
// lb_ds_set_grads' jobs (returns their count)
int set_grad_params(const float* setvec, const float* dlogits, const float* dmean, int64_t num_sets,
                    int32_t num_elements, float* out, SetGradParams& p) {
    const int SV = LB_DS_SETVEC_FLOATS;
    p = SetGradParams{};
    p.S = num_sets;
    int nj = 0;
    auto job = [&](const float* a, int lda, int M, int amode, int alen, int boff, const float* b, int ldb, int N,
                   float scale, float* o) {
        p.job[nj++] = SetGradJob{a, lda, M, amode, alen, b ? b : setvec + boff, ldb, N, scale, o};
    };
    // actor: dGamma1 = -GS1A^T MAX0, dGamma2 = -GS2A^T MAX1A, dLambda3 = sum GA3,
    // dGamma3 = -(row sums of dlogits)^T MAX2A
    job(setvec + LB_DSV_GS1A, SV, 64, 0, 0, LB_DSV_MAX0, nullptr, SV, 8, -1.f, out);
    job(setvec + LB_DSV_GS2A, SV, 64, 0, 0, LB_DSV_MAX1A, nullptr, SV, 64, -1.f, out + 512);
    job(nullptr, 0, 1, 1, 0, LB_DSV_GA3, nullptr, SV, 64, 1.f, out + 4608);
    job(dlogits, num_elements, 1, 2, num_elements, LB_DSV_MAX2A, nullptr, SV, 64, -1.f, out + 4672);
    if (dmean) {  // critic: the same for psi, layer 3 from dmean (the mean's 1/R on Lambda3)
        float* c = out + LB_DS_SETGRAD_ACTOR;
        job(setvec + LB_DSV_GS1C, SV, 64, 0, 0, LB_DSV_MAX0, nullptr, SV, 8, -1.f, c);
        job(setvec + LB_DSV_GS2C, SV, 64, 0, 0, LB_DSV_MAX1C, nullptr, SV, 64, -1.f, c + 512);
        job(dmean, 64, 64, 0, 0, LB_DSV_CS2, nullptr, SV, 64, 1.f / (float)num_elements, c + 4608);
        job(dmean, 64, 64, 0, 0, LB_DSV_MAX2C, nullptr, SV, 64, -1.f, c + 8704);
    }
    static_assert(LB_DS_SETGRAD_ACTOR == 4736 && LB_DS_SETGRAD_CRITIC == 12800, "set-gradient layout");
    return nj;
}
// the training backward's launches (set_grads_out: lb_ds_train_backward_sets)
int train_backward(const float* bwd_frag, const float* obs, int64_t num_envs, int32_t num_elements,
                   const float* save_actor, const float* save_critic, const float* dlogits, const float* dmean,
                   float* wgrad_out, float* workspace, float* setvec, float* set_grads_out, void* stream) {
    static_assert(DSV_FLOATS == LB_DS_SETVEC_FLOATS, "per-set vector layout and header disagree");
    static_assert(DSW_FLOATS == LB_DS_WGRAD_FLOATS && DSW_SLOTS * 2 * DSW_FLOATS <= LB_DS_WORKSPACE_FLOATS,
                  "weight-gradient layout and header disagree");
    if (!bwd_frag || !obs || !setvec || !wgrad_out || !workspace || num_envs < 1)
        return fail("bwd_frag/obs/setvec/wgrad_out/workspace NULL or num_envs < 1");
    if (num_elements < 1 || num_elements > LB_DS_MAX_ELEMENTS_TRAIN)
        return fail("num_elements must be in [1, 257] (LB_DS_MAX_ELEMENTS_TRAIN)");
    const bool actor = dlogits != nullptr, critic = dmean != nullptr;
    if ((actor && !save_actor) || (critic && !save_critic)) return fail("a head's activation buffer is NULL");
    DSBwdParams p{obs, bwd_frag, save_actor, save_critic, dlogits, dmean, workspace, setvec,
                  num_envs, num_elements, actor, critic};
    // fixed grid: one workspace slot per block, so the reduction order never depends on B
    hipStream_t s = (hipStream_t)stream;
    // each head's backward (layer 1's pooled term in its slots too)
    if (actor) {
        hipLaunchKernelGGL(k_ds_train_bwd<0>, dim3(DSW_GRID), dim3(DSB_BLOCK), 0, s, p);
        if (int r = check_launch()) return r;
    }
    if (critic) {
        hipLaunchKernelGGL(k_ds_train_bwd<1>, dim3(DSW_GRID), dim3(DSB_BLOCK), 0, s, p);
        if (int r = check_launch()) return r;
    }
    static_assert(DSW_SLOTS % (2 * DSR_GROUPS) == 0, "reduction stride");
    if (set_grads_out) {
        SetGradParams sg;
        const int nj = set_grad_params(setvec, dlogits, dmean, num_envs, num_elements, set_grads_out, sg);
        hipLaunchKernelGGL(k_ds_wgrad_reduce_sets, dim3(DSR_BLOCKS + SG_TILES * nj), dim3(SG_THREADS), 0, s, workspace,
                           wgrad_out, (int)actor, (int)critic, sg);
        return check_launch();
    }
    hipLaunchKernelGGL(k_ds_wgrad_reduce, dim3(DSR_BLOCKS), dim3(DSR_COLS * DSR_GROUPS), 0, s, workspace, wgrad_out,
                       (int)actor, (int)critic);
    return check_launch();
}
}  // namespace

extern "C" {

int lb_dqn_head(const float* q, const float* q_next, const int64_t* actions, const float* rewards, const float* dones,
                int64_t num_sets, int32_t num_elements, float gamma, float* dq_out, float* sq_err_out, float* td_out,
                float* old_out, float* loss_out, void* stream) {
    if (!q || !q_next || !actions || !rewards || !dones || !dq_out || !sq_err_out || num_sets < 1)
        return fail("lb_dqn_head: NULL buffer or num_sets < 1");
    if (num_elements < 1 || num_elements > LB_DS_MAX_ELEMENTS_TRAIN) return fail("num_elements must be in [1, 257]");
    if (loss_out && num_sets > DQN_HEAD_BLOCK_MAX) return fail("lb_dqn_head: loss_out needs num_sets <= 1024");
    DQNHeadParams p{q, q_next, actions, rewards, dones, num_sets, num_elements, gamma, 2.0f / (float)num_sets, dq_out,
                    sq_err_out, td_out, old_out, loss_out};
    if (loss_out) {  // one block, one lane per sample, the mean in the same launch
        hipLaunchKernelGGL(k_dqn_head_block, dim3(1), dim3((unsigned)((num_sets + 63) / 64 * 64)), 0,
                           (hipStream_t)stream, p);
        return check_launch();
    }
    const unsigned grid = (unsigned)std::min<int64_t>((num_sets + 3) / 4, 65535);
    hipLaunchKernelGGL(k_dqn_head, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    return check_launch();
}

int lb_ppo_head(const float* logits, const uint8_t* masks, const float* actions, const float* oldlogp,
                const float* adv, const float* ret, const float* vold, const float* value, int64_t num_sets,
                int32_t num_elements, float clip_coef, float ent_coef, float vf_coef, int32_t clip_vloss,
                float* dlogits, float* dvalue, float* terms, void* stream) {
    if (!logits || !actions || !oldlogp || !adv || !ret || !vold || !value || !dlogits || !dvalue || !terms ||
        num_sets < 1)
        return fail("ppo head buffers NULL or num_sets < 1");
    if (num_elements < 1 || num_elements > LB_DS_MAX_ELEMENTS_TRAIN) return fail("num_elements must be in [1, 257]");
    PPOHeadParams p{logits, masks, actions, oldlogp, adv, ret, vold, value, dlogits, dvalue, terms,
                    num_sets, num_elements, clip_coef, ent_coef, vf_coef, 1.0f / (float)num_sets, clip_vloss};
    const unsigned grid = (unsigned)std::min<int64_t>((num_sets + 3) / 4, 8192);
    hipLaunchKernelGGL(k_ppo_head, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    return check_launch();
}

int lb_ds_pack_backward(const lb_ds_weights* w, float* bwd_frag_out, void* stream) {
    static_assert(DSB_FLOATS == LB_DS_BWD_FLOATS, "backward image layout and header disagree");
    if (!w || !bwd_frag_out) return fail("weights/bwd_frag_out NULL");
    if (!w->actor_lambda[1] || !w->actor_gamma[1] || !w->actor_lambda[2] || !w->actor_gamma[2])
        return fail("actor weights are required");
    hipLaunchKernelGGL(k_ds_pack_bwd, dim3((DSB_FLOATS + 255) / 256), dim3(256), 0, (hipStream_t)stream, *w,
                       bwd_frag_out);
    return check_launch();
}

int lb_ds_pack_pair(const lb_ds_weights* w, float* frag_out, float* bwd_frag_out, void* stream) {
    if (!w || !frag_out || !bwd_frag_out) return fail("weights/frag_out/bwd_frag_out NULL");
    for (int i = 0; i < 3; ++i)
        if (!w->actor_lambda[i] || !w->actor_gamma[i]) return fail("actor weights are required");
    hipLaunchKernelGGL(k_ds_pack_pair, dim3(DS_PACK_BLOCKS + DSB_PACK_BLOCKS), dim3(256), 0, (hipStream_t)stream, *w,
                       frag_out, bwd_frag_out);
    return check_launch();
}

int lb_ds_train_backward(const float* bwd_frag, const float* obs, int64_t num_envs, int32_t num_elements,
                         const float* save_actor, const float* save_critic, const float* dlogits, const float* dmean,
                         float* wgrad_out, float* workspace, float* setvec, void* stream) {
    return train_backward(bwd_frag, obs, num_envs, num_elements, save_actor, save_critic, dlogits, dmean, wgrad_out,
                          workspace, setvec, nullptr, stream);
}

int lb_ds_train_backward_sets(const float* bwd_frag, const float* obs, int64_t num_envs, int32_t num_elements,
                              const float* save_actor, const float* save_critic, const float* dlogits,
                              const float* dmean, float* wgrad_out, float* workspace, float* setvec,
                              float* set_grads_out, void* stream) {
    if (!set_grads_out || !dlogits) return fail("lb_ds_train_backward_sets: set_grads_out and dlogits are required");
    return train_backward(bwd_frag, obs, num_envs, num_elements, save_actor, save_critic, dlogits, dmean, wgrad_out,
                          workspace, setvec, set_grads_out, stream);
}

int lb_ds_over_sets(const lb_set_job* jobs, int32_t num_jobs, int64_t num_sets, float* workspace,
                    int64_t workspace_floats, void* stream) {
    if (!jobs || num_jobs < 1 || num_jobs > OS_JOBS || num_sets < 1 || !workspace)
        return fail("lb_ds_over_sets: jobs NULL, num_jobs not in [1, 16], num_sets < 1 or workspace NULL");
    OverSetsParams p{};
    int row = 0;
    auto vec_ok = [](const float* x, int64_t ld) { return ((uintptr_t)x & 15) == 0 && ld % 4 == 0; };
    for (int i = 0; i < num_jobs; ++i) {
        const lb_set_job& j = jobs[i];
        if (!j.b || !j.out || j.M < 1 || j.N < 1 || j.M > 64 || j.N > 64 || (!j.a && j.M != 1))
            return fail("lb_ds_over_sets: a job needs b and out, 1 <= M, N <= 64 (M == 1 when a is NULL)");
        p.job[i] = OverSetsJob{j.a, j.lda, j.b, j.ldb, j.M, j.N, j.scale, j.out, row,
                               (vec_ok(j.a, j.lda) ? 1 : 0) | (vec_ok(j.b, j.ldb) ? 2 : 0)};
        row += j.M * j.N;
    }
    p.njobs = num_jobs;
    p.row = row;
    p.S = num_sets;
    p.work = workspace;
    const int64_t spans = (num_sets + OS_SPAN - 1) / OS_SPAN;
    if (spans * row > workspace_floats) return fail("lb_ds_over_sets: workspace too small (spans x outputs)");
    if (spans > 65535) return fail("lb_ds_over_sets: num_sets too large");
    hipLaunchKernelGGL(k_ds_over_sets, dim3((unsigned)((num_jobs + 3) / 4), (unsigned)spans), dim3(256), 0,
                       (hipStream_t)stream, p);
    if (int r = check_launch()) return r;
    hipLaunchKernelGGL(k_ds_over_sets_reduce, dim3((unsigned)((row + 63) / 64)), dim3(64 * OS_RG), 0, (hipStream_t)stream, p,
                       (int)spans);
    return check_launch();
}

int lb_ds_set_grads(const float* setvec, const float* dlogits, const float* dmean, int64_t num_sets,
                    int32_t num_elements, float* out, void* stream) {
    if (!setvec || !dlogits || !out || num_sets < 1) return fail("setvec/dlogits/out NULL or num_sets < 1");
    if (num_elements < 1 || num_elements > LB_DS_MAX_ELEMENTS_TRAIN)
        return fail("num_elements must be in [1, 257] (LB_DS_MAX_ELEMENTS_TRAIN)");
    SetGradParams p;
    const int nj = set_grad_params(setvec, dlogits, dmean, num_sets, num_elements, out, p);
    hipLaunchKernelGGL(k_ds_set_grads, dim3(SG_TILES, nj), dim3(SG_THREADS), 0, (hipStream_t)stream, p);
    return check_launch();
}

}  // extern "C"

// the one-launch step kernels for envs of up to 64 endpoints and their entry points, compiled in
// this unit (the build's shortest; the set of units stays as it was: csrc/Makefile)
#include "lbk8s_steps64.hip"

// the one-launch greedy evaluation, DQN train period and PPO rollout for envs of up to 256 endpoints
// and their entry points, likewise
// (alone, this unit stays shorter with it than lbk8s_learn.hip would: DESIGN §1)
#include "lbk8s_steps256.hip"
