// lbk8s_ds_chunked.h — the chunked deep-sets forward of large sets (LB_DS_MAX_ELEMENTS < R <=
// LB_DS_MAX_ELEMENTS_FWD): ds_chunked_set<MODE, Rows>, the forward of ONE set by one wave, and
// k_deepsets_fwd_big<MODE>, the kernel around it.  Part of lbk8s_deepsets.h, which includes it
// after the tiled forwards (eq_layer, row_reduce, row_scan, mfma4 .. are theirs): include that.
//
// One set per wave; the set is streamed in chunks of DS_CT 16-row tiles (32 elements).  A layer
// needs the set-wise max of its input, so each layer's max is one pass over the chunks that
// recomputes the earlier layers of the chunk: nothing per element leaves registers, at the
// price of layer 1 three times and layer 2 twice for the actor (R up to 257: E <= 256 with
// the reject row).  Same fragments, same per-element math as k_deepsets_fwd.
//
// ds_chunked_set has two parameters beside the mode, and three callers:
//   Rows     where a chunk's observation rows are read: DSRowsGlobal (the [R][8] rows of the set in
//            global memory: k_deepsets_fwd_big) or DSRowsLds (a wave's LDS observation image:
//            k_eval_steps256 / k_dqn_steps256 through eval_steps_wide and the kernel, MODE 2, and
//            k_ppo_steps256, MODE 5).  Its trait HEADS_FROM_PARAMS says whether p.actor / p.critic /
//            p.logits choose the outputs at run time or the mode fixes them (the step kernels).
//   W, We    the fragment image the chunk loops read (below DS_C3L) and the one the critic's
//            epilogue reads from DS_C3L on (layer 3 on the set's mean and max, rho: whole 64-float
//            rows, once per set).  k_deepsets_fwd_big passes its LDS image twice; k_ppo_steps256,
//            whose LDS holds the fragments below DS_C3L only, passes it and the image in global
//            memory: the same values in the same operations.
// So the bits of lb_eval_steps256 / lb_dqn_steps256 / lb_ppo_steps256 at R > 80 are those of
// lb_ds_q_argmax / lb_ds_sample by construction.
#pragma once

namespace lbk {

constexpr int DS_CT = 2;

template <int KS>
__device__ __forceinline__ void chunk_max_acc(const float (&h)[DS_CT][KS], float (&acc)[KS], int row0, int col, int R) {
#pragma unroll
    for (int t = 0; t < DS_CT; ++t)
        if (row0 + 16 * t + col < R)
#pragma unroll
            for (int k = 0; k < KS; ++k) acc[k] = max2(acc[k], h[t][k]);
}

// a chunk's observation rows (A-fragment layout, 0 past R) from the set's [R][8] rows at x ...
template <class Ptr>
__device__ __forceinline__ void load_obs_chunk(Ptr x, int row0, int R, int col, int grp, float (&h0)[DS_CT][2]) {
#pragma unroll
    for (int t = 0; t < DS_CT; ++t) {
        const int row = row0 + 16 * t + col;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) h0[t][kk] = row < R ? x[row * 8 + 4 * kk + grp] : 0.f;
    }
}
// ... in global memory, or in an LDS image of them: the same words, read by ds_reads through the
// address-space-3 pointer (a generic pointer to LDS compiles to flat loads)
struct DSRowsGlobal {
    static constexpr bool HEADS_FROM_PARAMS = true;  // (the entry points' callers choose the outputs)
    const float* x;
    __device__ __forceinline__ void load(int row0, int R, int col, int grp, float (&h0)[DS_CT][2]) const {
        load_obs_chunk(x, row0, R, col, grp, h0);
    }
};
typedef __attribute__((address_space(3))) const float lds_cfloat;
struct DSRowsLds {
    static constexpr bool HEADS_FROM_PARAMS = false;  // (the step kernels: the mode fixes the heads)
    const float4* img;
    __device__ __forceinline__ void load(int row0, int R, int col, int grp, float (&h0)[DS_CT][2]) const {
        load_obs_chunk((lds_cfloat*)(img), row0, R, col, grp, h0);
    }
};

// training (chunked): each lane's running max of its rows per feature and the FIRST row
// attaining it (strict > over ascending rows)
template <int KS>
__device__ __forceinline__ void chunk_argmax_acc(const float (&h)[DS_CT][KS], float (&v)[KS], float (&r)[KS], int row0,
                                                 int col, int R) {
#pragma unroll
    for (int t = 0; t < DS_CT; ++t) {
        const int row = row0 + 16 * t + col;
        if (row >= R) continue;
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            const bool u = h[t][k] > v[k];
            v[k] = u ? h[t][k] : v[k];
            r[k] = u ? (float)row : r[k];
        }
    }
}
// ... then the set's max over the 16 columns (into v, every lane) and the smallest row among
// the lanes holding it, both to setvec (feature 16q + 4grp + i of the accumulator layout)
__device__ __forceinline__ void chunk_argmax_store(float (&v)[16], float (&r)[16], int col, int grp, float* sv,
                                                   int off_max, int off_id) {
    float M[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) M[k] = v[k];
    row_reduce<true>(M);
#pragma unroll
    for (int k = 0; k < 16; ++k) r[k] = v[k] == M[k] ? -r[k] : -1e9f;
    row_reduce<true>(r);
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = M[k];
    if (col != 0) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int f0 = 16 * q + 4 * grp;
        *reinterpret_cast<float4*>(sv + off_max + f0) = make_float4(M[4 * q], M[4 * q + 1], M[4 * q + 2], M[4 * q + 3]);
        *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(sv + off_id) + f0) =
            make_uint2((uint32_t)(-r[4 * q]) | ((uint32_t)(-r[4 * q + 1]) << 16),
                       (uint32_t)(-r[4 * q + 2]) | ((uint32_t)(-r[4 * q + 3]) << 16));
    }
}
// a chunk's layer output rows (accumulator layout) into plane [B][R][64]
__device__ __forceinline__ void store_rows_chunk(float* plane, const float (&h)[DS_CT][16], int64_t env, int R, int row0,
                                                 int col, int grp) {
#pragma unroll
    for (int t = 0; t < DS_CT; ++t) {
        const int row = row0 + 16 * t + col;
        if (row >= R) continue;
        float* q = plane + (env * (int64_t)R + row) * 64 + 4 * grp;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) ds_stream(q + 16 * nt, h[t][4 * nt], h[t][4 * nt + 1], h[t][4 * nt + 2], h[t][4 * nt + 3]);
    }
}

// sample mode of the chunked forward (ds_sample_group's definition): lg[j] is the masked logit
// of row 64 j + lane (-inf past R).  The scan of a slot is row_scan over each 16-lane row, plus
// the totals of the rows before it and of the slots before it; the lane holding the action's
// row writes the set's outputs.  Every lane returns the action (k_ppo_steps256 steps the env with it).
constexpr int DS_SLOTS = (LB_DS_MAX_ELEMENTS_FWD + 63) / 64;
__device__ __forceinline__ float ds_wave_max(float v) {
    float a[1] = {v};
    row_reduce<true>(a);
    a[0] = max2(a[0], __shfl_xor(a[0], 16));
    return max2(a[0], __shfl_xor(a[0], 32));
}
__device__ __forceinline__ int32_t ds_sample_wave(const DSParams& p, const float (&lg)[DS_SLOTS], int64_t env, int lane) {
    const int grp = lane >> 4;
    float m = lg[0];
#pragma unroll
    for (int j = 1; j < DS_SLOTS; ++j) m = max2(m, lg[j]);
    m = ds_wave_max(m);
    float e[DS_SLOTS], c[DS_SLOTS], run = 0.f;
#pragma unroll
    for (int j = 0; j < DS_SLOTS; ++j) {
        e[j] = __builtin_amdgcn_exp2f((lg[j] - m) * DS_LOG2E);
        const float sc = row_scan(e[j]);
        const float t0 = ds_read_lane(sc, 15), t1 = ds_read_lane(sc, 31), t2 = ds_read_lane(sc, 47),
                    t3 = ds_read_lane(sc, 63);
        const float before = grp == 0 ? 0.f : (grp == 1 ? t0 : (grp == 2 ? t0 + t1 : (t0 + t1) + t2));
        c[j] = run + (before + sc);
        run = run + (((t0 + t1) + t2) + t3);
    }
    const float thr = p.uniforms[env] * run;
    float first = 1e9f, last = -1.f;
#pragma unroll
    for (int j = DS_SLOTS - 1; j >= 0; --j) {
        const float row = (float)(64 * j + lane);
        if (e[j] > 0.f && c[j] >= thr) first = row;
        if (e[j] > 0.f && last < 0.f) last = row;
    }
    const float f = -ds_wave_max(-first), l = ds_wave_max(last);
    const int a = f < 1e8f ? (int)f : (int)l;
    if (lane != (a & 63)) return a;
    float la = lg[0];
#pragma unroll
    for (int j = 1; j < DS_SLOTS; ++j) la = (a >> 6) == j ? lg[j] : la;
    p.actions[env] = a;
    if (p.actions_f32) p.actions_f32[env] = (float)a;
    p.logprob[env] = (la - m) - logf(run);
    return a;
}

// The forward of set env (R rows, read through rows) by one wave; W / We: see the head of the file.
// MODE 0: logits / value; 1: training forward (activations, set maxima + first argmax rows,
// psi mean; as k_deepsets_fwd<.., 1>); 2: Q values and the masked greedy action (actor only);
// 5: MODE 0 and the sampled action with its log-probability (ds_sample_wave); 6 (DS_FWD_WHERE,
// k_deepsets_fwd_big skips the unflagged sets): MODE 0.
// Rows::HEADS_FROM_PARAMS: p.actor / p.critic / p.logits choose the heads and the logits row at run
// time, as in the tiled forwards; the step kernels' sets (DSRowsLds) run the actor, the critic with
// the draw (MODE 5: PPO) and write no logits row, whatever p says, so their code holds no such test
// (measured: lb_dqn_steps256 at 256 envs of 256 endpoints).  Returns the action: MODE 2 to the lanes of row group 0 (lane 0 writes p.actions[env]),
// MODE 5 to every lane (the lane of the action's row writes the set's outputs); 0 otherwise.
template <int MODE, class Rows>
__device__ __forceinline__ int32_t ds_chunked_set(const DSParams& p, const float* W, const float* We, const Rows& rows,
                                                  int64_t env, int lane, int R) {
    constexpr bool ARGMAX = MODE == 2, TRAIN = MODE == 1, SAMPLE = MODE == LB_DS_FWD_SAMPLE;
    const int col = lane & 15, grp = lane >> 4;
    const int nch = (R + 16 * DS_CT - 1) / (16 * DS_CT);
    constexpr bool PF = Rows::HEADS_FROM_PARAMS;
    const bool actor = PF ? p.actor != 0 : true, critic = PF ? p.critic != 0 : SAMPLE;
    float* const logits = PF ? p.logits : nullptr;
    int32_t act = 0;
    // the weight fragments are re-read from LDS in every chunk: an opaque base pointer
    // per chunk keeps the compiler from hoisting KiBs of loop-invariant loads into
    // registers (which spilled to scratch)
    // (an opaque 32-bit offset into the shared array keeps the loads ds_reads)
    float h0[DS_CT][2], h1[DS_CT][16], h2[DS_CT][16];
    float m0[2] = {-INFINITY, -INFINITY};
    for (int c = 0; c < nch; ++c) {
        rows.load(16 * DS_CT * c, R, col, grp, h0);
        chunk_max_acc<2>(h0, m0, 16 * DS_CT * c, col, R);
    }
    row_reduce<true>(m0);
    float* sv = TRAIN ? p.setvec + env * (int64_t)LB_DS_SETVEC_FLOATS : nullptr;
    if (TRAIN && col == 0) {
        sv[LB_DSV_MAX0 + grp] = m0[0];
        sv[LB_DSV_MAX0 + 4 + grp] = m0[1];
    }
    if (actor) {
        float m1[16], m2[16], r1[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            m1[k] = m2[k] = -INFINITY;
            r1[k] = 1e9f;
        }
        for (int c = 0; c < nch; ++c) {
            uint32_t wo = 0;
            asm volatile("" : "+s"(wo));
            const float* Wc = W + wo;
            rows.load(16 * DS_CT * c, R, col, grp, h0);
            eq_layer<DS_CT, 1, 2, 1>(Wc + DS_A1L, Wc + DS_A1G, h0, m0, h1, lane);
            if (TRAIN) chunk_argmax_acc<16>(h1, m1, r1, 16 * DS_CT * c, col, R);
            else chunk_max_acc<16>(h1, m1, 16 * DS_CT * c, col, R);
        }
        if (TRAIN) chunk_argmax_store(m1, r1, col, grp, sv, LB_DSV_MAX1A, LB_DSV_ID1A);
        else row_reduce<true>(m1);
#pragma unroll
        for (int k = 0; k < 16; ++k) r1[k] = 1e9f;
        for (int c = 0; c < nch; ++c) {
            uint32_t wo = 0;
            asm volatile("" : "+s"(wo));
            const float* Wc = W + wo;
            rows.load(16 * DS_CT * c, R, col, grp, h0);
            eq_layer<DS_CT, 1, 2, 1>(Wc + DS_A1L, Wc + DS_A1G, h0, m0, h1, lane);
            eq_layer<DS_CT, 1, 16, 2>(Wc + DS_A2L, Wc + DS_A2G, h1, m1, h2, lane);
            if (TRAIN) chunk_argmax_acc<16>(h2, m2, r1, 16 * DS_CT * c, col, R);
            else chunk_max_acc<16>(h2, m2, 16 * DS_CT * c, col, R);
        }
        if (TRAIN) chunk_argmax_store(m2, r1, col, grp, sv, LB_DSV_MAX2A, LB_DSV_ID2A);
        else row_reduce<true>(m2);
        const float* G = W + DS_A3G + 16 * grp;
        float gl = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) gl += G[k * 64] * m2[k];
        gl += __shfl_xor(gl, 16);
        gl += __shfl_xor(gl, 32);
        float best = -INFINITY, brow = 1e9f;
        // sample mode: the set's masked logits stay in registers for the draw, lane l keeps
        // rows l, 64 + l, .. (row 32 c + 16 t + col is lane (col, 2 (c & 1) + t)'s slot c >> 1)
        float lgr[DS_SLOTS];
#pragma unroll
        for (int j = 0; j < DS_SLOTS; ++j) lgr[j] = -INFINITY;
        for (int c = 0; c < nch; ++c) {
            uint32_t wo = 0;
            asm volatile("" : "+s"(wo));
            const float* Wc = W + wo;
            rows.load(16 * DS_CT * c, R, col, grp, h0);
            eq_layer<DS_CT, 1, 2, 1>(Wc + DS_A1L, Wc + DS_A1G, h0, m0, h1, lane);
            eq_layer<DS_CT, 1, 16, 2>(Wc + DS_A2L, Wc + DS_A2G, h1, m1, h2, lane);
            if (TRAIN) {
                store_rows_chunk(p.save_actor, h1, env, R, 16 * DS_CT * c, col, grp);
                store_rows_chunk(p.save_actor + p.B * (int64_t)R * 64, h2, env, R, 16 * DS_CT * c, col, grp);
            }
#pragma unroll
            for (int t = 0; t < DS_CT; ++t) {
                float v = 0.f;
#pragma unroll
                for (int k = 0; k < 16; ++k) v += Wc[DS_A3L + 16 * grp + k * 64] * h2[t][k];
                v += __shfl_xor(v, 16);
                v += __shfl_xor(v, 32);
                const int row = 16 * DS_CT * c + 16 * t + col;
                if (row >= R) continue;
                if (grp == 0 && logits) logits[env * R + row] = gl + v;
                if (SAMPLE && grp == 2 * (c & 1) + t) {
                    const float q = (!p.masks || p.masks[env * R + row]) ? gl + v : -1e8f;
#pragma unroll
                    for (int j = 0; j < DS_SLOTS; ++j) lgr[j] = j == (c >> 1) ? q : lgr[j];
                }
                if (ARGMAX) {
                    const float q = (!p.masks || p.masks[env * R + row]) ? gl + v : -1e8f;
                    if (q > best) {  // rows ascend: the first maximum of this lane wins
                        best = q;
                        brow = (float)row;
                    }
                }
            }
        }
        if (ARGMAX) {
            float m[1] = {best};
            row_reduce<true>(m);
            float cc[1] = {best == m[0] ? -brow : -1e9f};
            row_reduce<true>(cc);
            act = (int32_t)(-cc[0]);
            if (lane == 0) p.actions[env] = act;
        }
        if (SAMPLE) act = ds_sample_wave(p, lgr, env, lane);
    }
    if (ARGMAX || !critic) return act;
    // critic: the max of c1, then the max and the sum of c2, then layer 3 / rho as above
    float mc1[16], mc2[16], sm[16], rc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        mc1[k] = mc2[k] = -INFINITY;
        sm[k] = 0.f;
        rc[k] = 1e9f;
    }
    for (int c = 0; c < nch; ++c) {
        uint32_t wo = 0;
        asm volatile("" : "+s"(wo));
        const float* Wc = W + wo;
        rows.load(16 * DS_CT * c, R, col, grp, h0);
        eq_layer<DS_CT, 1, 2, 2>(Wc + DS_C1L, Wc + DS_C1G, h0, m0, h1, lane);
        if (TRAIN) chunk_argmax_acc<16>(h1, mc1, rc, 16 * DS_CT * c, col, R);
        else chunk_max_acc<16>(h1, mc1, 16 * DS_CT * c, col, R);
    }
    if (TRAIN) chunk_argmax_store(mc1, rc, col, grp, sv, LB_DSV_MAX1C, LB_DSV_ID1C);
    else row_reduce<true>(mc1);
#pragma unroll
    for (int k = 0; k < 16; ++k) rc[k] = 1e9f;
    for (int c = 0; c < nch; ++c) {
        uint32_t wo = 0;
        asm volatile("" : "+s"(wo));
        const float* Wc = W + wo;
        rows.load(16 * DS_CT * c, R, col, grp, h0);
        eq_layer<DS_CT, 1, 2, 2>(Wc + DS_C1L, Wc + DS_C1G, h0, m0, h1, lane);
        eq_layer<DS_CT, 1, 16, 2>(Wc + DS_C2L, Wc + DS_C2G, h1, mc1, h2, lane);
        if (TRAIN) {
            chunk_argmax_acc<16>(h2, mc2, rc, 16 * DS_CT * c, col, R);
            store_rows_chunk(p.save_critic, h1, env, R, 16 * DS_CT * c, col, grp);
            store_rows_chunk(p.save_critic + p.B * (int64_t)R * 64, h2, env, R, 16 * DS_CT * c, col, grp);
        } else {
            chunk_max_acc<16>(h2, mc2, 16 * DS_CT * c, col, R);
        }
#pragma unroll
        for (int t = 0; t < DS_CT; ++t)
            if (16 * DS_CT * c + 16 * t + col < R)
#pragma unroll
                for (int k = 0; k < 16; ++k) sm[k] += h2[t][k];
    }
    if (TRAIN) chunk_argmax_store(mc2, rc, col, grp, sv, LB_DSV_MAX2C, LB_DSV_ID2C);
    else row_reduce<true>(mc2);
    row_reduce<false>(sm);
    // (from here on the fragments are We's: whole rows of 64 lanes)
    const float invR = 1.0f / (float)R;
    float mean[16];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        dsf4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 16; ++k) acc = mfma4(We[DS_C3G + (nt * 16 + k) * 64 + lane], mc2[k], acc);
#pragma unroll
        for (int k = 0; k < 16; ++k) acc = mfma4(We[DS_C3L + (nt * 16 + k) * 64 + lane], sm[k] * invR, acc);
#pragma unroll
        for (int i = 0; i < 4; ++i) mean[4 * nt + i] = acc[i];
    }
    if (TRAIN) {  // psi mean (rho runs in torch): every column holds the set's value
        if (col == 0) {
            float* q = p.psi_mean + env * 64 + 4 * grp;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
                *reinterpret_cast<float4*>(q + 16 * nt) =
                    make_float4(mean[4 * nt], mean[4 * nt + 1], mean[4 * nt + 2], mean[4 * nt + 3]);
        }
        return act;
    }
    float r1[16];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        dsf4 acc;
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = We[DS_R1B + 16 * nt + 4 * grp + i];
#pragma unroll
        for (int k = 0; k < 16; ++k) acc = mfma4(We[DS_R1W + (nt * 16 + k) * 64 + lane], mean[k], acc);
#pragma unroll
        for (int i = 0; i < 4; ++i) r1[4 * nt + i] = act_elu(acc[i]);
    }
    dsf4 v = {We[DS_R2B], 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 16; ++k) v = mfma4(We[DS_R2W + k * 64 + lane], r1[k], v);
    if (lane == 0) p.value[env] = v[0];
    return act;
}

// lb_ds_forward / lb_ds_forward_train / lb_ds_q_argmax / lb_ds_sample at R > LB_DS_MAX_ELEMENTS:
// ds_chunked_set<MODE> of every set, the rows read from p.obs, the whole image (the actor's part
// where no critic runs) staged in LDS
template <int MODE>
__global__ __launch_bounds__(DS_BLOCK, 2) void k_deepsets_fwd_big(DSParams p) {
    constexpr bool ARGMAX = MODE == 2;
    if (ARGMAX && p.ex_on && ds_dqn_explore(p)) return;
    if constexpr (MODE == DS_FWD_WHERE) {  // (as ds_fwd_body: the zeros, and no staging without a flagged set)
        int any = 0;
        for (int64_t env = (int64_t)blockIdx.x * (DS_BLOCK / 64) + (threadIdx.x >> 6); env < p.B;
             env += (int64_t)gridDim.x * (DS_BLOCK / 64)) {
            if (threadIdx.x & 63) continue;
            const int f = p.masks[env] != 0;
            if (!f) p.value[env] = 0.f;
            any |= f;
        }
        if (!__syncthreads_or(any)) return;
    }
    __shared__ __attribute__((aligned(16))) float W[DS_LDS_FLOATS];
    const int nstage = (ARGMAX || !p.critic) ? DS_C1L : DS_FLOATS;
    for (int i = threadIdx.x * 4; i < nstage; i += DS_BLOCK * 4)
        *reinterpret_cast<float4*>(W + i) = *reinterpret_cast<const float4*>(p.wfrag + i);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (DS_BLOCK / 64) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (DS_BLOCK / 64);
    const int R = p.R;
    for (int64_t env = wave; env < p.B; env += nwaves) {
        if constexpr (MODE == DS_FWD_WHERE)  // (wave-uniform: an unflagged set does no forward work)
            if (!__builtin_amdgcn_readfirstlane((int)p.masks[env])) continue;
        ds_chunked_set<MODE>(p, W, W, DSRowsGlobal{p.obs + env * (int64_t)R * 8}, env, lane, R);
    }
}

}  // namespace lbk
