/*
 * lbk8s_abi_steps64.h -- C ABI of liblbk8s.so, ABI 17 additions: the one-launch PPO rollout and greedy
 * evaluation for envs of up to 64 endpoints.  Included by lbk8s.h (inside its extern "C" block);
 * not meant to be included on its own.
 */
#ifndef LBK8S_ABI_STEPS64_H
#define LBK8S_ABI_STEPS64_H

/* ---- ABI 17, additions: lb_ppo_steps and lb_eval_steps for envs of up to 64 endpoints.
 * lb_ppo_steps64 / lb_eval_steps64 take the arguments of lb_ppo_steps / lb_eval_steps and have the
 * same effect, bit for bit the separate launches written out above, on a superset of their shapes;
 * the old names keep their meaning (the 16-lane subset) and their answers.
 * Supported (lb_ppo_steps64_supported == 1, the same answer as lb_eval_steps64_supported; a property
 * of the shape, never of the device; 1 wherever lb_ppo_steps_supported is 1): Philox mode,
 * num_elements the env's action count, num_envs in [1, 32767], the slice layout with one endpoint
 * per lane (below 32,768 envs: E <= 64, and not LB_GEOMETRY_TPE at E <= 8), num_elements <= 65; and
 * every shape of lb_ppo_steps_supported (E = 9..16 keeps 16 lanes per env at 32,768 envs and above).
 * On a shape lb_ppo_steps / lb_eval_steps supports the call runs that entry point's kernel;
 * elsewhere one wave carries one env (16, 32 or 64 lanes by E) through the steps, the forward that
 * of lb_ds_sample / lb_ds_q_argmax at that num_elements (config 4: E = 64, R = 65).
 * Refused: what lb_ppo_steps / lb_eval_steps refuses, under the new names; an unsupported shape
 * (there is no fallback: ask lb_ppo_steps64_supported / lb_eval_steps64_supported first). */
int lb_ppo_steps64_supported(const lb_config* cfg, int64_t num_envs, int32_t num_elements);
int lb_ppo_steps64(const float* frag, const float* obs, void* state, const lb_config* cfg,
                   int64_t num_envs, int32_t num_elements, int32_t steps, int32_t store_rows,
                   const float* uniforms, float* actions_f32, float* logprobs, float* values, float* rewards,
                   float* obs_next, float* dones_next, float* last_obs, float* last_done,
                   int32_t* actions_out, uint8_t* done_out, double* ep_stats_out,
                   double* ep_sum, double* ep_cnt,
                   float* ret32, float* ep_r32, int64_t tag0, double* log, int64_t cap, uint32_t* count,
                   void* stream);
int lb_eval_steps64_supported(const lb_config* cfg, int64_t num_envs, int32_t num_elements);
int lb_eval_steps64(const float* frag, float* obs, void* state, const lb_config* cfg,
                    int64_t num_envs, int32_t num_elements, const uint8_t* masks, int32_t steps,
                    int32_t* actions_all, float* rewards_all, uint8_t* dones_all,
                    int32_t* actions_out, float* reward_out, uint8_t* done_out, double* ep_stats_out,
                    double* ep_sum, double* ep_cnt,
                    float* ret32, float* ep_r32, int64_t tag0, double* log, int64_t cap, uint32_t* count,
                    void* stream);

#endif /* LBK8S_ABI_STEPS64_H */
