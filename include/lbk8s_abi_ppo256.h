/*
 * lbk8s_abi_ppo256.h -- C ABI of liblbk8s.so, ABI 17 additions: the one-launch PPO rollout for envs
 * of up to 256 endpoints.  Included by lbk8s.h (inside its extern "C" block); not meant to be
 * included on its own.
 */
#ifndef LBK8S_ABI_PPO256_H
#define LBK8S_ABI_PPO256_H

/* ---- ABI 17, additions: lb_ppo_steps for envs of up to 256 endpoints.
 * lb_ppo_steps256 takes the arguments of lb_ppo_steps, argument for argument, and has the same
 * effect -- bit for bit `steps` times lb_ds_sample, lb_step and lb_ppo_record -- on a superset of
 * lb_ppo_steps64's shapes; the older names keep their meaning and their answers.
 * Supported (lb_ppo_steps256_supported == 1; a property of the shape, never of the device):
 * wherever lb_ppo_steps64_supported is 1; otherwise Philox mode, num_elements the env's action
 * count, num_envs in [1, 32767], the slice layout of 64 lanes with 2 or 4 endpoints per lane
 * (E = 65..256), num_elements <= 257 (the rule of lb_eval_steps256_supported).
 * On a shape lb_ppo_steps64 supports the call runs that entry point's kernel (or lb_ppo_steps'
 * where that applies); elsewhere one wave carries one env through the steps, the sampling forward
 * that of lb_ds_sample at that num_elements (up to 80 rows held in registers, above streamed in
 * chunks of 32 rows from the wave's LDS image; the critic's last layer and rho read their weights
 * from the image in global memory there).
 * Refused, before any device call and under this name: what lb_ppo_steps refuses (num_envs < 1;
 * steps outside [1, 4096]; store_rows neither steps nor steps - 1; a NULL among frag, obs, state,
 * uniforms, actions_f32, logprobs, values, rewards, actions_out, done_out, ep_stats_out; obs_next /
 * dones_next NULL with store_rows > 0; last_obs / last_done NULL with store_rows == steps - 1; one
 * of ep_sum / ep_cnt alone; a log without ret32, count or cap >= 0); an unsupported shape (there is
 * no fallback: ask lb_ppo_steps256_supported first). */
int lb_ppo_steps256_supported(const lb_config* cfg, int64_t num_envs, int32_t num_elements);
int lb_ppo_steps256(const float* frag, const float* obs, void* state, const lb_config* cfg,
                    int64_t num_envs, int32_t num_elements, int32_t steps, int32_t store_rows,
                    const float* uniforms, float* actions_f32, float* logprobs, float* values, float* rewards,
                    float* obs_next, float* dones_next, float* last_obs, float* last_done,
                    int32_t* actions_out, uint8_t* done_out, double* ep_stats_out,
                    double* ep_sum, double* ep_cnt,
                    float* ret32, float* ep_r32, int64_t tag0, double* log, int64_t cap, uint32_t* count,
                    void* stream);

/* ---- ABI 17, additions: lb_gae_tl, lb_ds_value_where, lb_ppo_steps_tl and its _supported query
 * (PPO value targets that bootstrap from the terminal state at a time limit) */
#include "lbk8s_abi_ppo_tl.h"

#endif /* LBK8S_ABI_PPO256_H */
