/*
 * lbk8s_abi_steps256.h -- C ABI of liblbk8s.so, ABI 17 additions: the one-launch greedy evaluation
 * for envs of up to 256 endpoints.  Included by lbk8s.h (inside its extern "C" block); not meant
 * to be included on its own.
 */
#ifndef LBK8S_ABI_STEPS256_H
#define LBK8S_ABI_STEPS256_H

/* ---- ABI 17, additions: lb_eval_steps for envs of up to 256 endpoints.
 * lb_eval_steps256 takes the arguments of lb_eval_steps and has the same effect, bit for bit
 * steps x (lb_ds_q_argmax, lb_step with obs updated in place, lb_ppo_record), on a superset of
 * lb_eval_steps64's shapes; the older names keep their meaning and their answers.
 * Supported (lb_eval_steps256_supported == 1; a property of the shape, never of the device):
 * wherever lb_eval_steps64_supported is 1; otherwise Philox mode, num_elements the env's action
 * count, num_envs in [1, 32767], the slice layout of 64 lanes with 2 or 4 endpoints per lane
 * (E = 65..256), num_elements <= 257.
 * On a shape lb_eval_steps64 supports the call runs that entry point (which hands on to
 * lb_eval_steps where that applies); elsewhere one wave carries one env through the steps, the
 * forward that of lb_ds_q_argmax at that num_elements (up to 80 rows held in registers, above
 * streamed in chunks of 32 rows).
 * Refused, before any device call: what lb_eval_steps refuses, under the new name; an
 * unsupported shape (there is no fallback: ask lb_eval_steps256_supported first). */
int lb_eval_steps256_supported(const lb_config* cfg, int64_t num_envs, int32_t num_elements);
int lb_eval_steps256(const float* frag, float* obs, void* state, const lb_config* cfg,
                     int64_t num_envs, int32_t num_elements, const uint8_t* masks, int32_t steps,
                     int32_t* actions_all, float* rewards_all, uint8_t* dones_all,
                     int32_t* actions_out, float* reward_out, uint8_t* done_out, double* ep_stats_out,
                     double* ep_sum, double* ep_cnt,
                     float* ret32, float* ep_r32, int64_t tag0, double* log, int64_t cap, uint32_t* count,
                     void* stream);

#endif /* LBK8S_ABI_STEPS256_H */
