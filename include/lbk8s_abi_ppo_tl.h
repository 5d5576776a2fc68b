/*
 * lbk8s_abi_ppo_tl.h -- C ABI of liblbk8s.so, ABI 17 additions: PPO value targets that bootstrap
 * from the terminal state at a time limit.  Included by lbk8s.h (through lbk8s_abi_ppo256.h, inside
 * the extern "C" block); not meant to be included on its own.
 */
#ifndef LBK8S_ABI_PPO_TL_H
#define LBK8S_ABI_PPO_TL_H

/* ---- ABI 17, additions: partial-episode bootstrapping for PPO.
 * Every episode of this env ends at its time limit (current_step == episode_length), a truncation,
 * and the observation holds no step index.  The reference's GAE treats `done` as a true terminal
 * and drops the bootstrap term there; lb_gae keeps that.  The three calls below are the option:
 * at a `done` the TD error bootstraps from the critic's value of the episode's terminal
 * observation, and the lambda-chain is still cut there.  With a rollout of T steps over B envs the
 * option's one storage array is term_values [T][B] f32: term_values[t][b] = V(terminal observation
 * of env b) if env b's episode ended in step t, else +0.0f. */

/* lb_gae_tl: lb_gae with the time-limit bootstrap, one launch, one thread per env.  The arguments
 * of lb_gae plus term_values [T][B]; the same conventions (f32, op for op, no contraction,
 * g = (float)gamma, gl = (float)(gamma * gae_lambda) with the product in double, 64-bit indexing,
 * no LDS, no atomics, capturable).  For t = T-1 .. 0, last = 0 before t = T-1:
 *   nd    = t == T-1 ? next_done[b]  : dones[t+1][b]
 *   nv    = t == T-1 ? next_value[b] : values[t+1][b]
 *   bv    = nd != 0.f ? term_values[t][b] : nv
 *   nnt   = 1 - nd
 *   delta = (rewards[t][b] + g * bv) - values[t][b]
 *   last  = delta + (gl * nnt) * last
 *   advantages_out[t][b] = last,  returns_out[t][b] = last + values[t][b]
 * For finite inputs the outputs are lb_gae's bit for bit when term_values is all zero, and when no
 * done is set anywhere, whatever term_values holds.
 * Refused: what lb_gae refuses; term_values NULL or equal to an output. */
int lb_gae_tl(const float* rewards, const float* values, const float* dones,
              const float* next_value, const float* next_done, const float* term_values,
              int64_t num_steps, int64_t num_envs, double gamma, double gae_lambda,
              float* advantages_out, float* returns_out, void* stream);

/* lb_ds_value_where: the critic's forward on the flagged sets only.  value_out[b] for
 * flags[b] != 0 is bit for bit what lb_ds_forward(frag, obs, num_envs, num_elements, NULL,
 * value_out) writes for set b (the same kernel variant, chosen by the same rule at the same
 * (num_envs, num_elements); every num_elements in [1, LB_DS_MAX_ELEMENTS_FWD]); for flags[b] == 0
 * it is +0.0f and that set's observation rows are not read (NaN or stale memory there has no
 * effect: lb_step leaves the terminal_obs rows of unfinished envs untouched).  A wave whose sets are
 * all unflagged does no forward work, and a block none of whose sets is flagged does not stage the
 * weights: the call then costs a launch and a flag read.  The actor is never evaluated.
 * flags [num_envs] u8.  No host synchronisation, no allocation, no atomics; capturable.
 * Refused, before any device call: num_envs < 1; a NULL pointer; num_elements outside
 * [1, LB_DS_MAX_ELEMENTS_FWD]. */
int lb_ds_value_where(const float* frag, const float* obs, const uint8_t* flags,
                      int64_t num_envs, int32_t num_elements, float* value_out, void* stream);

/* lb_ppo_steps_tl: lb_ppo_steps with the terminal values.  The arguments of lb_ppo_steps, then
 * terminal_obs [B][R][8] and term_values [steps][B].  Supported exactly where
 * lb_ppo_steps_supported is 1 (lb_ppo_steps_tl_supported gives that answer).  The call has, bit for
 * bit, the effect of lb_ppo_steps' per-step sequence with two changes: lb_step gets terminal_obs in
 * place of NULL, and after lb_ppo_record of step i follows
 *   lb_ds_value_where(frag, terminal_obs, done_out, num_envs, num_elements, term_values + i B).
 * At the end terminal_obs holds every env's last terminal observation (untouched for an env that
 * never finished); every other output is lb_ppo_steps'.
 * Refused, before any device call and under this name: what lb_ppo_steps refuses; terminal_obs or
 * term_values NULL. */
int lb_ppo_steps_tl_supported(const lb_config* cfg, int64_t num_envs, int32_t num_elements);
int lb_ppo_steps_tl(const float* frag, const float* obs, void* state, const lb_config* cfg,
                    int64_t num_envs, int32_t num_elements, int32_t steps, int32_t store_rows,
                    const float* uniforms, float* actions_f32, float* logprobs, float* values, float* rewards,
                    float* obs_next, float* dones_next, float* last_obs, float* last_done,
                    int32_t* actions_out, uint8_t* done_out, double* ep_stats_out,
                    double* ep_sum, double* ep_cnt,
                    float* ret32, float* ep_r32, int64_t tag0, double* log, int64_t cap, uint32_t* count,
                    float* terminal_obs, float* term_values, void* stream);

#endif /* LBK8S_ABI_PPO_TL_H */
