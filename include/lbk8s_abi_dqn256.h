/*
 * lbk8s_abi_dqn256.h -- C ABI of liblbk8s.so, ABI 17 additions: a DQN train period's vector steps in
 * one launch for envs of up to 256 endpoints.  Included by lbk8s.h (inside its extern "C" block);
 * not meant to be included on its own.
 */
#ifndef LBK8S_ABI_DQN256_H
#define LBK8S_ABI_DQN256_H

/* ---- ABI 17, additions: lb_dqn_steps for envs of up to 256 endpoints.
 * lb_dqn_steps256 takes the arguments of lb_dqn_steps, argument for argument, and has the same
 * effect -- bit for bit `steps` calls of lb_dqn_step, which at the new shapes are lb_dqn_act, lb_step
 * and lb_replay_add each -- on a superset of lb_dqn_steps64's shapes; the older names keep their
 * meaning and their answers.  steps in [1, 32]; sync (a device int32 that is 0, left 0) is required,
 * and with it pos_in / pos_out and the explore struct's vstep_in / vstep_out may each be one word.
 * Supported (lb_dqn_steps256_supported == 1; a property of the shape, never of the device):
 * wherever lb_dqn_steps64_supported is 1; otherwise Philox mode, num_elements the env's action
 * count, num_envs in [1, 32767], the slice layout of 64 lanes with 2 or 4 endpoints per lane
 * (E = 65..256), num_elements <= 257.
 * On a shape lb_dqn_steps64 supports the call runs that entry point's kernel (or lb_dqn_steps'
 * where that applies); elsewhere one wave carries one env through the steps, the greedy forward
 * that of lb_dqn_act / lb_ds_q_argmax at that num_elements (up to 80 rows held in registers, above
 * streamed in chunks of 32 rows).
 * Refused, before any device call and under this name: what lb_dqn_steps refuses (a NULL among
 * frag, obs, state, ex, actions_out, next_obs_out, reward_out, done_out, the explore struct's
 * words, the replay buffers, pos_in, pos_out; num_envs < 1; slots < 1; trace mode; num_elements not
 * the action count; one of ep_sum / ep_cnt alone or without ep_stats_out; steps outside [1, 32];
 * sync NULL); an unsupported shape (there is no fallback: ask lb_dqn_steps256_supported first). */
int lb_dqn_steps256_supported(const lb_config* cfg, int64_t num_envs, int32_t num_elements);
int lb_dqn_steps256(const float* frag, float* obs, int64_t num_envs, int32_t num_elements, const uint8_t* masks,
                    void* state, const lb_config* cfg, const lb_dqn_explore* ex, int32_t* actions_out,
                    float* next_obs_out, float* reward_out, uint8_t* done_out, float* terminal_obs_out,
                    double* ep_stats_out, int64_t slots, const int64_t* pos_in, int64_t* pos_out,
                    float* rb_obs, float* rb_next_obs, int64_t* rb_actions, float* rb_rewards, float* rb_dones,
                    double* ep_sum, double* ep_cnt, int32_t steps, int32_t* sync, void* stream);

#endif /* LBK8S_ABI_DQN256_H */
