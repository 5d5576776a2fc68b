"""k_ppo_steps256 (csrc/lbk8s_ppo256.h: lb_ppo_steps256, a PPO rollout's vector steps in one launch
for envs of 65 to 256 endpoints) pinned to the C oracle and the float64 definition of the draw,
independently of the three launches tests/test_gpu_ppo_steps256.py compares it with, through
LBVecEnv.ppo_steps256 (tests/test_gpu_ppo_oracle.py: the C ABI, with the episode log).

One launch of 6 steps on 8 envs with 2-step episodes (every env ends inside the launch and goes on
from its restart), at the first row count of each kernel instance and the largest: R = 66
(<2, false>), 81 (<2, true>), 129 and 257 (<4, true>: E = 129 .. 256 have four endpoints per lane;
129 rows with the reject row on E = 128 is <2, true>'s last).  The envs start from a plain reset,
every row is stored (store_rows = steps, last_obs / last_done None) and the env has no monitor, so
there is no log.  tests/ppo_ref.PPOChecker then checks:

  * the env: oracle.OracleBatch follows the launch's own actions; every step's reward, done flag
    and next observations equal the oracle's bit for bit;
  * the draw: for every stored row, lb_ds_forward's logits and value of that row's input
    observation (the plain forward, another kernel), with the row's uniform, action,
    log-probability and value, go through tests/ds_sample_ref.check_sample -- the logits and the
    value near the float64 network (ds_ref.near), the row's value equal to the plain forward's bit
    for bit, the action inside its inverse-CDF interval under the float64 softmax, the
    log-probability within the checker's bound.  Tolerances are the checker's, unchanged; no row is
    exempt;
  * the rest of what the launch wrote: actions / dones as the last step leaves them, the
    lb_reward64 array, the env's ep_stats rows, ep_sum / ep_cnt from non-zero starting values, the
    guard elements of every buffer, ret32 / ep_r32 / log / count untouched, stats(), the state
    fields and status().

(These seeds' agents leave the reject row, the last, less probability than the draw's tolerance,
so finish() is not asked for an action on it here; tests/test_gpu_ppo_oracle.py's seed has one.)
"""
import numpy as np
import pytest
import torch

import ds_sample_ref as sr
import ppo_ref
from ppo_ref import PPOChecker
from test_gpu_ppo_oracle import HipDevice

pytestmark = pytest.mark.gpu

B, STEPS, L = 8, 6, 2
# R: (E, reject, weight seed)
CASES = {66: (65, True, 3), 81: (80, True, 5), 129: (128, True, 7), 257: (256, True, 11)}


class WrapperDevice(HipDevice):
    """One launch through LBVecEnv.ppo_steps256 on views of the same buffers; ep_stats are the env's."""

    def run(self, n, store_rows, tag0):
        b, B_, R = self.b, self.B, self.R
        assert self.t == 0 and store_rows == n == b.steps and not self.with_log
        v = lambda k, *shape: getattr(b, k)[:b.n[k]].view(*shape)
        self.env.ppo_steps256(self.frag, self.env.obs.clone(), self.u, v("actions_f32", n, B_), v("logprobs", n, B_),
                              v("values", n, B_), v("rewards", n, B_), v("obs_next", n, B_, R, 8),
                              v("dones_next", n, B_), None, None, v("actions_out", B_), v("done_out", B_), v("ep_sum", B_), v("ep_cnt", B_))
        self.t += n

    def read(self):
        out = super().read()
        rows = self.env.ep_stats.cpu().numpy().reshape(-1)
        out["ep_stats"] = np.concatenate([rows, out["ep_stats"][rows.size:]])
        return out


@pytest.mark.parametrize("R", sorted(CASES))
def test_ppo_steps256_equals_oracle_and_float64_draw(oracle_mod, R):
    E, rej, wseed = CASES[R]
    kw = dict(num_endpoints=E, rejection_allowed=rej, reward_function="multi", episode_length=L)
    plan = [(STEPS, STEPS)]
    u = torch.rand((STEPS, B), generator=torch.Generator().manual_seed(R))
    u[0, 0], u[0, 1] = 0.0, sr.U_ONE
    agent = ppo_ref.make_agent(wseed)
    dev = WrapperDevice("lb_ppo_steps256", kw, B, 5, agent, plan, u, 1, with_log=False, phase=False)
    env = dev.env
    assert env.cfg.obs_rows == R and env.ppo_steps256_supported(R) and not env.ppo_steps64_supported(R)
    ref = PPOChecker(oracle_mod, agent, kw, B, 5, plan, u, 1, with_log=False, phase=False)
    ppo_ref.run_plan(ref, dev, plan, last_row=False)
    print(f"R{R}", ref.summary())
    a_all = dev.read()["actions_f32"][:STEPS * B].reshape(STEPS, B)
    assert a_all[0, 0] == 0.0  # u = 0: the first row
    assert ref.ended.min() >= STEPS // L - 1 and ref.ended.max() >= 2  # every env went on from a restart
