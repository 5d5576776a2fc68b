"""k_ppo_steps, k_ppo_steps64 and k_ppo_steps256 (lb_ppo_steps, lb_ppo_steps64, lb_ppo_steps256: a PPO
rollout's vector steps in one launch) pinned DIRECTLY to the C oracle, a float64 network and the
numpy bookkeeping model, through the C ABI.

tests/test_gpu_ppo_steps.py, test_gpu_ppo_steps64.py and test_gpu_ppo_steps256.py show each launch
equal to steps x (lb_ds_sample, lb_step, lb_ppo_record), HIP against HIP.  Here the other side is
tests/ppo_ref.py: oracle.OracleBatch as the env (brought out of phase by the same calls), the
float64 copy of the DeepSetAgent on the oracle's observations, tests/ppo_tail_ref.ppo_record_ref
for ep_sum / ep_cnt, VecMonitor's float32 return and the log.  Every stored row's draw goes through
tests/ds_sample_ref.check_sample (tolerances unchanged, no row exempt) against lb_ds_forward of the
row's input observation; the oracle follows the validated actions, so rewards, dones_next /
obs_next or last_done / last_obs, actions_out, done_out, the lb_reward64 array, ep_stats, ep_sum /
ep_cnt, ret32 / ep_r32, count, every log row and its tag0 + i, the guard elements, stats() and the
state fields are compared bit for bit, over plans of one and two launches.  The cases, their
variants and the weight seed are tests/test_ppo_ref_harness.py's, which shows on the CPU that a
correct float32 implementation passes them and that fourteen planted defects do not.

Measured on an MI355X (draws, episodes ended; check_sample's worst |error| / allowed per quantity,
<= 1 required; the action's is its distance outside the float64 interval / tol):
                                         draws  ended  logits  value  action  logprob
    ppo_steps-r1                            15      8    0.02   0.03    0       0.00
    ppo_steps-run_py                        88     28    0.15   0.02    0       0.01
    ppo_steps-ragged                     1,170    260    0.16   0.01    0       0.01
    ppo_steps-r16                          536    268    0.15   0.01    0       0.01
    ppo_steps-r16_reject                   536    268    0.15   0.01    0       0.01
    ppo_steps64-a_r17_w16                  335    168    0.14   0.01    0       0.01
    ppo_steps64-b_w32                       35     10    0.10   0.01    0       0.01
    ppo_steps64-c_r32                      335    168    0.17   0.01    0       0.02
    ppo_steps64-d_r33_valu                 165     83    0.13   0.01    0       0.01
    ppo_steps64-e_w64                       63     18    0.14   0.01    0       0.02
    ppo_steps64-f_r49_ts4                   95     48    0.13   0.01    0       0.01
    ppo_steps64-g_r64                       85     43    0.18   0.01    0       0.01
    ppo_steps64-h_r65_config4              144     72    0.16   0.01    0       0.01
    ppo_steps64-j_more_groups_than_waves 6,153  3,077    0.19   0.01    0       0.02
    ppo_steps64-c_r32_two_launches         603    302    0.15   0.01    0       0.01
    ppo_steps256-b_r66                     335    168    0.16   0.01    0       0.02
    ppo_steps256-d_r81                      95     48    0.17   0.01    0       0.01
    ppo_steps256-h_r129_epl2               144     72    0.18   0.01    0       0.01
    ppo_steps256-i_r129_epl4                45     23    0.19   0.00    0       0.01
    ppo_steps256-k_r193_slot4               25     13    0.45   0.01    0       0.01
    ppo_steps256-m_r257                    144     72    0.22   0.01    0       0.01
    ppo_steps256-o_more_envs_than_waves  6,153  3,077    0.19   0.01    0       0.02
    ppo_steps256-d_r81_two_launches        171     86    0.20   0.01    0       0.01
  tests/test_gpu_ppo256_oracle.py's four (48 draws, 24 episodes each): R66 0.32 0.05 0 0.03,
  R81 0.01 0.01 0 0.01, R129 0.01 0.32 0 0.01, R257 0.05 0.02 0 0.02.
  No action outside its float64 interval; every other compared value equal bit for bit: no defect
  found in the three kernels or in the three-launch yardstick they share code with.
"""
import copy

import pytest
import torch

import ppo_ref
from ppo_ref import PPOChecker
from test_gpu_ppo_steps import Bufs, _rew64
from test_gpu_ppo_steps64 import _fused64
from test_ppo_ref_harness import CASES, SEED, WSEED, case_setup

pytestmark = pytest.mark.gpu


class HipDevice:
    """lb_ppo_steps / lb_ppo_steps64 / lb_ppo_steps256 (fn) through the C ABI on one Bufs of the
    whole plan's rows: a launch of n steps writes the rows t .. t + n - 1."""

    def __init__(self, fn, kw, B, seed, agent, plan, u, cap, with_log=True, phase=True):
        from lbk8s import LBVecEnv, fused
        self.fn, self.fused, self.with_log = fn, fused, with_log
        env = self.env = LBVecEnv(B, seed=seed, as_tensors=True, **kw)
        env.reset()
        self.reset_obs = env.obs.cpu().numpy()
        if phase and kw["episode_length"] > 1:  # test_gpu_ppo_steps._env
            env.step_device(None)
            env.reset_masked((torch.arange(B, device="cuda") % 2).to(torch.uint8))
        self.agent = copy.deepcopy(agent).cuda()
        self.frag = fused.packed(self.agent, self.agent.actor.net, self.agent.critic).clone()
        self.B, self.R = B, env.cfg.obs_rows
        T = sum(n for n, _ in plan)
        S = T - (plan[-1][0] - plan[-1][1])
        self.b = Bufs(B, self.R, T, S, cap)
        assert self.b.n == ppo_ref.sizes(B, self.R, T, S, cap)
        self.u = u.cuda()
        self.t = 0

    def first_obs(self):
        """The launch's input: the env's observations, then the previous launch's last stored row."""
        return self.env.obs if self.t == 0 else self.b.obs_next[(self.t - 1) * self.B * self.R * 8:
                                                                self.t * self.B * self.R * 8].view(self.B, self.R, 8)

    def run(self, n, store_rows, tag0):
        _fused64(self.env, self.frag, self.first_obs().data_ptr(), self.u, self.b, steps=n, S=store_rows, step0=self.t,
                 tag0=tag0 - self.t, with_log=self.with_log, fn=self.fn)
        self.t += n

    def read(self):
        torch.cuda.synchronize()
        out = {k: getattr(self.b, k).cpu().numpy() for k in Bufs.ALL}
        out.update(reward64=_rew64(self.env).cpu().numpy(), obs=self.env.obs.cpu().numpy())
        return out

    def forward(self, x):
        logits, value = self.fused.deepsets_forward(self.agent, torch.from_numpy(x).cuda(), require=True)
        return logits.cpu().numpy(), value.cpu().numpy()

    def stats(self):
        return self.env.stats().cpu().numpy()

    def field(self, name):
        return self.env.field(name).cpu().numpy()

    def status(self):
        return self.env.status()


def assert_runs_the_kernel_it_names(env, fn, R):
    """The narrowest entry point that supports the shape is the one the case names."""
    answers = (env.ppo_steps_supported(R), env.ppo_steps64_supported(R), env.ppo_steps256_supported(R))
    assert answers == {"lb_ppo_steps": (True, True, True), "lb_ppo_steps64": (False, True, True),
                       "lb_ppo_steps256": (False, False, True)}[fn], (fn, R, answers)


@pytest.mark.parametrize("name", list(CASES))
def test_ppo_steps_equal_oracle_and_float64_draw(oracle_mod, name):
    fn = CASES[name][0]
    kw, B, plan, u, cap, with_log = case_setup(CASES[name])
    agent = ppo_ref.make_agent(WSEED)
    dev = HipDevice(fn, kw, B, SEED, agent, plan, u, cap, with_log)
    assert_runs_the_kernel_it_names(dev.env, fn, dev.R)
    ref = PPOChecker(oracle_mod, agent, kw, B, SEED, plan, u, cap, with_log)
    ppo_ref.run_plan(ref, dev, plan)
    print(f"\nppo-margin {name}: {ref.summary()}")
