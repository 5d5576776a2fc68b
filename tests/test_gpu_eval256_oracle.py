"""k_eval_steps256 (csrc/lbk8s_steps256.h: lb_eval_steps256, a greedy evaluation's vector steps in one
launch for envs of 65 to 256 endpoints) pinned DIRECTLY to the C oracle and a float64 network.

tests/test_gpu_eval_steps256.py shows the launch equal to steps x (lb_ds_q_argmax, lb_step,
lb_ppo_record), HIP against HIP.  Here the other side is tests/eval_ref.py, as in
tests/test_gpu_eval64_oracle.py: oracle.OracleBatch as the env, the float64 copy of the actor / Q
network on the oracle's observations; the device's actions are validated with tests/dqn_ref.py's
rules and bounds (valid under the mask, within action_tol of the float64 maximum, the first of
identical rows; at most 1e-3 of a case's decisions off the float64 argmax), then followed, so every
other output is compared bit for bit.  The cases are tests/test_eval256_ref_harness.py's, which
shows on the CPU that a correct float32 forward passes them.

Measured on an MI355X (decisions, disagreements with the float64 argmax, largest Q64 shortfall, tol
at the largest max|Q|; tol = 2 (2e-5 + 4e-6 max|Q|), cap 1e-3 of a case's decisions):
    R66-B53-dqn-w3                 2,120   0   0        4.0e-4 at 45.5
    R80-norej-B53-ppo-w5-masks     2,120   0   0        1.0e-3 at 122.2
    R81-B53-dqn-w11-masks          2,120   0   0        4.4e-4 at 49.7
    R96-norej-B53-ppo-w3           2,120   0   0        3.5e-4 at 38.5
    R129-B53-ppo-w3-masks          2,120   0   0        4.3e-4 at 48.4
    R130-B53-dqn-w5                2,120   0   0        9.6e-4 at 115.0
    R151-B53-ppo-w11               2,120   1   7.0e-6   4.1e-4 at 46.7    (share 4.7e-4)
    R181-B53-dqn-w3-masks          2,120   0   0        4.4e-4 at 49.7
    R256-norej-B53-dqn-w7-masks    2,120   0   0        8.2e-4 at 97.3
    R257-B53-ppo-w5-masks          2,120   0   0        1.0e-3 at 124.3
    R181-B300-dqn-w7-no-reset      2,100   0   0        8.1e-4 at 96.8
  One decision in 23,300 off the float64 argmax (inside the tolerance); every other compared value
  equal bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import eval_ref
from eval_ref import EvalChecker
from test_eval256_ref_harness import CASES
from test_gpu_eval_oracle import HipDevice

pytestmark = pytest.mark.gpu


class HipDevice256(HipDevice):
    """lb_eval_steps256 through the C ABI on HipDevice's buffers."""

    def run(self, n, tag0):
        env, p = self.env, lambda t: None if t is None else t.data_ptr()
        self.n = n
        self.native.check(self.native.lib().lb_eval_steps256(
            p(self.frag), p(self.obs), p(env.state), C.byref(env._c), self.B, self.R, p(self.masks), n,
            p(self.actions_all), p(self.rewards_all), p(self.dones_all), p(self.act), p(self.rew), p(self.done),
            p(self.ep_stats), p(self.ep_sum), p(self.ep_cnt), p(self.ret32), p(self.ep_r32), tag0, p(self.log),
            self.cap, p(self.count), None))


@pytest.mark.parametrize("name", list(CASES))
def test_eval_steps256_equals_oracle(oracle_mod, name):
    kw, B, kind, wseed, masks, auto, plan = CASES[name]
    R = kw["num_endpoints"] + (1 if kw["rejection_allowed"] else 0)
    m = eval_ref.random_masks(B, R, seed=B) if masks else None
    dev = HipDevice256(kw, B, 5, kind, wseed, m, auto)
    assert dev.env.eval_steps256_supported(R) and not dev.env.eval_steps64_supported(R)
    ref = EvalChecker(oracle_mod, dev.net, kw, B, 5, m, auto)
    np.testing.assert_array_equal(dev.read()["obs"], ref.obs, err_msg="reset obs")
    for n in plan:
        ref.launch(dev, n)
    print(f"\n{name}: {ref.summary()}, share {ref.share():.2e}")
    assert ref.greedy_decisions >= 2000
    ref.finish(dev)
