"""k_dqn_steps256 (csrc/lbk8s_dqn256.h: lb_dqn_steps256, a DQN train period's vector steps in one
launch for envs of up to 256 endpoints) pinned DIRECTLY to the C oracle and a float64 Q network.

tests/test_gpu_dqn_steps256.py shows the launch equal to n x (lb_dqn_act + lb_step + lb_replay_add),
HIP against HIP.  Here the other side is tests/dqn_ref.py's StepChecker, as in
tests/test_gpu_dqn64_oracle.py: oracle.OracleBatch as the env, oracle.dqn_explore as the explore
decision, policy_random() as an exploring step's actions, the float64 copy of the Q network for the
greedy ones, a numpy ring for the replay buffer.  The device supplies each step's action; the
reference validates it and follows it, so every replay row, output buffer, terminal obs,
episode-statistics row, finished-episode sum and device word of every launch is compared bit for
bit.  The device is test_gpu_dqn_oracle.HipDevice with every launch of the plan -- the single
steps too, as n = 1 -- sent through LBVecEnv.dqn_steps256, on shapes lb_dqn_steps64 does not cover.

Cases (tests/test_dqn256_ref_harness.py's): reward "multi", episode length 7, dqn_ref.MIXED (79
steps: n = 1, 2, 7, 32, 32 and five single steps; the ring of 40 slots wraps inside and across
launches) under DEFAULT_SCHEDULE; the first and last row count of each kernel instance and the
evaluation sweep's 180 endpoints, with and without masks (~30 % invalid, an all-invalid env and a
last-row-only env).

Bounds (tests/dqn_ref.py, unchanged): tol = 2 (2e-5 + 4e-6 max|Q|) per decision; at most 1e-3 of
a case's greedy decisions off the float64 argmax; at least 2,000 greedy decisions per case.
Measured:
  CPU, torch's float32 forward as the device (tests/test_dqn256_ref_harness.py, these cases): 19
  explored + 60 greedy steps, 2,220 .. 3,180 greedy decisions, 0 or 1 disagreements per case (R66:
  1 of 3,180, shortfall 3.1e-6), tol 4.3e-4 .. 1.0e-3.
  MI355X, the HIP kernel (this file; explored + greedy steps, greedy decisions, disagreements,
  largest Q64 shortfall, tol at the largest max|Q|):
    R66-B53-w3           19 + 60   3,180   0   0   5.2e-4 at 60.0
    R80-B53-w5-masks     19 + 60   3,180   0   0   1.0e-3 at 121.3
    R81-B53-w11-masks    19 + 60   3,180   0   0   4.8e-4 at 55.4
    R129-B41-w3-masks    19 + 60   2,460   0   0   4.3e-4 at 49.0
    R130-B41-w5          19 + 60   2,460   0   0   9.6e-4 at 114.5
    R181-B37-w3-masks    19 + 60   2,220   0   0   4.3e-4 at 49.3
    R256-B37-w7-masks    19 + 60   2,220   0   0   8.2e-4 at 97.2
    R257-B37-w5          19 + 60   2,220   0   0   9.6e-4 at 114.4
  Every case: no greedy decision off the float64 argmax (cap 1e-3), every other compared value
  equal bit for bit.
"""
import pytest

import dqn_ref
from dqn_ref import DEFAULT_SCHEDULE, MIXED, SLOTS, StepChecker
from test_dqn256_ref_harness import CASES256, case_id, kw_of
from test_gpu_dqn_oracle import HipDevice

pytestmark = pytest.mark.gpu


class HipDevice256(HipDevice):
    """HipDevice with every launch through LBVecEnv.dqn_steps256 (a single step: n = 1)."""

    def supported(self):
        return self.env.dqn_steps256_supported(self.R) and not self.env.dqn_steps64_supported(self.R)

    def run(self, n, single):
        p, end = self.parity, self.parity ^ (n & 1)
        s, v, pp = self.schedule, self.vpp.data_ptr(), self.rb.pos_pp.data_ptr()
        ex = self.native.LBDQNExploreC(s.start, s.slope, s.end, s.seed, v + 8 * p, v + 8 * end, self.flag.data_ptr())
        self.env.dqn_steps256(n, self.frag, self.obs, self.masks, ex, self.act, self.next_obs, self.rew, self.done,
                              self.rb, pp + 8 * p, pp + 8 * end, self.ep_sum, self.ep_cnt, self.sync)
        self.parity = end


@pytest.mark.parametrize("E,rej,B,wseed,masks", CASES256, ids=[case_id(c) for c in CASES256])
def test_dqn_steps256_equals_oracle(oracle_mod, E, rej, B, wseed, masks):
    kw = kw_of(E, rej)
    m = dqn_ref.random_masks(B, E + int(rej), seed=B) if masks else None
    dev = HipDevice256(kw, B, 5, wseed, SLOTS, DEFAULT_SCHEDULE, m)
    assert dev.supported()  # the new kernel, not lb_dqn_steps64's
    ref = StepChecker(oracle_mod, dev.q, kw, B, 5, SLOTS, DEFAULT_SCHEDULE, m)
    ref.check_reset(dev)
    for n, single in MIXED:
        ref.launch(dev, n, single)
    print(f"\n{case_id((E, rej, B, wseed, masks))}: {ref.summary()}")
    ref.finish(dev)
    assert ref.greedy_decisions >= 2000
    assert ref.max_shortfall <= ref.max_tol
    assert ref.disagreements <= dqn_ref.MAX_DISAGREE_SHARE * ref.greedy_decisions
