"""The greedy evaluation's reference harness (tests/eval_ref.py) at the shapes of lb_eval_steps64,
checked on the CPU with no GPU: tests/test_eval_ref_harness.py's float32 stand-in (a second oracle
as the env, torch's float32 forward with first-index argmax) at E = 16 with the reject row up to
E = 64 with it (R = 17 .. 65).  The float64 reference must accept a correct float32 implementation
at these set sizes too: every case inside the action tolerance (dqn_ref.action_tol) and the
disagreement cap (at most 1e-3 of a case's decisions).  tests/test_gpu_eval64_oracle.py runs the
same cases on the HIP kernels.

Measured, the stand-in (decisions, disagreements with the float64 argmax, largest Q64 shortfall,
tol at the largest max|Q|); 40 steps in launches of 1, 6, 13 and 20 unless noted:
    R65-B104-dqn-w3                4,160   1   2.8e-6   4.1e-4 at 45.7    (share 2.4e-4, cap 1e-3)
    R65-B104-ppo-w5-masks          4,160   0   0        1.0e-3 at 123.8
    R33-B61-ppo-w3-masks           2,440   0   0        4.4e-4 at 49.8
    R17-B67-dqn-w3-masks           2,680   0   0        4.5e-4 at 50.8
    R48-norej-B53-dqn-w11-masks    2,120   0   0        4.4e-4 at 50.5
    R17-norej-B67-ppo-w11          2,680   0   0        4.4e-4 at 50.1
    R65-B300-dqn-w7-no-reset       2,100   0   0        8.1e-4 at 96.0    (auto-reset off, one launch of L = 7)
"""
import pytest

import eval_ref
from test_eval_ref_harness import PLAN, run_case


def _kw(E, rej):
    return dict(num_endpoints=E, rejection_allowed=rej, reward_function="multi", episode_length=7)


# name: (kw, B, network, weight seed, masks, auto-reset, plan): at least 2,000 decisions each
CASES = {
    "R65-B104-dqn-w3": (_kw(64, True), 104, "dqn", 3, False, True, PLAN),
    "R65-B104-ppo-w5-masks": (_kw(64, True), 104, "ppo", 5, True, True, PLAN),
    "R33-B61-ppo-w3-masks": (_kw(32, True), 61, "ppo", 3, True, True, PLAN),
    "R17-B67-dqn-w3-masks": (_kw(16, True), 67, "dqn", 3, True, True, PLAN),
    "R48-norej-B53-dqn-w11-masks": (_kw(48, False), 53, "dqn", 11, True, True, PLAN),
    "R17-norej-B67-ppo-w11": (_kw(17, False), 67, "ppo", 11, False, True, PLAN),
    # run_test's: auto-reset off, the episode in one launch
    "R65-B300-dqn-w7-no-reset": (_kw(64, True), 300, "dqn", 7, False, False, (7,)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_reference_accepts_float32_forward_up_to_64_endpoints(oracle_mod, name):
    kw, B, kind, wseed, masks, auto, plan = CASES[name]
    ref = run_case(oracle_mod, kw, B, kind, wseed, masks, auto, plan)
    assert ref.greedy_decisions >= 2000
    assert ref.max_shortfall <= ref.max_tol and ref.share() <= eval_ref.MAX_DISAGREE_SHARE
