"""The greedy evaluation's reference harness (tests/eval_ref.py) at the shapes of lb_eval_steps256,
checked on the CPU with no GPU: tests/test_eval_ref_harness.py's float32 stand-in (a second oracle
as the env, torch's float32 forward with first-index argmax) at E = 65 with the reject row up to
E = 256 with it (R = 66 .. 257).  The float64 reference must accept a correct float32 implementation
at these set sizes too: every case inside the action tolerance (dqn_ref.action_tol) and the
disagreement cap (at most 1e-3 of a case's decisions).  tests/test_gpu_eval256_oracle.py runs the
same cases on the HIP kernels.

Measured, the stand-in: 0 disagreements with the float64 argmax and a largest Q64 shortfall of 0 in
every case; 2,120 decisions each (40 steps in launches of 1, 6, 13 and 20), 2,100 for the no-reset
case (one launch of L = 7), so the cap allows 2 disagreements per case.
"""
import pytest

import eval_ref
from test_eval_ref_harness import PLAN, run_case

assert PLAN == (1, 6, 13, 20)


def _kw(E, rej):
    return dict(num_endpoints=E, rejection_allowed=rej, reward_function="multi", episode_length=7)


# name: (kw, B, network, weight seed, masks, auto-reset, plan): at least 2,000 decisions each
CASES = {
    "R66-B53-dqn-w3": (_kw(65, True), 53, "dqn", 3, False, True, PLAN),
    "R80-norej-B53-ppo-w5-masks": (_kw(80, False), 53, "ppo", 5, True, True, PLAN),
    "R81-B53-dqn-w11-masks": (_kw(80, True), 53, "dqn", 11, True, True, PLAN),
    "R96-norej-B53-ppo-w3": (_kw(96, False), 53, "ppo", 3, False, True, PLAN),
    "R129-B53-ppo-w3-masks": (_kw(128, True), 53, "ppo", 3, True, True, PLAN),
    "R130-B53-dqn-w5": (_kw(129, True), 53, "dqn", 5, False, True, PLAN),
    "R151-B53-ppo-w11": (_kw(150, True), 53, "ppo", 11, False, True, PLAN),
    "R181-B53-dqn-w3-masks": (_kw(180, True), 53, "dqn", 3, True, True, PLAN),
    "R256-norej-B53-dqn-w7-masks": (_kw(256, False), 53, "dqn", 7, True, True, PLAN),
    "R257-B53-ppo-w5-masks": (_kw(256, True), 53, "ppo", 5, True, True, PLAN),
    # run_test's: auto-reset off, the episode in one launch
    "R181-B300-dqn-w7-no-reset": (_kw(180, True), 300, "dqn", 7, False, False, (7,)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_reference_accepts_float32_forward_up_to_256_endpoints(oracle_mod, name):
    kw, B, kind, wseed, masks, auto, plan = CASES[name]
    ref = run_case(oracle_mod, kw, B, kind, wseed, masks, auto, plan)
    assert ref.greedy_decisions >= 2000
    assert ref.max_shortfall <= ref.max_tol and ref.share() <= eval_ref.MAX_DISAGREE_SHARE
