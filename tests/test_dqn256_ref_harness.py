"""The DQN vector step's reference harness (tests/dqn_ref.py) at the shapes of lb_dqn_steps256
(R = 66 .. 257), on the CPU: tests/test_dqn_ref_harness.py's stand-in (a second oracle as the env,
torch's float32 forward as the Q network) through tests/test_gpu_dqn256_oracle.py's cases.

(a) The float64 reference accepts a correct float32 implementation at these set sizes: every case
    stays inside the action tolerance tol = 2 (2e-5 + 4e-6 max|Q|) and the disagreement cap of
    1e-3 of its greedy decisions, over at least 2,000 greedy decisions (the cap leaves room for 2
    disagreements at the smallest case; the stand-in's worst case needs 1 of 3).
(b) The checker still catches what it claims to at R = 257: the broken stand-ins fail it.
"""
import pytest

import dqn_ref
from test_dqn_ref_harness import BUGS, run_case


def kw_of(E, rej):
    return dict(num_endpoints=E, rejection_allowed=rej, reward_function="multi", episode_length=7)


# (E, reject row, B, weight seed, masks): the first and the last row count of each k_dqn_steps256
# instance (R = 66, 80 | 81, 129 on two endpoints per lane | 129, 257 on four), the evaluation
# sweep's 180 endpoints; every case runs dqn_ref.MIXED under dqn_ref.DEFAULT_SCHEDULE
CASES256 = [
    (65, True, 53, 3, False),
    (80, False, 53, 5, True),
    (80, True, 53, 11, True),
    (128, True, 41, 3, True),
    (129, True, 41, 5, False),
    (180, True, 37, 3, True),
    (256, False, 37, 7, True),
    (256, True, 37, 5, False),
]


def case_id(c):
    E, rej, B, wseed, masks = c
    return f"R{E + int(rej)}-B{B}-w{wseed}" + ("-masks" if masks else "")


@pytest.mark.parametrize("E,rej,B,wseed,masks", CASES256, ids=[case_id(c) for c in CASES256])
def test_reference_accepts_float32_forward(oracle_mod, E, rej, B, wseed, masks):
    ref = run_case(oracle_mod, kw_of(E, rej), B, wseed, masks, schedule=dqn_ref.DEFAULT_SCHEDULE, plan=dqn_ref.MIXED)
    assert ref.R == E + int(rej)
    assert ref.greedy_decisions >= 2000, ref.summary()
    assert ref.max_shortfall <= ref.max_tol
    assert ref.disagreements <= dqn_ref.MAX_DISAGREE_SHARE * ref.greedy_decisions


@pytest.mark.parametrize("bug", ("slot_late", "ignore_mask", "last_duplicate", "ep_sum_twice"))
def test_checker_catches_broken_stand_in_at_r257(oracle_mod, bug):
    masks, match = BUGS[bug]
    with pytest.raises(AssertionError, match=match):
        run_case(oracle_mod, kw_of(256, True), 37, 3, masks, bug=bug)
