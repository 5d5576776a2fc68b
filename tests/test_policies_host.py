"""The host side of the policies LB_POLICY_ROUND_ROBIN .. LB_POLICY_REWARD_GREEDY (include/lbk8s.h):
the names, the host forms of lbk8s.baselines on a stub env, the refusals of lb_policy / lb_rollout
(answered before any device call: the pointers handed over are not device memory), and the harness
of the reward-greedy checker (tests/policies_ref.py) on the C oracle alone.  No GPU; the refusals
need the built library, as tests/test_eval_steps_host.py.
"""
import ctypes as C

import numpy as np
import pytest

import policies_ref as pr

FAKE = 4096  # never dereferenced: a refused call makes no device call


def test_policy_names():
    from lbk8s import _native, baselines, run_baselines
    assert _native.LB_POLICY == {"topo": 0, "zone_cpu": 1, "endpoint_cpu": 2, "random": 3, "round_robin": 4,
                                 "least_loaded": 5, "least_latency": 6, "reward_greedy": 7}
    assert set(baselines.POLICIES) == {"topo", "zone_cpu", "endpoint_cpu"}  # the reference's three, unchanged
    assert set(baselines.K8S_POLICIES) == {"round_robin", "least_loaded", "least_latency"}
    assert run_baselines.POLICIES == ("topo", "zone_cpu", "endpoint_cpu")
    assert run_baselines.DEVICE_POLICIES == run_baselines.POLICIES + ("round_robin", "least_loaded", "least_latency",
                                                                      "reward_greedy")
    assert all(k in _native.LB_POLICY for k in run_baselines.DEVICE_POLICIES)
    assert "lbk8s_policies.hip" in _native.SOURCES


class StubEnv:
    def __init__(self, step, loads, lat, topo):
        self.current_step = step
        self.avg_load_served = np.asarray(loads, float)
        self.endpoint_latency = np.asarray(lat, float)
        self.endpoint_topology_latency = np.asarray(topo, float)


def test_host_forms_semantics():
    from lbk8s import baselines as b
    env = StubEnv(0, [2, 1, 1, 1], [30.5, 10.25, 9.25, 9.0], [1, 1, 2, 1])
    rej, norej = np.ones(5, bool), np.ones(4, bool)
    for mask in (rej, norej):  # all E endpoints either way, never the reject action
        assert b.least_loaded_policy(env, mask) == 1              # first of the tied minima
        assert b.least_latency_policy(env, mask) == 3             # 10.0: the last endpoint is eligible
    # a tie of the float64 sums goes to the lowest index: 10.25 + 1 == 9.25 + 2
    assert b.least_latency_policy(StubEnv(0, [0] * 4, [30.5, 10.25, 9.25, 10.5], [1, 1, 2, 1]), norej) == 1
    # the last endpoint without rejection (the reference's mask[:-1] would never pick it)
    assert b.least_loaded_policy(StubEnv(0, [3, 3, 3, 2], [1] * 4, [1] * 4), norej) == 3
    # round robin: current_step mod E, wrapping at E, whatever the mask's length
    for step in range(10):
        env = StubEnv(step, [0] * 4, [1] * 4, [1] * 4)
        assert b.round_robin_policy(env, rej) == b.round_robin_policy(env, norej) == step % 4
    # the batched references agree with the host forms
    rng = np.random.default_rng(3)
    lat, topo = rng.uniform(1, 100, (50, 5)), rng.integers(1, 500, (50, 5))
    loads = rng.integers(0, 3, (50, 5))
    for i in range(50):
        env = StubEnv(i, loads[i], lat[i], topo[i])
        assert b.least_loaded_policy(env, None) == pr.least_loaded(loads)[i]
        assert b.least_latency_policy(env, None) == pr.least_latency(lat, topo)[i]
        assert b.round_robin_policy(env, None) == pr.round_robin(np.arange(50), 5)[i]


def test_unknown_kind_is_refused_before_any_device_call():
    from lbk8s import LBConfig, _native
    L = _native.lib()
    cfg = LBConfig().to_c(0, 0, True, False, "auto")
    for kind in (-1, 8):
        assert L.lb_policy(FAKE, C.byref(cfg), 8, kind, FAKE + 64, None) < 0
        assert b"unknown policy kind" in L.lb_last_error()
        assert L.lb_rollout(FAKE, C.byref(cfg), 8, kind, 3, None, None, None, None, None, None, None) < 0
        assert b"unknown policy kind" in L.lb_last_error()
        with pytest.raises(RuntimeError, match="unknown policy kind"):
            _native.check(L.lb_policy(FAKE, C.byref(cfg), 8, kind, FAKE + 64, None))
    assert L.lb_abi_version() == 17


def test_run_baselines_refuses_other_names():
    from lbk8s.run_baselines import run_baselines
    for name in ("random", "greedy"):  # before any env is built
        with pytest.raises(ValueError, match="unrecognized policy"):
            run_baselines(policy=name, n_episodes=4)


# ---- the reward-greedy checker on the oracle alone ----------------------------------------------

def _last_argmax(r):
    return (r.shape[1] - 1 - np.argmax(r[:, ::-1], axis=1)).astype(np.int32)


def _model(defect):
    return lambda ck, r: pr.first_argmax(pr.reward_model(ck.cur, ck.kw, defect))


# broken stand-in -> the case that catches it
BROKEN = {
    "last_index_on_ties": ("fairness_e6_tpe", lambda ck, r: _last_argmax(r)),
    "gini_before_the_accept": ("fairness_e6_tpe", _model("gini_pre")),
    # (under the fairness reward j' < j and j' <= j order the endpoints alike; the multi reward
    # weighs the term against the latency, so its size matters)
    "cnt_less_than": ("multi", _model("cnt_lt")),
    "latency_after_the_increment": ("latency_e3_norej", _model("lat_after")),
    "reject_left_out": ("multi_negative_reject", lambda ck, r: pr.first_argmax(r[:, :ck.E])),
    "wrong_zone_topology": ("latency_e3_norej", _model("wrong_zone")),
}


def _checker(oracle_mod, name):
    B, kw, _ = pr.GREEDY_CASES[name]
    return pr.GreedyChecker(oracle_mod, dict(kw, episode_length=pr.L_GREEDY), B, pr.GREEDY_SEED)


@pytest.mark.parametrize("name", list(pr.GREEDY_CASES))
def test_checker_passes_the_first_argmax_and_cases_hold(oracle_mod, name):
    """The stand-in that returns the first argmax of the brute-force rewards passes; the formula
    in numpy (policies_ref.reward_model) equals the brute force bit for bit at every decision;
    and the case has what makes it a test: decisions other than action 0, exact ties, decisions
    the pre-accept Gini gets wrong, decisions where reject is the argmax."""
    ck = _checker(oracle_mod, name)
    kw = ck.kw
    seen = dict(n=0, nonzero=0, ties=0, gini_pre=0, reject=0)

    def on_decision(t, r, want):
        np.testing.assert_array_equal(pr.reward_model(ck.cur, kw), r)
        seen["n"] += len(want)
        seen["nonzero"] += int((want != 0).sum())
        seen["ties"] += int(((r == r.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
        seen["gini_pre"] += int((pr.first_argmax(pr.reward_model(ck.cur, kw, "gini_pre")) != want).sum())
        seen["reject"] += int((want == ck.E).sum())

    assert ck.run(lambda c, r: pr.first_argmax(r), pr.T_GREEDY, on_decision) == 0
    assert seen["n"] == ck.B * pr.T_GREEDY and pr.T_GREEDY > 2 * pr.L_GREEDY  # two episode ends crossed
    fn = kw["reward_function"]
    if fn == "naive":
        assert seen["nonzero"] == 0 and seen["ties"] == seen["n"]  # every accept pays 1.0: action 0
    else:
        assert seen["nonzero"] >= 0.3 * seen["n"], seen
    if name in ("fairness_e6_tpe", "multi"):
        assert seen["gini_pre"] >= 20, seen
    if fn == "fairness":  # where equal loads make equal rewards: the tie rule is exercised
        assert seen["ties"] >= 20, seen
    if name == "multi_negative_reject":
        assert 20 <= seen["reject"] < seen["n"], seen
    elif ck.A > ck.E:
        assert seen["reject"] == 0  # weights >= 0: every accept pays more than the reject constant


@pytest.mark.parametrize("bug", list(BROKEN))
def test_checker_fails_each_broken_stand_in(oracle_mod, bug):
    name, policy = BROKEN[bug]
    assert _checker(oracle_mod, name).run(policy, pr.T_GREEDY) > 0, bug
