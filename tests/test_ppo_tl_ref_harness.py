"""GAE with the time-limit bootstrap on the CPU, with no GPU: the segment-wise float32 reference
(tests/ppo_tl_ref.py) against lbk8s.ppo.compute_gae_tl, which is lb_gae_tl's expression in torch.

(a) The checker accepts compute_gae_tl on the GPU test's shapes (tests/test_gpu_ppo_tl.py runs the
    same checker on lb_gae_tl).
(b) The checker catches what it claims to: five variants of the recurrence with one planted defect
    each change at least one output bit of the case and are refused.
(c) compute_gae_tl is compute_gae, bit for bit, with term_values all zero and, whatever term_values
    holds, with no done anywhere.
"""
import numpy as np
import pytest
import torch

import ppo_tl_ref as tl

SHAPES = ((1, 1), (5, 67), (12, 130))


def _torch_fn(f):
    def run(*a):
        *arrays, gamma, lam = a
        adv, ret = f(*(torch.from_numpy(x.copy()) for x in arrays), gamma, lam)
        return adv.numpy(), ret.numpy()
    return run


@pytest.mark.parametrize("T,B", SHAPES)
def test_checker_accepts_compute_gae_tl(T, B):
    from lbk8s.ppo import compute_gae_tl
    case = tl.make_case(T, B, seed=100 * T + B)
    tl.check_gae_tl(_torch_fn(compute_gae_tl), case)
    if T > 1:  # the case holds what it promises
        d, nd = case["dones"], case["next_done"]
        assert d[1].any() and nd.any() and (d[1:-1] * d[2:]).any() if T > 2 else nd.any()


BUGS = ("bootstrap_from_next_episode", "chain_not_cut", "term_values_next_row", "next_done_ignored",
        "bootstrap_times_nonterminal")


def variant(bug=None):
    """The header's recurrence in float32 torch; bug: one of BUGS."""
    assert bug is None or bug in BUGS

    def f(rewards, values, dones, next_value, next_done, term_values, gamma, gae_lambda):
        T = rewards.shape[0]
        adv = torch.zeros_like(rewards)
        last = torch.zeros_like(rewards[0])
        for t in reversed(range(T)):
            nd = next_done if t == T - 1 else dones[t + 1]
            nv = next_value if t == T - 1 else values[t + 1]
            if bug == "next_done_ignored" and t == T - 1:
                nd = torch.zeros_like(nd)
            tv = term_values[t]
            if bug == "term_values_next_row":
                tv = term_values[t + 1] if t + 1 < T else torch.zeros_like(tv)
            bv = nv if bug == "bootstrap_from_next_episode" else torch.where(nd != 0, tv, nv)
            nnt = 1.0 - nd
            if bug == "bootstrap_times_nonterminal":  # (lb_gae's expression: the reference's behaviour)
                delta = rewards[t] + gamma * bv * nnt - values[t]
            else:
                delta = rewards[t] + gamma * bv - values[t]
            chain = gamma * gae_lambda * last if bug == "chain_not_cut" else gamma * gae_lambda * nnt * last
            last = delta + chain
            adv[t] = last
        return adv, adv + values
    return f


DEFECT_SHAPE = (12, 130)


def test_variant_without_defect_is_accepted():
    T, B = DEFECT_SHAPE
    tl.check_gae_tl(_torch_fn(variant()), tl.make_case(T, B, seed=7))


@pytest.mark.parametrize("bug", BUGS)
def test_checker_catches_broken_variant(bug):
    T, B = DEFECT_SHAPE
    case = tl.make_case(T, B, seed=7)
    args = [case[k] for k in tl.ORDER] + [tl.GAMMA, tl.LAMBDA]
    clean, broken = _torch_fn(variant())(*args), _torch_fn(variant(bug))(*args)
    assert any(not np.array_equal(tl.bits(a), tl.bits(b)) for a, b in zip(clean, broken)), \
        f"{bug} changes no output bit of the case"
    with pytest.raises(AssertionError, match="gae_tl: (advantages|returns)"):
        tl.check_gae_tl(_torch_fn(variant(bug)), case)


@pytest.mark.parametrize("T,B", SHAPES)
def test_compute_gae_tl_is_compute_gae_where_it_must(T, B):
    from lbk8s.ppo import compute_gae, compute_gae_tl
    for name, case in (("zero term_values", dict(tl.make_case(T, B, seed=3), term_values=np.zeros((T, B), np.float32))),
                       ("no done", tl.make_case(T, B, seed=4, no_done=True))):
        t = {k: torch.from_numpy(v.copy()) for k, v in case.items()}
        assert (name == "no done") == (not case["dones"].any() and not case["next_done"].any())
        old = compute_gae(t["rewards"], t["values"], t["dones"], t["next_value"].reshape(1, -1), t["next_done"],
                          tl.GAMMA, tl.LAMBDA)
        new = compute_gae_tl(t["rewards"], t["values"], t["dones"], t["next_value"].reshape(1, -1), t["next_done"],
                             t["term_values"], tl.GAMMA, tl.LAMBDA)
        for a, b in zip(old, new):
            assert np.array_equal(tl.bits(a.numpy()), tl.bits(b.numpy())), name
        assert np.isfinite(new[0].numpy()).all()


def test_option_defaults_off():
    import inspect
    from lbk8s import cli
    from lbk8s.ppo import PPO_DeepSets
    assert inspect.signature(PPO_DeepSets).parameters["bootstrap_timeouts"].default is False
    assert cli.build_parser().parse_args([]).bootstrap_timeouts is False
    assert cli.build_parser().parse_args(["--bootstrap-timeouts"]).bootstrap_timeouts is True
    with pytest.raises(SystemExit, match="ppo_deepsets option"):
        cli.main(["--alg", "dqn_deepsets", "--bootstrap-timeouts"])
