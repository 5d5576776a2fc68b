"""The loss heads', episode log's and replay sample's reference harness (tests/heads_ref.py)
checked on the CPU, with no GPU.

The device under test here is a stand-in: each kernel's documented formula in float32 torch /
numpy (tests/test_gpu_heads.py runs the same checkers on the HIP kernels).

(a) The references accept a correct float32 implementation on every case of every table.
(b) The recipes meet their own conditions: no set within the margins, ties that are ties in
    both precisions, at least 16 rounding-sensitive envs, a high counter word that matters.
(c) The checkers catch what they claim to: each deliberately broken stand-in fails a named case.
"""
import numpy as np
import pytest

import heads_ref as hr


class StandIn:
    def __init__(self, oracle_mod=None, bug=None):
        self.oracle, self.bug = oracle_mod, bug

    def ppo_head(self, c, bufs):
        return hr.ppo_stand_in(c, bufs, self.bug)

    def dqn_head(self, c, bufs, block):
        return hr.dqn_stand_in(c, bufs, block, self.bug)

    def episode_log(self, *a):
        return hr.eplog_stand_in(*a, bug=self.bug)

    def replay_sample(self, c, ring, bufs):
        return hr.sample_stand_in(c, ring, bufs, self.oracle, self.bug)


# ---- (a) ---------------------------------------------------------------------------------------

def test_ppo_case_names():
    assert list(hr.ppo_cases()) == hr.PPO_CASE_NAMES


@pytest.mark.parametrize("name", hr.PPO_CASE_NAMES)
def test_ppo_reference_accepts_float32(name):
    shares = hr.run_ppo(StandIn(), name)
    print(name, {k: round(v, 3) for k, v in shares.items()})
    assert max(shares.values()) <= 1.0


@pytest.mark.parametrize("spec", hr.DQN_CASES, ids=hr.dqn_case_id)
def test_dqn_reference_accepts_float32(spec):
    shares, bitwise = hr.run_dqn(StandIn(), spec)
    print(hr.dqn_case_id(spec), {k: {q: round(v, 3) for q, v in s.items()} for k, s in shares.items()})
    assert bitwise is (True if spec[0] <= 1024 else None)


@pytest.mark.parametrize("spec", hr.eplog_specs(), ids=hr.eplog_id)
def test_eplog_reference_accepts_stand_in(spec):
    hr.run_eplog(StandIn(), spec)


@pytest.mark.parametrize("spec", hr.SAMPLE_CASES, ids=lambda s: s[0])
def test_sample_reference_accepts_stand_in(oracle_mod, spec):
    hr.run_sample(StandIn(oracle_mod), spec, oracle_mod)


# ---- (b) ---------------------------------------------------------------------------------------

def test_ppo_recipes_meet_their_conditions():
    kinds, ratio_sides, v_sides = set(), set(), set()
    for name, c in hr.ppo_cases().items():
        a = c.actions.astype(int)
        assert ((a >= 0) & (a < c.R)).all()
        assert set(c.forced) <= set(a.tolist()), name
        if c.M == 517:   # rows 0, R - 1 and both sides of every 64-row register slot
            assert set(c.forced) == {0, c.R - 1} | {b for b in hr.BOUNDARY_ROWS if b < c.R}, name
        if c.masks is not None:
            valid = c.masks.sum(1)
            assert (valid[c.in_scope] >= 1).all() and (valid[~c.in_scope] == 0).all()
            assert c.masks[np.arange(c.M), a][c.in_scope].all(), "a taken action is masked"
            assert all(valid[s] == 1 for s in c.one_valid)
            if c.M >= 5:
                assert len(c.one_valid) == 2 and (~c.in_scope).sum() == 1
            if c.M == 517 and c.R >= 9:
                share = 1 - c.masks[c.in_scope].mean()
                assert 0.15 < share < 0.25, (name, share)
        near = hr.ppo_margins(c) & c.in_scope
        if c.ties:
            out = hr.ppo_stand_in(c, hr.ppo_buffers(c))
            kinds |= hr.check_tie_recipe(c, out["ratio32"])
            assert set(np.flatnonzero(near)) <= set(c.tie_sets), name
        else:
            assert not near.any(), name
            if c.M == 517:  # both sides of every kink are populated
                ref = hr.ppo_reference(c)
                clip = float(np.float32(c.clip))
                ratio_sides |= {int(x) for x in np.sign(np.abs(ref.ratio - 1) - clip)}
                v_sides |= {int(x) for x in np.sign(np.abs(c.value - c.vold) - clip)}
    assert kinds == {"ratio1", "bound", "vmax", "same"}
    assert ratio_sides == {-1, 1} and v_sides == {-1, 1}
    c = hr.ppo_cases()["M32773-R3-masks-loop"]
    assert c.M > 4 * 8192 and c.M % 4
    np.testing.assert_array_equal(c.logits[-1], np.roll(c.logits[0], 1))
    assert not np.array_equal(c.logits[-1], c.logits[0])


def test_dqn_recipes_meet_their_conditions():
    Ms, Rs = set(), set()
    for spec in hr.DQN_CASES:
        c = hr.dqn_case(spec)
        Ms.add(c.M)
        Rs.add(c.R)
        assert c.actions[-1] == c.R - 1 and (c.M == 1 or c.actions[0] == 0)
        top = c.q_next.max(1)
        assert ((c.q_next == top[:, None]).sum(1)[c.twice] >= 2).all()
        assert c.twice.any() == (c.R >= 2)
    assert {1, 5, 63, 64, 65, 128, 1024, 1025, 2000, 4 * 65535 + 5} <= Ms
    assert {1, 2, 63, 64, 65, 128, 257} <= Rs
    assert sum(1 for s in hr.DQN_CASES if s[3]) >= 1
    assert {s[2] for s in hr.DQN_CASES} == {"zeros", "ones", "mixed"}


def test_eplog_recipes_meet_their_conditions():
    specs = hr.eplog_specs()
    assert {s[0] for s in specs} == set(hr.EPLOG_B)
    assert {s[1] for s in specs} == set(hr.EPLOG_PATTERNS)
    assert {s[4] for s in specs} == {"ample", "exact", "short", "zero"}
    assert any(not s[2] for s in specs) and any(not s[3] for s in specs)
    for spec in specs:
        c = hr.eplog_case(spec)
        assert c.sensitive >= min(c.B, 16), (c.name, c.sensitive)
        if spec[4] == "short":
            assert 0 < c.cap < c.total, c.name
        if spec[1] == "wave":   # a whole wave finished beside three waves of its block with none
            d = c.calls[0].done
            assert d[64:128].all() and not d[:64].any() and not d[128:256].any()
        if spec[1] == "none":
            assert c.total == 0


def test_sample_recipes_meet_their_conditions(oracle_mod):
    cases = {s[0]: hr.sample_case(s) for s in hr.SAMPLE_CASES}
    assert {c.B for c in cases.values()} == {1, 300}
    assert {c.F for c in cases.values()} == {4, 72, 2056}
    assert {c.batch for c in cases.values()} == {1, 5, 512}
    assert sum(1 for c in cases.values() if c.threads % 256) >= 3
    assert any(c.B & (c.B - 1) for c in cases.values())   # a B that is no power of two
    for name in ("empty-B300-F72-n512", "empty-B1-F4-n1"):
        assert cases[name].base + cases[name].vstep == 0 and hr.sample_upper(cases[name]) == 1
    hi, lo = cases["hi-part-B300-F72-n512"], cases["lo-part-B300-F72-n512"]
    assert hi.vstep >> 32 == 1 and hi.vstep & 0xFFFFFFFF == lo.vstep
    assert hr.sample_upper(hi) == hr.sample_upper(lo) == 3 < hi.S
    assert hr.sample_upper(cases["hi-full-B300-F72-n512"]) == hi.S
    a = oracle_mod.replay_sample(hi.seed, hi.vstep, 3, hi.B, hi.batch)
    b = oracle_mod.replay_sample(lo.seed, lo.vstep, 3, lo.B, lo.batch)
    assert (a[0] != b[0]).any() and (a[1] != b[1]).any()


# ---- (c) ---------------------------------------------------------------------------------------

# mutation: (a case that must fail, the checker's message)
PPO_BUGS = {
    "tie_first": ("ties-R9-clip0.25-masks", "dvalue"),           # max ties weighted 1 / 0
    "open_clamp": ("ties-R9-clip0.25-masks", "dvalue"),          # clamp's interval taken open
    "no_entropy_grad": ("M517-R65-masks", "dlogits"),
    "masked_grad": ("M517-R65-masks", "no valid row got a logit gradient|masked row got a gradient"),
    "low_bits": ("M517-R65-masks", "term pg|term kl|dlogits"),   # log-prob at a & 63, a >> 6 ignored
    "wrong_m": ("M517-R9-ent0", "dlogits|dvalue"),               # 1 / (M + 1)
    "last_terms": ("M32773-R3-masks-loop", "terms: .* unwritten"),
}
DQN_BUGS = {
    "no_done": ((65, 65, "mixed", False), "td at"),
    "dq_sparse": ((65, 65, "mixed", False), "dq: .* unwritten"),
}
EPLOG_BUGS = {
    "two_roundings": ((257, "random", True, True, "ample"), "ret32"),
    "count_capped": ((257, "random", True, True, "short"), "count"),
    "past_cap": ((257, "random", True, True, "short"), "past min"),
    "no_restart": ((257, "random", True, True, "ample"), "ret32"),
}
SAMPLE_BUGS = {
    "unclamped": ("empty-B300-F72-n512", "unwritten"),
    "low_word": ("hi-part-B300-F72-n512", "drawn"),
}


@pytest.mark.parametrize("bug", list(PPO_BUGS))
def test_ppo_checker_catches(bug):
    name, match = PPO_BUGS[bug]
    hr.run_ppo(StandIn(), name)
    with pytest.raises(AssertionError, match=match):
        hr.run_ppo(StandIn(bug=bug), name)


def test_ppo_low_bits_caught_at_every_slot():
    """The a & 63 mutation fails every case whose actions reach a second register slot."""
    for name, c in hr.ppo_cases().items():
        if c.M == 517 and c.R >= 65:
            with pytest.raises(AssertionError):
                hr.run_ppo(StandIn(bug="low_bits"), name)


@pytest.mark.parametrize("bug", list(DQN_BUGS))
def test_dqn_checker_catches(bug):
    spec, match = DQN_BUGS[bug]
    hr.run_dqn(StandIn(), spec)
    with pytest.raises(AssertionError, match=match):
        hr.run_dqn(StandIn(bug=bug), spec)


@pytest.mark.parametrize("bug", list(EPLOG_BUGS))
def test_eplog_checker_catches(bug):
    spec, match = EPLOG_BUGS[bug]
    assert spec in hr.eplog_specs()
    hr.run_eplog(StandIn(), spec)
    with pytest.raises(AssertionError, match=match):
        hr.run_eplog(StandIn(bug=bug), spec)


@pytest.mark.parametrize("bug", list(SAMPLE_BUGS))
def test_sample_checker_catches(oracle_mod, bug):
    name, match = SAMPLE_BUGS[bug]
    spec = next(s for s in hr.SAMPLE_CASES if s[0] == name)
    hr.run_sample(StandIn(oracle_mod), spec, oracle_mod)
    with pytest.raises(AssertionError, match=match):
        hr.run_sample(StandIn(oracle_mod, bug), spec, oracle_mod)
