"""The training backward's reference harness (tests/ds_bwd_ref.py) checked on the CPU, with no GPU.

The device under test here is a stand-in: the kernels' documented formulas in float32 numpy, laid
out over the backward's grid (tests/test_gpu_ds_backward.py runs the same runners on the HIP
kernels).

(a) The model is a reference: summed over the sets it equals float64 autograd through the
    project's modules to 1e-10 of each gradient's largest entry.
(b) The planted recipes meet their own conditions.
(c) The runners accept a correct float32 implementation on every GPU case.
(d) They catch what they claim to: each deliberately broken stand-in fails the case named for it.
"""
import numpy as np
import pytest

import ds_bwd_ref as br


# ---- (a) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", br.AUTOGRAD_CASES, ids=br.case_id)
def test_model_equals_float64_autograd(c):
    d = br.real_data(c, True)
    got = br.named_grads(d.net, br.model_of(c, True), c.heads)
    exp = br.autograd_grads(c)
    assert sorted(got) == sorted(exp)
    worst = 0.0
    for n, e in exp.items():
        scale = np.abs(e).max()
        assert scale > 0
        worst = max(worst, float(np.abs(got[n] - e).max() / scale))
    print(f"{br.case_id(c)}: worst |model - autograd| / max|autograd| = {worst:.2e}")
    assert worst <= 1e-10


def test_per_set_dlambda_sums_to_the_total():
    c = br.Case("planted", "ac", 17, 9)
    for h, m in br.model_of(c).items():
        for k in ("dL2", "dL1"):
            assert m[k + "_set"].shape[0] == c.B
            np.testing.assert_allclose(m[k + "_set"].sum(0), m[k], rtol=1e-12, atol=1e-12 * np.abs(m[k]).max())


# ---- (b) ---------------------------------------------------------------------------------------
def test_planted_recipes_meet_their_conditions():
    seen = set()
    for c in br.PLANTED_CASES + br.MANY_CASES[:1]:
        if c.heads == "ac":   # (the heads do not enter the recipe)
            seen |= br.check_planted(br.planted_data(c))
    for R in br.PLANTED_R:
        for r in br.named_rows(R):
            assert (R, r) in seen, f"no maximum planted on row {r} at R = {R}"
    assert {(257, 255), (257, 256), (17, 15), (17, 16), (65, 64), (1, 0)} <= seen


def test_case_tables():
    ntl = lambda R: (R + 15) // 16
    nct = lambda R: ((R - 1) % 16) // 4 + 1
    assert {nct(R) for R in br.PLANTED_R} == {1, 2, 3, 4}
    assert {ntl(R) for R in br.PLANTED_R if R % 16 == 1} >= {1, 2, 5, 17}     # the one_row path
    per_wave = lambda B: -(-B // br.GRID_WAVES)
    assert {per_wave(c.B) for c in br.MANY_CASES} == {1, 2, 3, 4}
    assert all(c.B * c.R * 64 * 4 * 4 <= 300e6 for c in br.MANY_CASES)
    assert {(M, N) for L in br.OS_LISTS.values() for _, _, M, N, _ in L} >= set(br._PAIRS)
    assert sorted(len(L) for L in br.OS_LISTS.values()) == [1, 4, 5, 16, 16, 16]


# ---- (c) ---------------------------------------------------------------------------------------
def _fmt(shares):
    return " ".join(f"{k}={v:.3f}" for k, v in shares.items())


@pytest.mark.parametrize("c", br.PLANTED_CASES + br.MANY_CASES, ids=br.case_id)
def test_backward_accepts_float32(c):
    shares, _ = br.run_backward(br.StandIn(), c, repeat=False)
    print(f"{br.case_id(c)}: worst {max(shares.values()):.3f} | {_fmt(shares)}")


def test_backward_accepts_float32_with_a_dirty_workspace():
    c = br.Case("planted", "ac", 17, 9)
    _, a = br.run_backward(br.StandIn(), c, repeat=False)
    _, b = br.run_backward(br.StandIn(), c, ws_fill=1e30, repeat=False)
    for k in ("wgrad", "setvec"):
        br.same_bits(a[k], b[k], k)


@pytest.mark.parametrize("c", br.REAL_CASES, ids=br.case_id)
def test_train_step_accepts_float32(c):
    shares = br.run_real(br.StandIn(), c)
    print(f"{br.case_id(c)}: worst {max(shares.values()):.3f} | {_fmt(shares)}")


@pytest.mark.parametrize("spec", br.SG_CASES, ids=br.sg_id)
def test_set_grads_accepts_float32(spec):
    print(f"set_grads {br.sg_id(spec)}: worst {br.run_set_grads(br.StandIn(), spec):.3f}")


@pytest.mark.parametrize("spec", br.OS_CASES, ids=lambda s: f"{s[0]}-S{s[1]}")
def test_over_sets_accepts_float32(spec):
    print(f"over_sets {spec[0]}-S{spec[1]}: worst {br.run_over_sets(br.StandIn(), spec):.3f}")


# ---- (d) ---------------------------------------------------------------------------------------
P = lambda heads, R, B: br.Case("planted", heads, R, B)  # noqa: E731
BROKEN_BACKWARD = [
    ("last_argmax", P("ac", 17, 7)),            # duplicates of the maximum on later rows
    ("gs1_no_pool", P("a", 9, 2)),
    ("pool_obs_at_id2", P("ac", 33, 1)),
    ("padding_counted", P("c", 13, 8)),
    ("no_1_over_R", P("c", 5, 1)),
    ("dl1_drops_last_row", P("ac", 65, 1)),
    ("dl1_drops_last_row", P("a", 1, 2)),
    ("g3_of_previous_set", P("ac", 9, 2049)),   # one wave holds two sets
    ("other_half_unwritten", P("a", 16, 7)),
    ("other_half_unwritten", P("c", 16, 7)),
    ("stale_idle_slots", P("ac", 2, 7)),        # one block at work, 255 idle
    ("id_u8", P("ac", 257, 2)),                 # a maximum planted on row 256
]


@pytest.mark.parametrize("bug,c", BROKEN_BACKWARD, ids=lambda v: v if isinstance(v, str) else br.case_id(v))
def test_broken_backward_fails_its_case(bug, c):
    br.run_backward(br.StandIn(), c, repeat=False)
    with pytest.raises(AssertionError):
        br.run_backward(br.StandIn(bug), c, repeat=False)


def test_previous_sets_g3_shows_only_with_two_sets_on_a_wave():
    """Set j's g3 used for set j + 1 changes nothing while every wave holds at most one set."""
    for B in (2047, 2048):
        c = P("ac", 9, B)
        _, a = br.run_backward(br.StandIn(), c, repeat=False)
        _, b = br.run_backward(br.StandIn("g3_of_previous_set"), c, repeat=False)
        br.same_bits(a["wgrad"], b["wgrad"], "wgrad")
        br.same_bits(a["setvec"], b["setvec"], "setvec")
    # ... and with the grid a test hands it: two waves make set 2 the second set of wave 0
    with pytest.raises(AssertionError):
        br.run_backward(br.StandIn("g3_of_previous_set", nwaves=2), P("ac", 9, 7), repeat=False)


def test_stale_slots_show_under_a_dirty_workspace_too():
    c = P("ac", 2, 7)
    with pytest.raises(AssertionError):
        br.run_backward(br.StandIn("stale_idle_slots"), c, ws_fill=1e30, repeat=False)


@pytest.mark.parametrize("spec", [(65, 13, False), (1, 5, True), (513, 7, False)], ids=br.sg_id)
def test_broken_row_sum_fails(spec):
    with pytest.raises(AssertionError):
        br.run_set_grads(br.StandIn("rowsum_tail"), spec)


def test_broken_row_sum_passes_where_the_tail_is_whole():
    br.run_set_grads(br.StandIn("rowsum_tail"), (65, 16, False))
    br.run_set_grads(br.StandIn("rowsum_tail"), (65, 4, False))


@pytest.mark.parametrize("bug,spec", [("os_drop_partial_step", ("L5", 33)), ("os_drop_partial_step", ("L1", 1)),
                                      ("os_drop_partial_step", ("L16b", 2049)), ("os_first_twice", ("L4", 257)),
                                      ("os_first_twice", ("L16a", 4))],
                         ids=lambda v: v if isinstance(v, str) else f"{v[0]}-S{v[1]}")
def test_broken_over_sets_fails(bug, spec):
    with pytest.raises(AssertionError):
        br.run_over_sets(br.StandIn(bug), spec)


def test_dropped_partial_step_passes_whole_steps():
    br.run_over_sets(br.StandIn("os_drop_partial_step"), ("L5", 256))
