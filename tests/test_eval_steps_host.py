"""The host-only side of lb_eval_steps / lb_eval_steps_supported (ABI 17, additions): the symbols,
the supported shape (a property of (cfg, num_envs, num_elements) only: lb_ppo_steps_supported's
answer) and every documented refusal, answered before any device call (the pointers handed over
here are not device memory).  No GPU; needs the built library, as tests/test_ppo_steps_host.py.
"""
import ctypes as C
import inspect
import itertools

import pytest

FAKE = 4096  # never dereferenced: a refused call makes no device call


def _cfg(**kw):
    from lbk8s import LBConfig
    trace = kw.pop("trace", False)
    return LBConfig(**kw).to_c(0, 0, True, trace, "auto")


def test_symbols_and_abi_version():
    from lbk8s import _native
    L = _native.lib()
    for f in ("lb_eval_steps", "lb_eval_steps_supported"):
        assert f in _native.EXPORTED_SYMBOLS and hasattr(L, f)
        assert getattr(L, f).restype is C.c_int
    assert L.lb_abi_version() == 17 == _native.ABI_VERSION
    assert "lbk8s_eval.h" in _native.SOURCES
    assert _native.LB_EVAL_STEPS_MAX == 4096


def test_supported_is_ppo_steps_supported():
    from lbk8s import _native
    L = _native.lib()
    seen = set()
    for E, rej, B, trace in itertools.product((1, 6, 8, 15, 16, 17, 64), (False, True), (1, 8, 4096, 32767, 32768),
                                              (False, True)):
        c = _cfg(num_endpoints=E, rejection_allowed=rej, trace=trace)
        A = E + int(rej)
        for R in (A - 1, A, A + 1):
            got = L.lb_eval_steps_supported(C.byref(c), B, R)
            assert got == L.lb_ppo_steps_supported(C.byref(c), B, R), (E, rej, B, trace, R)
            if trace or R != A or R > 16:  # Philox only, the env's action count, at most 16 rows
                assert got == 0, (E, rej, B, trace, R)
            seen.add(got)
    assert seen == {0, 1}
    sup = lambda c, B, R: L.lb_eval_steps_supported(C.byref(c), B, R)
    e6 = _cfg(num_endpoints=6, rejection_allowed=True)
    assert sup(e6, 8, 7) == 1 and sup(e6, 2000, 7) == 1                       # run.py's shape, run_test's
    assert sup(_cfg(num_endpoints=16, rejection_allowed=False), 67, 16) == 1
    assert sup(_cfg(), 4096, 9) == 1 and sup(_cfg(), 1, 9) == 1 and sup(_cfg(), 32767, 9) == 1
    assert sup(_cfg(num_endpoints=64), 16, 65) == 0                           # 64 lanes per env
    assert sup(_cfg(), 32768, 9) == 0                                         # thread-per-env layout
    assert L.lb_eval_steps_supported(C.byref(e6), 0, 7) == 0
    bad = _cfg()
    bad.num_nodes = 10
    assert L.lb_eval_steps_supported(C.byref(bad), 8, 9) == 0


ARGS = ("frag", "obs", "state", "cfg", "B", "R", "masks", "steps", "actions_all", "rewards_all", "dones_all",
        "actions_out", "reward_out", "done_out", "ep_stats_out", "ep_sum", "ep_cnt", "ret32", "ep_r32", "tag0", "log",
        "cap", "count", "stream")
REQUIRED = ("frag", "obs", "state", "actions_out", "reward_out", "done_out", "ep_stats_out")


def _args(cfg, **kw):
    a = {k: FAKE + 64 * i for i, k in enumerate(ARGS)}
    a.update(cfg=C.byref(cfg), B=8, R=7, steps=5, ep_r32=None, tag0=0, cap=8, stream=None)
    a.update(kw)
    return [a[k] for k in ARGS]


def test_eval_steps_refusals():
    from lbk8s import _native
    L = _native.lib()
    e6 = _cfg(num_endpoints=6, rejection_allowed=True)
    bad = [({k: None}, b"NULL") for k in REQUIRED]
    bad += [(dict(B=0), b"num_envs"), (dict(B=-3), b"num_envs"),
            (dict(steps=0), b"steps"), (dict(steps=4097), b"steps"), (dict(steps=-1), b"steps"),
            (dict(ep_sum=None), b"ep_sum and ep_cnt"), (dict(ep_cnt=None), b"ep_sum and ep_cnt"),   # one alone
            (dict(ret32=None), b"a log needs"), (dict(count=None), b"a log needs"), (dict(cap=-1), b"a log needs"),
            (dict(R=6), b"lb_eval_steps_supported"), (dict(R=8), b"lb_eval_steps_supported")]  # not the action count
    for kw, why in bad:
        assert L.lb_eval_steps(*_args(e6, **kw)) < 0, kw
        msg = L.lb_last_error()
        assert msg and b"lb_eval_steps" in msg and why in msg, (kw, msg)
    # the unsupported shapes, by name
    for cfg, B, R in ((_cfg(num_endpoints=16, rejection_allowed=True), 67, 17), (_cfg(num_endpoints=64), 16, 65),
                      (_cfg(), 32768, 9), (_cfg(trace=True), 8, 9)):
        assert L.lb_eval_steps(*_args(cfg, B=B, R=R)) < 0, (B, R)
        assert b"lb_eval_steps_supported" in L.lb_last_error(), (B, R)
        with pytest.raises(RuntimeError, match="lb_eval_steps_supported"):
            _native.check(L.lb_eval_steps(*_args(cfg, B=B, R=R)))
    invalid = _cfg()
    invalid.episode_length = 0
    assert L.lb_eval_steps(*_args(invalid, R=9)) < 0 and L.lb_last_error()


def test_fused_evaluation_defaults_off():
    from lbk8s import cli, evaluate
    p = inspect.signature(evaluate.run_test).parameters
    assert p["fused"].default is False and p["return_trace"].default is False
    assert cli.build_parser().parse_args([]).test_fused is False
    assert cli.build_parser().parse_args(["--test-fused"]).test_fused is True
