"""The host-only side of lb_eval_steps256 and its _supported query (ABI 17, additions): the symbols,
the supported shape -- a property of (cfg, num_envs, num_elements) only, a superset of
lb_eval_steps64_supported -- and every documented refusal, answered before any device call (the
pointers handed over here are not device memory).  No GPU; needs the built library, as
tests/test_steps64_host.py, whose lists these mirror.
"""
import ctypes as C
import inspect
import itertools

import pytest

from test_steps64_host import EVAL_ARGS, EVAL_REQUIRED, _args, _cfg


def test_symbols_and_abi_version():
    from lbk8s import _native
    L = _native.lib()
    for f in ("lb_eval_steps256", "lb_eval_steps256_supported"):
        assert f in _native.STEPS256_SYMBOLS and hasattr(L, f)
        assert getattr(L, f).restype is C.c_int and getattr(L, f).argtypes == _native.STEPS256_PROTOTYPES[f][1]
    assert len(_native.STEPS256_SYMBOLS) == 2
    assert _native.STEPS256_PROTOTYPES["lb_eval_steps256"] == _native.PROTOTYPES["lb_eval_steps"]
    assert _native.STEPS256_PROTOTYPES["lb_eval_steps256_supported"] == _native.PROTOTYPES["lb_eval_steps_supported"]
    assert L.lb_abi_version() == 17 == _native.ABI_VERSION
    assert "lbk8s_steps256.h" in _native.SOURCES and "lbk8s_steps256.hip" in _native.SOURCES
    assert "../../include/lbk8s_abi_steps256.h" in _native.SOURCES


def test_prototypes_match_the_extension_header(monkeypatch):
    """The two prototypes live in include/lbk8s_abi_steps256.h, which include/lbk8s.h includes inside
    its extern "C" block; the header is compared with _native.STEPS256_PROTOTYPES argument by
    argument, as tests/test_native_abi.py compares the main one."""
    import os
    import test_native_abi as t
    from lbk8s import _native
    main = open(t.HEADER).read()
    assert main.index('#include "lbk8s_abi_steps256.h"') < main.rindex("#ifdef __cplusplus")
    monkeypatch.setattr(t, "HEADER", os.path.join(os.path.dirname(t.HEADER), "lbk8s_abi_steps256.h"))
    header = t.header_prototypes()
    assert set(header) == set(t.declared_functions()) == set(_native.STEPS256_SYMBOLS)
    assert t.abi_mismatches(header, _native.STEPS256_PROTOTYPES) == []
    assert header["lb_eval_steps256"][1][4:8] == ["i8", "i4", "ptr", "i4"]  # (the parser itself)
    assert not set(_native.STEPS256_SYMBOLS) & (set(_native.EXPORTED_SYMBOLS) | set(_native.STEPS64_SYMBOLS))


def _rule(E, rej, B, trace, R):
    """include/lbk8s_abi_steps256.h: Philox mode, num_elements the action count, num_envs in
    [1, 32767], the slice layout of 64 lanes with 2 or 4 endpoints per lane (E = 65..256),
    num_elements <= 257."""
    return int(not trace and R == E + int(rej) and 1 <= B <= 32767 and 65 <= E <= 256 and R <= 257)


def test_supported_shape_table():
    from lbk8s import _native
    L = _native.lib()
    seen, new = set(), 0
    for E, rej, B, trace in itertools.product((1, 8, 16, 64, 65, 80, 100, 128, 129, 180, 256), (False, True),
                                              (1, 4096, 32767, 32768), (False, True)):
        c = _cfg(num_endpoints=E, rejection_allowed=rej, trace=trace)
        A = E + int(rej)
        for R in (A - 1, A, A + 1):
            got = L.lb_eval_steps256_supported(C.byref(c), B, R)
            old64 = L.lb_eval_steps64_supported(C.byref(c), B, R)
            assert got == int(bool(old64) or bool(_rule(E, rej, B, trace, R))), (E, rej, B, trace, R)
            if E >= 65:  # the three older queries still say no
                assert old64 == 0 and L.lb_eval_steps_supported(C.byref(c), B, R) == 0
                assert L.lb_ppo_steps64_supported(C.byref(c), B, R) == 0
            new += got - old64
            seen.add(got)
    assert seen == {0, 1} and new > 0
    sup = lambda c, B, R: L.lb_eval_steps256_supported(C.byref(c), B, R)
    assert sup(_cfg(num_endpoints=180, rejection_allowed=True), 2000, 181) == 1   # the sweep's last point
    assert sup(_cfg(num_endpoints=256, rejection_allowed=True), 32767, 257) == 1
    assert sup(_cfg(num_endpoints=64), 4096, 65) == 1 and sup(_cfg(), 8, 9) == 1  # handed on
    assert sup(_cfg(num_endpoints=100, rejection_allowed=False), 0, 100) == 0
    bad = _cfg(num_endpoints=100, rejection_allowed=False)
    bad.num_nodes = 10
    assert sup(bad, 8, 100) == 0


def _unsupported():
    e100 = lambda **kw: _cfg(num_endpoints=100, rejection_allowed=False, **kw)
    return ((e100(), 0, 100), (e100(), 32768, 100), (_cfg(num_endpoints=64), 32768, 65), (e100(trace=True), 8, 100),
            (e100(), 8, 99), (e100(), 8, 101), (_cfg(num_endpoints=100, rejection_allowed=True), 8, 100),
            (_cfg(geometry="tpe"), 8, 9))


def test_eval_steps256_refusals():
    from lbk8s import _native
    L = _native.lib()
    e100 = _cfg(num_endpoints=100, rejection_allowed=False)
    bad = [({k: None}, b"NULL") for k in EVAL_REQUIRED]
    bad += [(dict(B=-3), b"num_envs"),
            (dict(steps=0), b"steps"), (dict(steps=4097), b"steps"), (dict(steps=-1), b"steps"),
            (dict(ep_sum=None), b"ep_sum and ep_cnt"), (dict(ep_cnt=None), b"ep_sum and ep_cnt"),   # one alone
            (dict(ret32=None), b"a log needs"), (dict(count=None), b"a log needs"), (dict(cap=-1), b"a log needs"),
            (dict(R=99), b"lb_eval_steps256_supported"), (dict(R=101), b"lb_eval_steps256_supported")]
    assert L.lb_eval_steps256_supported(C.byref(e100), 16, 100) == 1
    for kw, why in bad:
        if "R" in kw:  # (a shape refusal: never a launch on these pointers)
            assert L.lb_eval_steps256_supported(C.byref(e100), 16, kw["R"]) == 0
        assert L.lb_eval_steps256(*_args(EVAL_ARGS, e100, **dict(dict(R=100), **kw))) < 0, kw
        msg = L.lb_last_error()
        assert msg and b"lb_eval_steps256" in msg and why in msg, (kw, msg)
    # an older shape's refusals carry the new name too (checked before the call is handed on)
    for cfg, R in ((_cfg(num_endpoints=6, rejection_allowed=True), 7), (_cfg(num_endpoints=64), 64)):
        for kw in (dict(frag=None), dict(steps=0), dict(ep_cnt=None), dict(cap=-1)):
            assert L.lb_eval_steps256(*_args(EVAL_ARGS, cfg, B=8, R=R, **kw)) < 0, kw
            assert b"lb_eval_steps256" in L.lb_last_error(), kw
    for cfg, B, R in _unsupported():
        assert L.lb_eval_steps256_supported(cfg, B, R) == 0, (B, R)
        assert L.lb_eval_steps256(*_args(EVAL_ARGS, cfg, B=B, R=R)) < 0, (B, R)
        msg = L.lb_last_error()
        assert b"lb_eval_steps256" in msg and (b"lb_eval_steps256_supported" in msg or (B < 1 and b"num_envs" in msg))
        with pytest.raises(RuntimeError, match="lb_eval_steps256"):
            _native.check(L.lb_eval_steps256(*_args(EVAL_ARGS, cfg, B=B, R=R)))
    invalid = _cfg(num_endpoints=100, rejection_allowed=False)
    invalid.episode_length = 0
    assert L.lb_eval_steps256(*_args(EVAL_ARGS, invalid, R=100)) < 0 and L.lb_last_error()


def test_new_flags_default_off():
    from lbk8s import cli, evaluate
    assert inspect.signature(evaluate.run_test).parameters["e256"].default is False
    assert inspect.signature(evaluate.run_test).parameters["e64"].default is False
    sw = inspect.signature(evaluate.run_sweep).parameters
    assert sw["num_endpoints"].default == evaluate.SWEEP_ENDPOINTS == (6, 12, 16, 24, 32, 48, 64, 80, 128, 150, 180)
    assert (sw["n_episodes"].default, sw["seed"].default, sw["out_dir"].default) == (2000, 42, None)
    assert sw["fused"].default is False and sw["e64"].default is False and sw["e256"].default is False
    args = cli.build_parser().parse_args([])
    assert args.test_fused_e256 is False and args.test_sweep is None
    assert args.test_fused_e64 is False and args.test_fused is False
