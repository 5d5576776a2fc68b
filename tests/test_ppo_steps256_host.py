"""The host-only side of lb_ppo_steps256 and lb_ppo_steps256_supported (ABI 17, additions): the
symbols, the supported shape -- a property of (cfg, num_envs, num_elements) only, lb_ppo_steps64's
OR lb_eval_steps256's -- and every documented refusal, answered before any device call (the
pointers handed over here are not device memory).  No GPU; needs the built library, as
tests/test_steps64_host.py, whose lists these mirror.
"""
import ctypes as C
import inspect
import itertools

import pytest

from test_steps64_host import PPO_ARGS, PPO_REQUIRED, _args, _cfg


def test_symbols_and_abi_version():
    from lbk8s import _native
    L = _native.lib()
    for f in ("lb_ppo_steps256", "lb_ppo_steps256_supported"):
        assert f in _native.PPO256_SYMBOLS and hasattr(L, f)
        assert getattr(L, f).restype is C.c_int and getattr(L, f).argtypes == _native.PPO256_PROTOTYPES[f][1]
    assert len(_native.PPO256_SYMBOLS) == 2
    assert _native.PPO256_PROTOTYPES["lb_ppo_steps256"] == _native.PROTOTYPES["lb_ppo_steps"]
    assert _native.PPO256_PROTOTYPES["lb_ppo_steps256_supported"] == _native.PROTOTYPES["lb_ppo_steps_supported"]
    assert L.lb_abi_version() == 17 == _native.ABI_VERSION
    for f in ("lbk8s_ppo256.h", "../../include/lbk8s_abi_ppo256.h", "lbk8s_steps256.hip"):
        assert f in _native.SOURCES
    assert _native.source_hash() == L.lb_source_hash().decode()  # (csrc/Makefile's SRCS lists them too)


def test_prototypes_match_the_extension_header(monkeypatch):
    """The two prototypes live in include/lbk8s_abi_ppo256.h, which include/lbk8s.h includes inside
    its extern "C" block, last.  The comparison of tests/test_native_abi.py, argument by argument,
    of that header with _native.PPO256_PROTOTYPES."""
    import os
    import test_native_abi as t
    from lbk8s import _native
    main = open(t.HEADER).read()
    assert (main.index('#include "lbk8s_abi_steps64.h"') < main.index('#include "lbk8s_abi_dqn64.h"')
            < main.index('#include "lbk8s_abi_steps256.h"') < main.index('#include "lbk8s_abi_dqn256.h"')
            < main.index('#include "lbk8s_abi_ppo256.h"') < main.rindex("#ifdef __cplusplus"))
    assert main.count("#include \"lbk8s_abi_") == 5  # (the last of them)
    monkeypatch.setattr(t, "HEADER", os.path.join(os.path.dirname(t.HEADER), "lbk8s_abi_ppo256.h"))
    header = t.header_prototypes()
    assert set(header) == set(t.declared_functions()) == set(_native.PPO256_SYMBOLS)
    assert t.abi_mismatches(header, _native.PPO256_PROTOTYPES) == []
    assert header["lb_ppo_steps256"][1][4:8] == ["i8", "i4", "i4", "i4"]  # (the parser itself)
    others = (set(_native.EXPORTED_SYMBOLS) | set(_native.STEPS64_SYMBOLS) | set(_native.DQN64_SYMBOLS)
              | set(_native.STEPS256_SYMBOLS) | set(_native.DQN256_SYMBOLS))
    assert not set(_native.PPO256_SYMBOLS) & others


def _rule(E, rej, B, trace, R):
    """The steps256 rule: Philox mode, num_elements the action count, num_envs in [1, 32767], the
    slice layout of 64 lanes with 2 or 4 endpoints per lane (E = 65..256), num_elements <= 257."""
    return int(not trace and R == E + int(rej) and 1 <= B <= 32767 and 65 <= E <= 256 and R <= 257)


def test_supported_shape_table():
    from lbk8s import _native
    L = _native.lib()
    seen, new = set(), 0
    for E, rej, B, trace in itertools.product((6, 16, 64, 65, 80, 128, 129, 256), (False, True), (1, 32767, 32768),
                                              (False, True)):
        c = _cfg(num_endpoints=E, rejection_allowed=rej, trace=trace)
        A = E + int(rej)
        for R in (A - 1, A, A + 1):  # (R that is not the action count on either side)
            got = L.lb_ppo_steps256_supported(C.byref(c), B, R)
            old = L.lb_ppo_steps64_supported(C.byref(c), B, R)
            assert got == (old | L.lb_eval_steps256_supported(C.byref(c), B, R)), (E, rej, B, trace, R)
            assert got == (old | _rule(E, rej, B, trace, R)), (E, rej, B, trace, R)
            new += got - old
            seen.add(got)
    assert seen == {0, 1} and new > 0
    sup = lambda c, B, R: L.lb_ppo_steps256_supported(C.byref(c), B, R)
    old = lambda c, B, R: L.lb_ppo_steps64_supported(C.byref(c), B, R)
    for E, rej in ((65, False), (65, True), (80, False), (80, True), (128, True), (129, False), (180, True), (256, True)):
        c = _cfg(num_endpoints=E, rejection_allowed=rej)
        assert sup(c, 4096, E + int(rej)) == 1 and old(c, 4096, E + int(rej)) == 0, (E, rej)
        assert sup(c, 0, E + int(rej)) == 0 and sup(c, 32768, E + int(rej)) == 0, (E, rej)
    e64 = _cfg(num_endpoints=64, rejection_allowed=True)
    assert sup(e64, 4096, 65) == 1 == old(e64, 4096, 65)
    e16 = _cfg(num_endpoints=16, rejection_allowed=False)
    assert sup(e16, 32768, 16) == 1 == L.lb_ppo_steps_supported(C.byref(e16), 32768, 16)  # (16 lanes at any batch)
    bad = _cfg(num_endpoints=128)
    bad.num_nodes = 10
    assert sup(bad, 8, 129) == 0


def test_ppo_steps256_refusals():
    """tests/test_steps64_host.py's list under the new name, on a new shape (E = 180 with the reject
    row), on an E = 64 shape and on a 16-lane shape: checked before the call is handed on."""
    from lbk8s import _native
    L = _native.lib()
    bad = [({k: None}, b"NULL") for k in PPO_REQUIRED]
    bad += [(dict(B=0), b"num_envs"), (dict(B=-3), b"num_envs"),
            (dict(steps=0, store_rows=0), b"steps"), (dict(steps=4097, store_rows=4097), b"steps"),
            (dict(steps=4097, store_rows=4096), b"steps"), (dict(steps=-1, store_rows=-1), b"steps"),
            (dict(store_rows=3), b"store_rows"), (dict(store_rows=6), b"store_rows"), (dict(store_rows=-1), b"store_rows"),
            (dict(last_obs=None), b"last_obs"), (dict(last_done=None), b"last_obs"),      # store_rows == steps - 1
            (dict(steps=1, store_rows=0, last_obs=None), b"last_obs"),
            (dict(steps=1, store_rows=0, last_done=None), b"last_obs"),
            (dict(ep_sum=None), b"ep_sum and ep_cnt"), (dict(ep_cnt=None), b"ep_sum and ep_cnt"),  # one alone
            (dict(ret32=None), b"a log needs"), (dict(count=None), b"a log needs"), (dict(cap=-1), b"a log needs"),
            (dict(dR=-1), b"lb_ppo_steps256_supported"), (dict(dR=1), b"lb_ppo_steps256_supported")]  # not the action count
    e180 = _cfg(num_endpoints=180, rejection_allowed=True)
    e64 = _cfg(num_endpoints=64)
    e6 = _cfg(num_endpoints=6, rejection_allowed=True)
    for cfg, B, R in ((e180, 16, 181), (e64, 16, 65), (e6, 8, 7)):
        for kw, why in bad:
            kw = dict(kw)
            kw = dict(dict(B=B, R=R + kw.pop("dR", 0)), **kw)
            assert L.lb_ppo_steps256(*_args(PPO_ARGS, cfg, **kw)) < 0, kw
            msg = L.lb_last_error()
            assert msg and b"lb_ppo_steps256" in msg and why in msg, (kw, msg)
    # outside the superset (a config holds at most 256 endpoints): 32,768 envs, trace mode, the
    # thread-per-env layout
    for cfg, B, R in ((e180, 32768, 181), (_cfg(num_endpoints=256, rejection_allowed=True), 32768, 257),
                      (_cfg(num_endpoints=64), 32768, 65), (_cfg(), 32768, 9),
                      (_cfg(num_endpoints=180, rejection_allowed=True, trace=True), 8, 181),
                      (_cfg(num_endpoints=64, trace=True), 8, 65), (_cfg(geometry="tpe"), 8, 9)):
        assert L.lb_ppo_steps256(*_args(PPO_ARGS, cfg, B=B, R=R)) < 0, (B, R)
        assert b"lb_ppo_steps256_supported" in L.lb_last_error(), (B, R)
        with pytest.raises(RuntimeError, match="lb_ppo_steps256_supported"):
            _native.check(L.lb_ppo_steps256(*_args(PPO_ARGS, cfg, B=B, R=R)))
    invalid = _cfg(num_endpoints=180, rejection_allowed=True)
    invalid.episode_length = 0
    assert L.lb_ppo_steps256(*_args(PPO_ARGS, invalid, R=181)) < 0 and L.lb_last_error()


def test_new_flags_default_off():
    from lbk8s import cli
    from lbk8s.ppo import PPO_DeepSets
    assert inspect.signature(PPO_DeepSets).parameters["fused_rollout_e256"].default is False
    args = cli.build_parser().parse_args([])
    assert args.fused_rollout_e256 is False and args.fused_rollout_e64 is False and args.fused_rollout is False
    on = cli.build_parser().parse_args(["--fused-rollout-e256"])
    assert on.fused_rollout_e256 is True
    assert on.fused_rollout_e64 is False and on.fused_rollout is False and on.dqn_steps_e256 is False
    import importlib.util
    import os
    import sys
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "rl_bench.py")
    spec = importlib.util.spec_from_file_location("rl_bench_for_ppo256", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    argv = sys.argv
    try:
        sys.argv = ["rl_bench.py"]
        off = mod.parse()
        assert off.fused_rollout_e256 is False and off.fused_rollout_e64 is False and off.endpoints is None
        sys.argv = ["rl_bench.py", "--algo", "ppo", "--fused-rollout-e256", "--endpoints", "180"]
        got = mod.parse()
        assert got.fused_rollout_e256 is True and got.fused_rollout_e64 is False and got.endpoints == 180
    finally:
        sys.argv = argv
