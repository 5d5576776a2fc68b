"""The host-only side of lb_ppo_steps64 / lb_eval_steps64 and their _supported queries (ABI 17,
additions): the symbols, the supported shape -- a property of (cfg, num_envs, num_elements) only,
a superset of lb_ppo_steps_supported -- and every documented refusal, answered before any device
call (the pointers handed over here are not device memory).  No GPU; needs the built library, as
tests/test_ppo_steps_host.py and tests/test_eval_steps_host.py, whose lists these mirror.
"""
import ctypes as C
import inspect
import itertools

import pytest

FAKE = 4096  # never dereferenced: a refused call makes no device call


def _cfg(**kw):
    from lbk8s import LBConfig
    trace = kw.pop("trace", False)
    geometry = kw.pop("geometry", "auto")
    return LBConfig(**kw).to_c(0, 0, True, trace, geometry)


def test_symbols_and_abi_version():
    from lbk8s import _native
    L = _native.lib()
    for f in ("lb_ppo_steps64", "lb_ppo_steps64_supported", "lb_eval_steps64", "lb_eval_steps64_supported"):
        assert f in _native.STEPS64_SYMBOLS and hasattr(L, f)
        assert getattr(L, f).restype is C.c_int and getattr(L, f).argtypes == _native.STEPS64_PROTOTYPES[f][1]
    assert len(_native.STEPS64_SYMBOLS) == 4
    assert _native.STEPS64_PROTOTYPES["lb_ppo_steps64"] == _native.PROTOTYPES["lb_ppo_steps"]
    assert _native.STEPS64_PROTOTYPES["lb_eval_steps64"] == _native.PROTOTYPES["lb_eval_steps"]
    assert L.lb_abi_version() == 17 == _native.ABI_VERSION
    assert "lbk8s_steps64.h" in _native.SOURCES and "lbk8s_steps64.hip" in _native.SOURCES
    assert "../../include/lbk8s_abi_steps64.h" in _native.SOURCES


def test_prototypes_match_the_extension_header(monkeypatch):
    """The four prototypes live in include/lbk8s_abi_steps64.h, which include/lbk8s.h includes (the
    main header's own list and its table in the binding stay as tests/test_native_abi.py pins
    them).  The same comparison as there, argument by argument, of that header with
    _native.STEPS64_PROTOTYPES; and lbk8s.h does include it, inside its extern "C" block."""
    import os
    import test_native_abi as t
    from lbk8s import _native
    main = open(t.HEADER).read()
    assert main.index('#include "lbk8s_abi_steps64.h"') < main.rindex("#ifdef __cplusplus")
    monkeypatch.setattr(t, "HEADER", os.path.join(os.path.dirname(t.HEADER), "lbk8s_abi_steps64.h"))
    header = t.header_prototypes()
    assert set(header) == set(t.declared_functions()) == set(_native.STEPS64_SYMBOLS)
    assert t.abi_mismatches(header, _native.STEPS64_PROTOTYPES) == []
    assert header["lb_ppo_steps64"][1][4:8] == ["i8", "i4", "i4", "i4"]  # (the parser itself)
    assert not set(_native.STEPS64_SYMBOLS) & set(_native.EXPORTED_SYMBOLS)


def _rule(E, rej, B, trace, R):
    """Issue / include/lbk8s.h: Philox mode, num_elements the action count, num_envs in [1, 32767],
    the slice layout with one endpoint per lane (below 32,768 envs: E <= 64), num_elements <= 65."""
    return int(not trace and R == E + int(rej) and 1 <= B <= 32767 and E <= 64 and R <= 65)


def test_supported_shape_table():
    from lbk8s import _native
    L = _native.lib()
    seen, beyond, new = set(), set(), 0
    for E, rej, B, trace in itertools.product((1, 6, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100), (False, True),
                                              (1, 8, 4096, 32767, 32768), (False, True)):
        c = _cfg(num_endpoints=E, rejection_allowed=rej, trace=trace)
        A = E + int(rej)
        for R in (A - 1, A, A + 1):
            got = L.lb_ppo_steps64_supported(C.byref(c), B, R)
            assert got == L.lb_eval_steps64_supported(C.byref(c), B, R), (E, rej, B, trace, R)
            old = L.lb_ppo_steps_supported(C.byref(c), B, R)
            assert old == L.lb_eval_steps_supported(C.byref(c), B, R)
            assert got >= old, (E, rej, B, trace, R)  # a superset
            # The rule, except where it and the superset cannot both hold: lb_ppo_steps_supported is
            # 1 for E = 9..16 at 32,768 envs too (16 lanes per env at every batch size), where the
            # rule's num_envs <= 32767 says 0; the old answer wins there (the same kernel runs).
            if got != _rule(E, rej, B, trace, R):
                assert got == old == 1 and B == 32768 and 9 <= E <= 16, (E, rej, B, trace, R)
                beyond.add((E, rej))
            new += got - old
            seen.add(got)
    assert seen == {0, 1} and new > 0
    assert beyond == {(15, False), (15, True), (16, False)}  # (E = 16 with the reject row: R = 17, new only)
    sup = lambda c, B, R: (L.lb_ppo_steps64_supported(C.byref(c), B, R), L.lb_eval_steps64_supported(C.byref(c), B, R))
    assert sup(_cfg(num_endpoints=64), 4096, 65) == (1, 1)                                   # config 4
    assert sup(_cfg(num_endpoints=16, rejection_allowed=True), 67, 17) == (1, 1)           # R = 17 on 16 lanes
    assert sup(_cfg(num_endpoints=64), 0, 65) == (0, 0)
    for E in (1, 6, 8):  # the thread-per-env layout, pinned by the config
        assert sup(_cfg(num_endpoints=E, geometry="tpe"), 8, E + 1) == (0, 0)
        assert sup(_cfg(num_endpoints=E, geometry="slice"), 8, E + 1) == (1, 1)
    bad = _cfg(num_endpoints=64)
    bad.num_nodes = 10
    assert sup(bad, 8, 65) == (0, 0)


PPO_ARGS = ("frag", "obs", "state", "cfg", "B", "R", "steps", "store_rows", "uniforms", "actions_f32", "logprobs",
            "values", "rewards", "obs_next", "dones_next", "last_obs", "last_done", "actions_out", "done_out",
            "ep_stats_out", "ep_sum", "ep_cnt", "ret32", "ep_r32", "tag0", "log", "cap", "count", "stream")
PPO_REQUIRED = ("frag", "obs", "state", "uniforms", "actions_f32", "logprobs", "values", "rewards", "obs_next",
                "dones_next", "actions_out", "done_out", "ep_stats_out")
EVAL_ARGS = ("frag", "obs", "state", "cfg", "B", "R", "masks", "steps", "actions_all", "rewards_all", "dones_all",
             "actions_out", "reward_out", "done_out", "ep_stats_out", "ep_sum", "ep_cnt", "ret32", "ep_r32", "tag0",
             "log", "cap", "count", "stream")
EVAL_REQUIRED = ("frag", "obs", "state", "actions_out", "reward_out", "done_out", "ep_stats_out")


def _args(names, cfg, **kw):
    a = {k: FAKE + 64 * i for i, k in enumerate(names)}
    a.update(cfg=C.byref(cfg), B=16, R=65, steps=5, store_rows=4, ep_r32=None, tag0=0, cap=16, stream=None)
    a.update(kw)
    return [a[k] for k in names]


# outside the superset: E > 64, 32,768 envs, trace mode, the thread-per-env layout
def _unsupported():
    return ((_cfg(num_endpoints=65), 16, 66), (_cfg(num_endpoints=100), 16, 101), (_cfg(num_endpoints=64), 32768, 65),
            (_cfg(), 32768, 9), (_cfg(num_endpoints=64, trace=True), 8, 65), (_cfg(geometry="tpe"), 8, 9))


def test_ppo_steps64_refusals():
    from lbk8s import _native
    L = _native.lib()
    e64 = _cfg(num_endpoints=64)
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
            (dict(R=64), b"lb_ppo_steps64_supported"), (dict(R=66), b"lb_ppo_steps64_supported")]  # not the action count
    for kw, why in bad:
        assert L.lb_ppo_steps64(*_args(PPO_ARGS, e64, **kw)) < 0, kw
        msg = L.lb_last_error()
        assert msg and b"lb_ppo_steps64" in msg and why in msg, (kw, msg)
    # a 16-lane shape's refusals carry the new name too (checked before the call is handed on)
    e6 = _cfg(num_endpoints=6, rejection_allowed=True)
    for kw in (dict(frag=None), dict(store_rows=3), dict(ep_cnt=None), dict(cap=-1)):
        assert L.lb_ppo_steps64(*_args(PPO_ARGS, e6, B=8, R=7, **kw)) < 0, kw
        assert b"lb_ppo_steps64" in L.lb_last_error(), kw
    for cfg, B, R in _unsupported():
        assert L.lb_ppo_steps64(*_args(PPO_ARGS, cfg, B=B, R=R)) < 0, (B, R)
        assert b"lb_ppo_steps64_supported" in L.lb_last_error(), (B, R)
        with pytest.raises(RuntimeError, match="lb_ppo_steps64_supported"):
            _native.check(L.lb_ppo_steps64(*_args(PPO_ARGS, cfg, B=B, R=R)))
    invalid = _cfg(num_endpoints=64)
    invalid.episode_length = 0
    assert L.lb_ppo_steps64(*_args(PPO_ARGS, invalid)) < 0 and L.lb_last_error()


def test_eval_steps64_refusals():
    from lbk8s import _native
    L = _native.lib()
    e64 = _cfg(num_endpoints=64)
    bad = [({k: None}, b"NULL") for k in EVAL_REQUIRED]
    bad += [(dict(B=0), b"num_envs"), (dict(B=-3), b"num_envs"),
            (dict(steps=0), b"steps"), (dict(steps=4097), b"steps"), (dict(steps=-1), b"steps"),
            (dict(ep_sum=None), b"ep_sum and ep_cnt"), (dict(ep_cnt=None), b"ep_sum and ep_cnt"),   # one alone
            (dict(ret32=None), b"a log needs"), (dict(count=None), b"a log needs"), (dict(cap=-1), b"a log needs"),
            (dict(R=64), b"lb_eval_steps64_supported"), (dict(R=66), b"lb_eval_steps64_supported")]
    for kw, why in bad:
        assert L.lb_eval_steps64(*_args(EVAL_ARGS, e64, **kw)) < 0, kw
        msg = L.lb_last_error()
        assert msg and b"lb_eval_steps64" in msg and why in msg, (kw, msg)
    e6 = _cfg(num_endpoints=6, rejection_allowed=True)
    for kw in (dict(frag=None), dict(steps=0), dict(ep_cnt=None), dict(cap=-1)):
        assert L.lb_eval_steps64(*_args(EVAL_ARGS, e6, B=8, R=7, **kw)) < 0, kw
        assert b"lb_eval_steps64" in L.lb_last_error(), kw
    for cfg, B, R in _unsupported():
        assert L.lb_eval_steps64(*_args(EVAL_ARGS, cfg, B=B, R=R)) < 0, (B, R)
        assert b"lb_eval_steps64_supported" in L.lb_last_error(), (B, R)
        with pytest.raises(RuntimeError, match="lb_eval_steps64_supported"):
            _native.check(L.lb_eval_steps64(*_args(EVAL_ARGS, cfg, B=B, R=R)))
    invalid = _cfg(num_endpoints=64)
    invalid.episode_length = 0
    assert L.lb_eval_steps64(*_args(EVAL_ARGS, invalid)) < 0 and L.lb_last_error()


def test_new_flags_default_off():
    from lbk8s import cli, evaluate
    from lbk8s.ppo import PPO_DeepSets
    assert inspect.signature(PPO_DeepSets).parameters["fused_rollout_e64"].default is False
    assert inspect.signature(evaluate.run_test).parameters["e64"].default is False
    args = cli.build_parser().parse_args([])
    assert args.fused_rollout_e64 is False and args.test_fused_e64 is False
    assert args.fused_rollout is False and args.test_fused is False
    on = cli.build_parser().parse_args(["--fused-rollout-e64", "--test-fused-e64"])
    assert on.fused_rollout_e64 is True and on.test_fused_e64 is True
    assert on.fused_rollout is False and on.test_fused is False  # (the old flags keep their meaning)
