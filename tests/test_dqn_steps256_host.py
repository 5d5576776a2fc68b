"""The host-only side of lb_dqn_steps256 and lb_dqn_steps256_supported (ABI 17, additions): the
symbols, the supported shape -- a property of (cfg, num_envs, num_elements) only, a superset of
lb_dqn_steps64_supported -- and every documented refusal, answered before any device call (the
pointers handed over here are not device memory).  No GPU; needs the built library, as
tests/test_dqn_steps64_host.py, whose lists these mirror.
"""
import ctypes as C
import inspect
import itertools

import pytest

from test_dqn_steps64_host import DQN_ARGS, DQN_REQUIRED, FAKE, _cfg, _explore


def test_symbols_and_abi_version():
    from lbk8s import _native
    L = _native.lib()
    for f in ("lb_dqn_steps256", "lb_dqn_steps256_supported"):
        assert f in _native.DQN256_SYMBOLS and hasattr(L, f)
        assert getattr(L, f).restype is C.c_int and getattr(L, f).argtypes == _native.DQN256_PROTOTYPES[f][1]
    assert len(_native.DQN256_SYMBOLS) == 2
    assert _native.DQN256_PROTOTYPES["lb_dqn_steps256"] == _native.PROTOTYPES["lb_dqn_steps"]
    assert _native.DQN256_PROTOTYPES["lb_dqn_steps256_supported"] == _native.PROTOTYPES["lb_dqn_steps_supported"]
    assert L.lb_abi_version() == 17 == _native.ABI_VERSION
    for f in ("lbk8s_dqn256.h", "../../include/lbk8s_abi_dqn256.h", "lbk8s_steps256.hip"):
        assert f in _native.SOURCES
    assert _native.source_hash() == L.lb_source_hash().decode()  # (csrc/Makefile's SRCS lists them too)


def test_prototypes_match_the_extension_header(monkeypatch):
    """The two prototypes live in include/lbk8s_abi_dqn256.h, which include/lbk8s.h includes inside
    its extern "C" block, after lbk8s_abi_steps256.h.  The comparison of tests/test_native_abi.py,
    argument by argument, of that header with _native.DQN256_PROTOTYPES."""
    import os
    import test_native_abi as t
    from lbk8s import _native
    main = open(t.HEADER).read()
    assert (main.index('#include "lbk8s_abi_steps64.h"') < main.index('#include "lbk8s_abi_dqn64.h"')
            < main.index('#include "lbk8s_abi_steps256.h"') < main.index('#include "lbk8s_abi_dqn256.h"')
            < main.rindex("#ifdef __cplusplus"))
    monkeypatch.setattr(t, "HEADER", os.path.join(os.path.dirname(t.HEADER), "lbk8s_abi_dqn256.h"))
    header = t.header_prototypes()
    assert set(header) == set(t.declared_functions()) == set(_native.DQN256_SYMBOLS)
    assert t.abi_mismatches(header, _native.DQN256_PROTOTYPES) == []
    assert header["lb_dqn_steps256"][1][2:4] == ["i8", "i4"] and header["lb_dqn_steps256"][1][-3] == "i4"  # (the parser)
    others = (set(_native.EXPORTED_SYMBOLS) | set(_native.STEPS64_SYMBOLS) | set(_native.DQN64_SYMBOLS)
              | set(_native.STEPS256_SYMBOLS))
    assert not set(_native.DQN256_SYMBOLS) & others


def _rule(E, rej, B, trace, R):
    """The steps256 rule: Philox mode, num_elements the action count, num_envs in [1, 32767], the
    slice layout of 64 lanes with 2 or 4 endpoints per lane (E = 65..256), num_elements <= 257."""
    return int(not trace and R == E + int(rej) and 1 <= B <= 32767 and 65 <= E <= 256 and R <= 257)


def test_supported_shape_table():
    from lbk8s import _native
    L = _native.lib()
    seen, new = set(), 0
    for E, rej, B, trace in itertools.product((6, 16, 64, 65, 80, 81, 128, 129, 180, 256), (False, True),
                                              (1, 8, 4096, 32767, 32768), (False, True)):
        c = _cfg(num_endpoints=E, rejection_allowed=rej, trace=trace)
        A = E + int(rej)
        for R in (A - 1, A, A + 1):
            got = L.lb_dqn_steps256_supported(C.byref(c), B, R)
            old = L.lb_dqn_steps64_supported(C.byref(c), B, R)
            assert got == (old | _rule(E, rej, B, trace, R)), (E, rej, B, trace, R)  # lb_dqn_steps64's OR the rule
            assert got == (L.lb_dqn_steps_supported(C.byref(c), B, R)
                           | L.lb_eval_steps256_supported(C.byref(c), B, R)), (E, rej, B, trace, R)
            new += got - old
            seen.add(got)
    assert seen == {0, 1} and new > 0
    sup = lambda c, B, R: L.lb_dqn_steps256_supported(C.byref(c), B, R)
    old = lambda c, B, R: L.lb_dqn_steps64_supported(C.byref(c), B, R)
    for E, rej in ((65, True), (80, False), (80, True), (128, True), (129, False), (180, True), (256, True)):
        c = _cfg(num_endpoints=E, rejection_allowed=rej)
        assert sup(c, 4096, E + int(rej)) == 1 and old(c, 4096, E + int(rej)) == 0, (E, rej)
        assert sup(c, 0, E + int(rej)) == 0 and sup(c, 32768, E + int(rej)) == 0, (E, rej)
    e64 = _cfg(num_endpoints=64, rejection_allowed=True)
    assert sup(e64, 4096, 65) == 1 == old(e64, 4096, 65)
    bad = _cfg(num_endpoints=128)
    bad.num_nodes = 10
    assert sup(bad, 8, 129) == 0


def _args(_native, cfg, keep, **kw):
    a = {k: FAKE + 64 * i for i, k in enumerate(DQN_ARGS)}
    ex = _explore(_native)
    keep.append(ex)
    a.update(cfg=C.byref(cfg), ex=C.byref(ex), B=16, R=181, slots=4, steps=5, stream=None)
    a.update(kw)
    return [a[k] for k in DQN_ARGS]


def test_dqn_steps256_refusals():
    from lbk8s import _native
    L = _native.lib()
    keep = []
    e180 = _cfg(num_endpoints=180, rejection_allowed=True)
    bad = [({k: None}, b"NULL") for k in DQN_REQUIRED]
    bad += [(dict(B=0), b"num_envs"), (dict(B=-3), b"num_envs"), (dict(slots=0), b"replay"),
            (dict(steps=0), b"steps must be in [1, 32]"), (dict(steps=33), b"steps must be in [1, 32]"),
            (dict(steps=-1), b"steps must be in [1, 32]"), (dict(sync=None), b"sync"),
            (dict(ep_sum=None), b"ep_sum"), (dict(ep_cnt=None), b"ep_sum"), (dict(ep_stats_out=None), b"ep_sum"),
            (dict(R=180), b"action count"), (dict(R=182), b"action count")]
    for word in ("vin", "vout", "flag"):
        ex = _explore(_native, **{word: None})
        keep.append(ex)
        bad.append((dict(ex=C.byref(ex)), b"device words"))
    # the whole list on a new shape, on a 16-lane shape and on an E = 64 shape: the new name each
    # time (checked before the call is handed on)
    e6 = _cfg(num_endpoints=6, rejection_allowed=True)
    e64 = _cfg(num_endpoints=64, rejection_allowed=True)
    for cfg, shape in ((e180, {}), (e6, dict(B=8, R=7)), (e64, dict(R=65))):
        for kw, why in bad:
            kw = dict(shape, **{k: (v + shape["R"] - 181 if k == "R" and shape else v) for k, v in kw.items()})
            assert L.lb_dqn_steps256(*_args(_native, cfg, keep, **kw)) < 0, kw
            msg = L.lb_last_error()
            assert msg and b"lb_dqn_steps256" in msg and why in msg, (kw, msg)
    # outside the superset (a config holds at most 256 endpoints): 32,768 envs, the thread-per-env
    # layout; trace mode
    for cfg, B, R in ((e180, 32768, 181), (_cfg(num_endpoints=256, rejection_allowed=True), 32768, 257), (_cfg(num_endpoints=64, rejection_allowed=True), 32768, 65),
                      (_cfg(), 32768, 9), (_cfg(geometry="tpe"), 8, 9)):
        assert L.lb_dqn_steps256(*_args(_native, cfg, keep, B=B, R=R)) < 0, (B, R)
        assert b"lb_dqn_steps256_supported" in L.lb_last_error(), (B, R)
        with pytest.raises(RuntimeError, match="lb_dqn_steps256_supported"):
            _native.check(L.lb_dqn_steps256(*_args(_native, cfg, keep, B=B, R=R)))
    tr = _cfg(num_endpoints=180, rejection_allowed=True, trace=True)
    assert L.lb_dqn_steps256(*_args(_native, tr, keep)) < 0
    assert b"lb_dqn_steps256" in L.lb_last_error() and b"Philox" in L.lb_last_error()
    invalid = _cfg(num_endpoints=180, rejection_allowed=True)
    invalid.episode_length = 0
    assert L.lb_dqn_steps256(*_args(_native, invalid, keep)) < 0 and L.lb_last_error()


def test_pos_and_step_words_may_coincide():
    """With sync (required here) pos_in == pos_out and vstep_in == vstep_out are accepted, as in
    lb_dqn_steps: such a call gets past those checks to the next refusal (an unsupported shape), and
    without sync it is refused for the missing sync, never for the equal words."""
    from lbk8s import _native
    L = _native.lib()
    keep = []
    big = _cfg(num_endpoints=180, rejection_allowed=True)
    same = _explore(_native, vin=FAKE + 8192, vout=FAKE + 8192)
    for steps in (1, 2, 5):
        kw = dict(B=32768, pos_in=FAKE, pos_out=FAKE, ex=C.byref(same), steps=steps)
        assert L.lb_dqn_steps256(*_args(_native, big, keep, **kw)) < 0
        assert b"lb_dqn_steps256_supported" in L.lb_last_error(), steps
        assert L.lb_dqn_steps256(*_args(_native, big, keep, sync=None, **kw)) < 0
        assert b"sync" in L.lb_last_error() and b"pos_in" not in L.lb_last_error(), steps


def test_new_flags_default_off():
    from lbk8s import cli
    from lbk8s.dqn import DQN_DeepSets
    assert inspect.signature(DQN_DeepSets).parameters["multi_step_e256"].default is False
    assert inspect.signature(cli.get_model).parameters["dqn_steps_e256"].default is False
    assert cli.build_parser().parse_args([]).dqn_steps_e256 is False
    on = cli.build_parser().parse_args(["--dqn-steps-e256"])
    assert on.dqn_steps_e256 is True and on.dqn_steps_e64 is False and on.test_fused_e256 is False
    import importlib.util
    import os
    import sys
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "rl_bench.py")
    spec = importlib.util.spec_from_file_location("rl_bench_for_dqn256", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    argv = sys.argv
    try:
        sys.argv = ["rl_bench.py"]
        off = mod.parse()
        assert off.dqn_steps_e256 is False and off.dqn_steps_e64 is False and off.endpoints is None
        sys.argv = ["rl_bench.py", "--algo", "dqn", "--dqn-steps-e256", "--endpoints", "180"]
        got = mod.parse()
        assert got.dqn_steps_e256 is True and got.dqn_steps_e64 is False and got.endpoints == 180
    finally:
        sys.argv = argv
