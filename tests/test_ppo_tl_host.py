"""The host-only side of lb_gae_tl, lb_ds_value_where, lb_ppo_steps_tl and lb_ppo_steps_tl_supported
(ABI 17, additions: include/lbk8s_abi_ppo_tl.h): the symbols, the prototypes against the header,
the supported shape (lb_ppo_steps') and every documented refusal, answered before any device call
(the pointers handed over here are not device memory).  No GPU; needs the built library, as
tests/test_ppo_steps_host.py, whose lists these mirror.
"""
import ctypes as C
import itertools
import os

import pytest

from test_ppo_steps_host import ARGS as PPO_ARGS, FAKE, REQUIRED as PPO_REQUIRED, _cfg

NAMES = ("lb_gae_tl", "lb_ds_value_where", "lb_ppo_steps_tl_supported", "lb_ppo_steps_tl")


def test_symbols_and_abi_version():
    from lbk8s import _native
    L = _native.lib()
    assert _native.PPO_TL_SYMBOLS == NAMES
    for f in NAMES:
        assert hasattr(L, f)
        assert getattr(L, f).restype is C.c_int and getattr(L, f).argtypes == _native.PPO_TL_PROTOTYPES[f][1]
    assert L.lb_abi_version() == 17 == _native.ABI_VERSION
    assert "../../include/lbk8s_abi_ppo_tl.h" in _native.SOURCES
    assert _native.source_hash() == L.lb_source_hash().decode()  # (csrc/Makefile's SRCS lists it too)
    others = (set(_native.EXPORTED_SYMBOLS) | set(_native.STEPS64_SYMBOLS) | set(_native.DQN64_SYMBOLS)
              | set(_native.STEPS256_SYMBOLS) | set(_native.DQN256_SYMBOLS) | set(_native.PPO256_SYMBOLS))
    assert not set(NAMES) & others


def test_prototypes_match_the_extension_header(monkeypatch):
    """The comparison of tests/test_native_abi.py, argument by argument, of
    include/lbk8s_abi_ppo_tl.h with _native.PPO_TL_PROTOTYPES; include/lbk8s.h reaches the header
    through lbk8s_abi_ppo256.h, inside its extern "C" block."""
    import test_native_abi as t
    from lbk8s import _native
    inc = os.path.dirname(t.HEADER)
    assert '#include "lbk8s_abi_ppo256.h"' in open(t.HEADER).read()
    assert '#include "lbk8s_abi_ppo_tl.h"' in open(os.path.join(inc, "lbk8s_abi_ppo256.h")).read()
    text = open(os.path.join(inc, "lbk8s_abi_ppo_tl.h")).read()
    assert "ABI 17, additions" in text
    monkeypatch.setattr(t, "HEADER", os.path.join(inc, "lbk8s_abi_ppo_tl.h"))
    header = t.header_prototypes()
    assert set(header) == set(t.declared_functions()) == set(NAMES)
    assert t.abi_mismatches(header, _native.PPO_TL_PROTOTYPES) == []
    assert header["lb_ds_value_where"][1] == ["ptr", "ptr", "ptr", "i8", "i4", "ptr", "ptr"]  # (the parser itself)
    assert header["lb_gae_tl"][1] == ["ptr"] * 6 + ["i8", "i8", "f8", "f8", "ptr", "ptr", "ptr"]
    assert header["lb_ppo_steps_tl"][1][-3:] == ["ptr"] * 3 and len(header["lb_ppo_steps_tl"][1]) == len(PPO_ARGS) + 2


def test_supported_equals_ppo_steps_supported():
    """tests/test_ppo_steps_host.py's shape table and a product around it."""
    from lbk8s import _native
    L = _native.lib()
    e6 = _cfg(num_endpoints=6, rejection_allowed=True)
    bad = _cfg()
    bad.num_nodes = 10
    table = [(e6, 8, 7), (_cfg(num_endpoints=16, rejection_allowed=False), 67, 16), (_cfg(), 4096, 9), (_cfg(), 1, 9),
             (_cfg(), 32767, 9), (_cfg(num_endpoints=16, rejection_allowed=True), 67, 17), (_cfg(num_endpoints=64), 16, 65),
             (_cfg(), 32768, 9), (_cfg(trace=True), 8, 9), (e6, 8, 6), (e6, 8, 8), (e6, 0, 7), (bad, 8, 9)]
    for E, rej, B, trace in itertools.product((6, 15, 16, 64, 65), (False, True), (1, 32767, 32768), (False, True)):
        c = _cfg(num_endpoints=E, rejection_allowed=rej, trace=trace)
        table += [(c, B, E + int(rej) + d) for d in (-1, 0, 1)]
    seen = set()
    for c, B, R in table:
        got = L.lb_ppo_steps_tl_supported(C.byref(c), B, R)
        assert got == L.lb_ppo_steps_supported(C.byref(c), B, R), (B, R)
        seen.add(got)
    assert seen == {0, 1}


GAE_ARGS = ("rewards", "values", "dones", "next_value", "next_done", "term_values", "T", "B", "gamma", "lam", "adv", "ret",
            "stream")


def _gae(**kw):
    a = {k: FAKE + 64 * i for i, k in enumerate(GAE_ARGS)}
    a.update(T=5, B=8, gamma=0.95, lam=0.97, stream=None)
    a.update(kw)
    return [a[k] for k in GAE_ARGS]


def test_gae_tl_refusals():
    from lbk8s import _native
    L = _native.lib()
    ptrs = ("rewards", "values", "dones", "next_value", "next_done", "term_values", "adv", "ret")
    bad = [{k: None} for k in ptrs] + [dict(T=0), dict(B=0), dict(T=-1), dict(B=-2)]
    a = dict(zip(GAE_ARGS, _gae()))
    bad += [{k: a[o]} for k in ptrs[:6] for o in ("adv", "ret")]  # an input that is an output, term_values among them
    bad += [dict(ret=a["adv"])]
    for kw in bad:
        assert L.lb_gae_tl(*_gae(**kw)) < 0, kw
        msg = L.lb_last_error()
        assert msg and b"lb_gae_tl" in msg, (kw, msg)
    with pytest.raises(RuntimeError, match="lb_gae_tl"):
        _native.check(L.lb_gae_tl(*_gae(term_values=None)))


def test_value_where_refusals():
    from lbk8s import _native
    L = _native.lib()
    good = dict(frag=FAKE, obs=FAKE + 64, flags=FAKE + 128, B=8, R=7, value_out=FAKE + 192, stream=None)
    bad = [{k: None} for k in ("frag", "obs", "flags", "value_out")]
    bad += [dict(B=0), dict(B=-1), dict(R=0), dict(R=-1), dict(R=_native.LB_DS_MAX_ELEMENTS_FWD + 1)]
    for kw in bad:
        a = dict(good, **kw)
        assert L.lb_ds_value_where(*(a[k] for k in ("frag", "obs", "flags", "B", "R", "value_out", "stream"))) < 0, kw
        msg = L.lb_last_error()
        assert msg and b"lb_ds_value_where" in msg, (kw, msg)


TL_ARGS = PPO_ARGS[:-1] + ("terminal_obs", "term_values", "stream")


def _tl(cfg, **kw):
    a = {k: FAKE + 64 * i for i, k in enumerate(TL_ARGS)}
    a.update(cfg=C.byref(cfg), B=8, R=7, steps=5, store_rows=4, ep_r32=None, tag0=0, cap=8, stream=None)
    a.update(kw)
    return [a[k] for k in TL_ARGS]


def test_ppo_steps_tl_refusals():
    """tests/test_ppo_steps_host.py's list under the new name, and the two new pointers."""
    from lbk8s import _native
    L = _native.lib()
    e6 = _cfg(num_endpoints=6, rejection_allowed=True)
    bad = [{k: None} for k in PPO_REQUIRED + ("terminal_obs", "term_values")]
    bad += [dict(B=0), dict(B=-3), dict(steps=0, store_rows=0), dict(steps=4097, store_rows=4097),
            dict(steps=4097, store_rows=4096), dict(steps=-1, store_rows=-1),
            dict(store_rows=3), dict(store_rows=6), dict(store_rows=-1),
            dict(last_obs=None), dict(last_done=None),
            dict(steps=1, store_rows=0, last_obs=None), dict(steps=1, store_rows=0, last_done=None),
            dict(ep_sum=None), dict(ep_cnt=None), dict(ret32=None), dict(count=None), dict(cap=-1),
            dict(R=6), dict(R=8)]
    for kw in bad:
        assert L.lb_ppo_steps_tl(*_tl(e6, **kw)) < 0, kw
        msg = L.lb_last_error()
        assert msg and b"lb_ppo_steps_tl" in msg, (kw, msg)
    for cfg, B, R in ((_cfg(num_endpoints=16, rejection_allowed=True), 67, 17), (_cfg(num_endpoints=64), 16, 65),
                      (_cfg(), 32768, 9), (_cfg(trace=True), 8, 9)):
        assert L.lb_ppo_steps_tl(*_tl(cfg, B=B, R=R)) < 0, (B, R)
        assert b"lb_ppo_steps_tl_supported" in L.lb_last_error(), (B, R)
        with pytest.raises(RuntimeError, match="lb_ppo_steps_tl_supported"):
            _native.check(L.lb_ppo_steps_tl(*_tl(cfg, B=B, R=R)))
    invalid = _cfg()
    invalid.episode_length = 0
    assert L.lb_ppo_steps_tl(*_tl(invalid, R=9)) < 0 and L.lb_last_error()


def test_gae_tl_device_refuses_cpu_and_misshaped_tensors():
    import torch
    from lbk8s.ppo import gae_tl_device
    T, B = 4, 6
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt)
    good = dict(rewards=z(T, B), values=z(T, B), dones=z(T, B), next_value=z(1, B), next_done=z(B), term_values=z(T, B),
                gamma=0.95, gae_lambda=0.97)
    with pytest.raises(ValueError, match="gae_tl_device: the tensors must be on a HIP device"):
        gae_tl_device(**good)
    with pytest.raises(ValueError, match="gae_tl_device: rewards must be a"):
        gae_tl_device(**dict(good, rewards=z(T * B)))
    with pytest.raises(ValueError, match="gae_tl_device: rewards must be a"):
        gae_tl_device(**dict(good, rewards=None))
    # the per-tensor check itself (its device is the first tensor's; on the CPU every shape, dtype
    # and layout fault is still named before the device one could be reached through `rewards`)
    from lbk8s.ppo import _gae_arg
    dev = torch.device("cpu")
    _gae_arg("term_values", z(T, B), (T, B), dev, "gae_tl_device")
    for t in (z(T, B + 1), z(B, T).t(), z(T, B, dt=torch.float64), z(T, B).numpy(), None):
        with pytest.raises(ValueError, match="gae_tl_device: term_values must be a contiguous"):
            _gae_arg("term_values", t, (T, B), dev, "gae_tl_device")
