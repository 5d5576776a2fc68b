"""The host-only side of lb_ppo_steps / lb_ppo_steps_supported (ABI 17, additions): the symbols,
the supported shape (a property of (cfg, num_envs, num_elements) only) and every documented
refusal, answered before any device call (the pointers handed over here are not device memory).
No GPU; needs the built library, as tests/test_ppo_tail_ref.py.
"""
import ctypes as C
import inspect

import pytest

FAKE = 4096  # never dereferenced: a refused call makes no device call


def _cfg(**kw):
    from lbk8s import LBConfig
    trace = kw.pop("trace", False)
    return LBConfig(**kw).to_c(0, 0, True, trace, "auto")


def test_symbols_and_abi_version():
    from lbk8s import _native
    L = _native.lib()
    for f in ("lb_ppo_steps", "lb_ppo_steps_supported"):
        assert f in _native.EXPORTED_SYMBOLS and hasattr(L, f)
    assert L.lb_abi_version() == 17 == _native.ABI_VERSION
    assert "lbk8s_ppo.h" in _native.SOURCES


def test_supported_shapes():
    from lbk8s import _native
    L = _native.lib()
    sup = lambda c, B, R: L.lb_ppo_steps_supported(C.byref(c), B, R)
    e6 = _cfg(num_endpoints=6, rejection_allowed=True)
    e16 = _cfg(num_endpoints=16, rejection_allowed=False)
    assert sup(e6, 8, 7) == 1
    assert sup(e16, 67, 16) == 1
    assert sup(_cfg(), 4096, 9) == 1 and sup(_cfg(), 1, 9) == 1 and sup(_cfg(), 32767, 9) == 1
    assert sup(_cfg(num_endpoints=16, rejection_allowed=True), 67, 17) == 0   # R = 17
    assert sup(_cfg(num_endpoints=64), 16, 65) == 0                           # 64 lanes per env
    assert sup(_cfg(), 32768, 9) == 0                                         # thread-per-env layout
    assert sup(_cfg(trace=True), 8, 9) == 0                                   # trace mode
    assert sup(e6, 8, 6) == 0 and sup(e6, 8, 8) == 0                          # not the action count
    assert sup(e6, 0, 7) == 0
    bad = _cfg()
    bad.num_nodes = 10
    assert sup(bad, 8, 9) == 0


ARGS = ("frag", "obs", "state", "cfg", "B", "R", "steps", "store_rows", "uniforms", "actions_f32", "logprobs", "values",
        "rewards", "obs_next", "dones_next", "last_obs", "last_done", "actions_out", "done_out", "ep_stats_out",
        "ep_sum", "ep_cnt", "ret32", "ep_r32", "tag0", "log", "cap", "count", "stream")
REQUIRED = ("frag", "obs", "state", "uniforms", "actions_f32", "logprobs", "values", "rewards", "obs_next", "dones_next",
            "actions_out", "done_out", "ep_stats_out")


def _args(cfg, **kw):
    a = {k: FAKE + 64 * i for i, k in enumerate(ARGS)}
    a.update(cfg=C.byref(cfg), B=8, R=7, steps=5, store_rows=4, ep_r32=None, tag0=0, cap=8, stream=None)
    a.update(kw)
    return [a[k] for k in ARGS]


def test_ppo_steps_refusals():
    from lbk8s import _native
    L = _native.lib()
    e6 = _cfg(num_endpoints=6, rejection_allowed=True)
    bad = [{k: None} for k in REQUIRED]
    bad += [dict(B=0), dict(B=-3), dict(steps=0, store_rows=0), dict(steps=4097, store_rows=4097),
            dict(steps=4097, store_rows=4096), dict(steps=-1, store_rows=-1),
            dict(store_rows=3), dict(store_rows=6), dict(store_rows=-1),
            dict(last_obs=None), dict(last_done=None),                     # store_rows == steps - 1
            dict(steps=1, store_rows=0, last_obs=None), dict(steps=1, store_rows=0, last_done=None),
            dict(ep_sum=None), dict(ep_cnt=None),                          # one accumulator alone
            dict(ret32=None), dict(count=None), dict(cap=-1),              # a log without ..
            dict(R=6), dict(R=8)]                                          # not the env's action count
    for kw in bad:
        assert L.lb_ppo_steps(*_args(e6, **kw)) < 0, kw
        msg = L.lb_last_error()
        assert msg and (b"lb_ppo_steps" in msg), (kw, msg)
    # the unsupported shapes, by name
    for cfg, B, R in ((_cfg(num_endpoints=16, rejection_allowed=True), 67, 17), (_cfg(num_endpoints=64), 16, 65),
                      (_cfg(), 32768, 9), (_cfg(trace=True), 8, 9)):
        assert L.lb_ppo_steps(*_args(cfg, B=B, R=R)) < 0, (B, R)
        assert b"lb_ppo_steps_supported" in L.lb_last_error(), (B, R)
        with pytest.raises(RuntimeError, match="lb_ppo_steps_supported"):
            _native.check(L.lb_ppo_steps(*_args(cfg, B=B, R=R)))
    invalid = _cfg()
    invalid.episode_length = 0
    assert L.lb_ppo_steps(*_args(invalid, R=9)) < 0 and L.lb_last_error()


def test_learner_flag_defaults_off():
    from lbk8s.ppo import PPO_DeepSets
    p = inspect.signature(PPO_DeepSets).parameters
    assert p["fused_rollout"].default is False
    assert p["fused_act"].default is False and p["fused_bookkeeping"].default is False
    from lbk8s import cli
    args = cli.build_parser().parse_args([])
    assert args.fused_rollout is False and args.fused_act is False and args.fused_bookkeeping is False
    assert cli.build_parser().parse_args(["--fused-rollout"]).fused_rollout is True
