"""The yardsticks of the PPO tail kernels pinned on the CPU, and the host-only side of their ABI.

(a) ppo_tail_ref.gae_ref reproduces, bit for bit, the advantages / returns the reference's own
    learn() computed (tests/golden/nn_gae.npz) and ppo.compute_gae on CPU tensors at seeded random
    inputs, so the GPU tests compare lb_gae with something that is itself tied to the reference.
(b) lb_gae and lb_ppo_record are exported at ABI 17 and refuse every documented bad argument
    with a message naming the function, before any device call (the pointers handed over here
    are not device memory).  Host only; they need the built library, as tests/test_native_abi.py.
"""
import numpy as np
import pytest
import torch

import ppo_tail_ref as pr


def test_gae_ref_matches_reference_learn_bitwise():
    d = pr.gae_fixture()
    adv, ret = pr.gae_ref(d["rewards"], d["values"], d["dones"], d["next_value"], d["next_done"],
                          float(d["gamma"]), float(d["gae_lambda"]))
    assert d["rewards"].shape == (24, 4) and d["dones"].sum() == 12 and d["next_done"].sum() == 2
    assert adv.dtype == d["advantages"].dtype == np.float32
    assert np.array_equal(adv, d["advantages"])
    assert np.array_equal(ret, d["returns"])


@pytest.mark.parametrize("p_done", (0.0, 0.2, 1.0))
@pytest.mark.parametrize("T,B", ((1, 1), (2, 64), (7, 5), (128, 1031)))
def test_gae_ref_matches_compute_gae_bitwise(T, B, p_done):
    from lbk8s.ppo import compute_gae
    x = pr.gae_inputs(T, B, p_done, seed=1000 * T + B)
    gamma, lam = 0.95, 0.97
    adv, ret = pr.gae_ref(gamma=gamma, gae_lambda=lam, **x)
    t = {k: torch.from_numpy(v) for k, v in x.items()}
    tadv, tret = compute_gae(t["rewards"], t["values"], t["dones"], t["next_value"], t["next_done"], gamma, lam)
    assert np.array_equal(adv, tadv.numpy())
    assert np.array_equal(ret, tret.numpy())
    if p_done == 1.0 and T > 1:  # every step bootstraps from nothing: delta = r - v
        assert np.array_equal(adv[:-1], x["rewards"][:-1] - x["values"][:-1])


def test_ppo_record_ref_accumulates_per_env():
    rng = np.random.default_rng(3)
    B = 5
    ep_sum, ep_cnt = np.zeros(B), np.zeros(B)
    log = dict(reward=np.ones(B, np.float32), reward64=None, actions=np.arange(B, dtype=np.int32),
               ret32=np.zeros(B, np.float32), ep_r32=np.zeros(B, np.float32), tag=0, rows=[], count=0)
    want = np.zeros(B)
    for tag, done in enumerate((np.array([1, 0, 0, 1, 0], np.uint8), np.array([1, 1, 0, 0, 0], np.uint8))):
        st = rng.standard_normal((B, pr.LB_ST_K))
        log["tag"] = tag
        nd = pr.ppo_record_ref(done, st, ep_sum, ep_cnt, log)
        want += np.where(done, st[:, 0], 0.0)
        assert np.array_equal(nd, done.astype(np.float32)) and nd.dtype == np.float32
    assert np.array_equal(ep_sum, want) and np.array_equal(ep_cnt, [2, 1, 0, 1, 0])
    assert log["count"] == 4 and np.array_equal(log["ret32"], [0, 0, 2, 1, 2])
    rows = pr.sort_rows(log["rows"])
    assert np.array_equal(rows[:, pr.LB_EPLOG_ENV], [0, 3, 0, 1]) and np.array_equal(rows[:, pr.LB_EPLOG_TAG], [0, 0, 1, 1])
    assert np.array_equal(rows[:, pr.LB_EPLOG_RET32], [1, 1, 1, 2])


# ---- host-only ABI ----------------------------------------------------------------------------------
FAKE = 4096  # never dereferenced: a refused call makes no device call


def test_symbols_and_abi_version():
    from lbk8s import _native
    L = _native.lib()
    assert "lb_gae" in _native.EXPORTED_SYMBOLS and "lb_ppo_record" in _native.EXPORTED_SYMBOLS
    assert L.lb_abi_version() == 17 == _native.ABI_VERSION


def _gae_args(**kw):
    a = dict(rewards=FAKE, values=FAKE + 64, dones=FAKE + 128, next_value=FAKE + 192, next_done=FAKE + 256, T=4, B=3,
             gamma=0.95, lam=0.97, adv=FAKE + 320, ret=FAKE + 384, stream=None)
    a.update(kw)
    return list(a.values())


def test_gae_refusals():
    from lbk8s import _native
    L = _native.lib()
    bad = [dict(T=0), dict(T=-3), dict(B=0), dict(B=-1)]
    bad += [{k: None} for k in ("rewards", "values", "dones", "next_value", "next_done", "adv", "ret")]
    for ptr in _gae_args()[:5]:  # an output that is also an input
        bad += [dict(adv=ptr), dict(ret=ptr)]
    bad.append(dict(ret=FAKE + 320))  # the two outputs the same buffer
    for kw in bad:
        assert L.lb_gae(*_gae_args(**kw)) < 0, kw
        assert b"lb_gae" in L.lb_last_error(), kw
        with pytest.raises(RuntimeError, match="lb_gae"):
            _native.check(L.lb_gae(*_gae_args(**kw)))


def _rec_args(**kw):
    a = dict(B=8, done=FAKE, ep_stats=FAKE + 64, next_done=FAKE + 128, ep_sum=FAKE + 192, ep_cnt=FAKE + 256,
             reward=FAKE + 320, reward64=None, actions=FAKE + 384, ret32=FAKE + 448, ep_r32=None, tag=0, log=FAKE + 512,
             cap=8, count=FAKE + 576, stream=None)
    a.update(kw)
    return list(a.values())


def test_ppo_record_refusals():
    from lbk8s import _native
    L = _native.lib()
    bad = [dict(B=0), dict(B=-2), dict(done=None), dict(ep_stats=None), dict(next_done=None),
           dict(ep_sum=None), dict(ep_cnt=None),                      # one accumulator alone
           dict(reward=None), dict(actions=None), dict(ret32=None), dict(count=None), dict(cap=-1)]  # a log without ..
    bad += [dict(kw, log=None) for kw in (dict(B=0), dict(done=None), dict(ep_stats=None), dict(next_done=None),
                                          dict(ep_sum=None), dict(ep_cnt=None))]
    for kw in bad:
        assert L.lb_ppo_record(*_rec_args(**kw)) < 0, kw
        assert b"lb_ppo_record" in L.lb_last_error(), kw


def test_gae_device_refuses_cpu_and_misshaped_tensors():
    """gae_device raises ValueError, in the style of fused._sample_out, before the library is
    called: CPU tensors, another dtype, a non-contiguous view, a wrong shape."""
    from lbk8s.ppo import gae_device
    x = {k: torch.from_numpy(v) for k, v in pr.gae_inputs(4, 6, 0.2, seed=0).items()}
    args = lambda **kw: [dict(x, **kw)[k] for k in ("rewards", "values", "dones", "next_value", "next_done")]
    with pytest.raises(ValueError, match="gae_device"):
        gae_device(*args(), 0.95, 0.97)
    with pytest.raises(ValueError, match="gae_device"):
        gae_device(x["rewards"][0], *args()[1:], 0.95, 0.97)
