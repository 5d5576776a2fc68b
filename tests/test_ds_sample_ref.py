"""The sampling forward's reference harness (tests/ds_sample_ref.py) checked on the CPU, and the
host-only side of lb_ds_sample's ABI.

(a) A float32 torch stand-in of the definition passes check_sample on every case and mask kind.
(b) Five broken stand-ins each fail it.
(c) lb_ds_forward_kernel(LB_DS_FWD_SAMPLE, ..) answers as LB_DS_FWD over the table and refuses
    R = 0 and R = 258; lb_ds_sample refuses each required pointer NULL before any device call.
    (Host only; they need the built library, as tests/test_native_abi.py.)
"""
import functools

import numpy as np
import pytest
import torch

import ds_ref
import ds_sample_ref as sr
from ds_sample_ref import MASK_KINDS, SAMPLE_CASES, case_id

BUGS = ("action_plus_one", "unrepaired_u0", "logprob_row0", "exclusive_scan", "tile_scan")


@functools.lru_cache(maxsize=2)
def forward32(c):
    """The float32 torch forward of the case: logits (B, R), value (B,) or None."""
    s = sr.setup(c)
    with torch.no_grad():
        if c.heads == "ac":
            return s.net.actor(s.x).numpy(), s.net.critic(s.x).numpy()
        return s.net.q_network(s.x).numpy(), None


def draw32(logits, masks, u, bug=None):
    """The header's draw in float32 numpy (or broken): (actions (B,) int64, logprob (B,) float32)
    of float32 logits (B, R), masks (B, R) bool or None and uniforms (B,) float32."""
    B, R = logits.shape
    l = logits if masks is None else np.where(masks, logits, np.float32(sr.HUGE_NEG))
    m = l.max(1, keepdims=True)
    e = np.exp(l - m)
    if bug == "tile_scan":  # the prefix restarts at every 16-row tile
        c_ = np.concatenate([np.cumsum(e[:, t:t + 16], 1, dtype=np.float32) for t in range(0, R, 16)], 1)
    else:
        c_ = np.cumsum(e, 1, dtype=np.float32)
    S = np.cumsum(e, 1, dtype=np.float32)[:, -1:]
    if bug == "exclusive_scan":
        c_ = c_ - e
    thr = u[:, None] * S
    if bug == "unrepaired_u0":  # DeepSetAgent.act's count of c < u S
        a = np.minimum((c_ < thr).sum(1), R - 1)
    else:
        hit = (e > 0) & (c_ >= thr)
        last = R - 1 - (e > 0)[:, ::-1].argmax(1)
        a = np.where(hit.any(1), hit.argmax(1), last)
    if bug == "action_plus_one":
        a = (a + 1) % R
    row = np.zeros(B, np.int64) if bug == "logprob_row0" else a
    logprob = l[np.arange(B), row] - m[:, 0] - np.log(S[:, 0])
    return a, logprob


def stand_in(c, kind, bug=None):
    """The definition in float32 numpy (or broken), into NaN-filled padded buffers."""
    s = sr.setup(c)
    B, R = s.B, c.R
    logits, value = forward32(c)
    masks = sr.sample_masks(c, kind)
    u = s.u.numpy()
    a, logprob = draw32(logits, masks, u, bug)
    got = sr.as_numpy(sr.alloc_outputs(B, R, c.heads))
    got["actions"][:B] = a
    got["actions_f32"][:B] = a
    got["logprob"][:B] = logprob
    got["logits"][:B * R] = logits.reshape(-1)
    if value is not None:
        got["value"][:B] = value
    return sr.check_sample(s, masks, u, got, fwd={"logits": logits, "value": value})


@pytest.mark.parametrize("c", SAMPLE_CASES, ids=case_id)
def test_stand_in_passes(c):
    out = {kind: stand_in(c, kind) for kind in MASK_KINDS}
    print("ds-sample-margin", case_id(c), out)
    for kind, m in out.items():
        assert max(m.values()) <= 1.0, (kind, m)


def _case(R, bname):
    return next(c for c in SAMPLE_CASES if c.R == R and c.bname == bname and c.heads == "ac")


@pytest.mark.parametrize("bug", BUGS)
def test_broken_stand_ins_fail(bug):
    if bug == "unrepaired_u0":
        # the formula is wrong where the u = 0 set (set 0) has row 0 masked and another row valid
        picks = [(c, k) for c in SAMPLE_CASES for k in ds_ref.LAST_SETS
                 if c.R > 1 and not sr.sample_masks(c, k)[0, 0] and sr.sample_masks(c, k)[0].any()]
        assert picks, "no case masks row 0 of the u = 0 set"
        picks = picks[:3]
    elif bug == "tile_scan":
        picks = [(_case(20, "B2"), None), (_case(65, "B1"), "equal"), (_case(257, "B1"), None)]
    else:
        picks = [(_case(9, "B4"), None), (_case(20, "B2"), "none"), (_case(65, "B1"), "only_last")]
    for c, kind in picks:
        with pytest.raises(AssertionError):
            stand_in(c, kind, bug)
        stand_in(c, kind)  # (the same case passes unbroken)


def test_canaries_are_checked():
    c = _case(9, "B4")
    s = sr.setup(c)
    logits, value = forward32(c)
    # (written past the end three times, then left unwritten twice)
    for name, where, v in (("logprob", s.B, 1.0), ("actions", s.B, 1), ("logits", s.B * c.R, 1.0),
                           ("logprob", s.B - 1, np.nan), ("actions", 0, -7)):
        got = sr.as_numpy(sr.alloc_outputs(s.B, c.R))
        got["actions"][:s.B] = 0
        for k in ("actions_f32", "logprob", "value"):
            got[k][:s.B] = 0.0
        got["logits"][:s.B * c.R] = logits.reshape(-1)
        sr.unpad(got, s.B, c.R, "clean")
        got[name][where] = v
        with pytest.raises(AssertionError):
            sr.unpad(got, s.B, c.R, name)


# ---- host-only ABI ----------------------------------------------------------------------------------
def test_sample_kernel_is_the_plain_forwards():
    from lbk8s import fused
    assert fused.FWD_SAMPLE == sr.FWD_SAMPLE == 5
    for c in SAMPLE_CASES:
        B = sr.batch(c.bname)
        assert fused.forward_kernel(fused.FWD_SAMPLE, B, c.R) == fused.forward_kernel(fused.FWD, B, c.R), case_id(c)
    for B in (1, 128, 300, 4096, 4099, 100000):
        for R in (1, 9, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 257):
            assert fused.forward_kernel(fused.FWD_SAMPLE, B, R) == fused.forward_kernel(fused.FWD, B, R), (B, R)
    for which, R in ((fused.FWD_SAMPLE, 0), (fused.FWD_SAMPLE, 258), (4, 9), (6, 9)):  # (4 names no forward)
        with pytest.raises(RuntimeError, match="lb_ds_forward_kernel"):
            fused.forward_kernel(which, 300, R)


def test_sample_refuses_null_pointers():
    """Each required pointer NULL in turn (and num_envs < 1, R out of range): < 0 with a message
    before anything is launched -- the other pointers here are not device memory."""
    from lbk8s import _native
    L = _native.lib()
    assert "lb_ds_sample" in _native.EXPORTED_SYMBOLS and _native.ABI_VERSION >= 16
    fake = 4096
    #       frag  obs   B    R  masks unif  logits act   actf  logp  value stream
    good = [fake, fake, 64, 9, None, fake, None, fake, None, fake, None, None]
    for i, name in ((0, "frag"), (1, "obs"), (5, "uniforms"), (7, "actions_out"), (9, "logprob_out")):
        args = list(good)
        args[i] = None
        assert L.lb_ds_sample(*args) < 0, name
        assert b"lb_ds_sample" in L.lb_last_error(), name
    for B, R in ((0, 9), (-1, 9), (64, 0), (64, 258)):
        args = list(good)
        args[2], args[3] = B, R
        assert L.lb_ds_sample(*args) < 0, (B, R)
        assert L.lb_last_error()
