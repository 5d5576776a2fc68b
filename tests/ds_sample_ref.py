"""The reference side of the sampling forward (lb_ds_sample: k_deepsets_fwd<TS, P, 5> and
k_deepsets_fwd_big<5>, csrc/lbk8s_deepsets.h), built on tests/ds_ref.py: the case table, the
inputs, and the checker.  tests/test_gpu_ds_sample.py runs the HIP kernels through it,
tests/test_ds_sample_ref.py a float32 torch stand-in and broken ones on the CPU.

The definition under test (include/lbk8s.h), per set b over its R rows:
    l[r] = (masks is None or masks[b][r]) ? logit[b][r] : -1e8
    m = max l,  e[r] = exp(l[r] - m),  c[r] = e[0] + .. + e[r] (float32),  S = c[R-1]
    action  = the first row with e[r] > 0 and c[r] >= u[b] S (else the last row with e[r] > 0)
    logprob = l[action] - m - log(S)

Cases (the smallest shapes at which each piece of the epilogue can go wrong; batch names as
ds_ref.batch): R in {1, 2, 7, 9, 15, 16} at B4 (four sets per wave, ragged last group);
{17, 20, 31, 32} at B2 (the scan crosses a tile boundary, two sets per wave); {9, 16} at B8 (waves
loop); at B1 = 300 (one set per wave) R = 1, 16, 17, 32, 33, 65, 80 and 81, 257 (the chunked
kernel); one actor-only case (value_out NULL, a DQNDeepSetAgent image).  Masks: None and
ds_ref.argmax_masks(..., last) for each of ds_ref.LAST_SETS (set 7 nothing valid, set 9 only
row R - 1 valid).  Inputs: ds_ref.infer_inputs, then set 3 with every row equal (a uniform
distribution: boundaries at k / R) and set 4 with one row dominating.  Uniforms: a seeded
torch.rand with u[0] = 0, u[1] = 1 - 2^-24 and u[3] = 0.5 (exactly on a boundary of the uniform
set when R is even).

Tolerances.  Logits and value: ds_ref.near against the float64 network, and bit-equal to the
plain forward's.  The action: with P64 the float64 softmax of the device's own masked logits and
C64 its cumulative sum (C64[-1] := 0), every set must satisfy
    C64[a - 1] - tol <= u <= C64[a] + tol,   tol = (2 R + 8) 2^-23:
each e[r] <= 1 <= S carries at most about 3 ulp absolute error (the exp, and its rounded argument:
|x| e^-|x| <= 0.37), a prefix sum of r terms adds at most r ulp relative, the product u S one
more.  No set is exempt.  The log-probability: |logprob - (l64[a] - logsumexp64(l))| <= 2e-5 + tol
(float32 log of a sum with relative error <= tol, and the rounding of l[a] - m, |l - m| <= 88).
Every output buffer carries PAD elements past its end, NaN (actions: -7) before the launch: the
outputs must be written in full and the padding untouched.  check_sample returns the worst
|error| / allowed per quantity (<= 1).
"""
import collections
import copy
import functools

import numpy as np
import torch

import ds_ref
from ds_ref import Case, batch, case_id  # noqa: F401

FWD_SAMPLE = 5  # lb_ds_forward_kernel's `which` (LB_DS_FWD_SAMPLE)
HUGE_NEG = -1e8
PAD = 64
U_ONE = 1.0 - 2.0 ** -24

SAMPLE_CASES = ([Case("sample", "ac", R, "B4", (1, 4, 0), False) for R in (1, 2, 7, 9, 15, 16)] +
                [Case("sample", "ac", R, "B2", (2, 2, 0), False) for R in (17, 20, 31, 32)] +
                [Case("sample", "ac", R, "B8", (1, 4, 0), False) for R in (9, 16)] +
                [Case("sample", "ac", R, "B1", v, False)
                 for R, v in ((1, (1, 1, 0)), (16, (1, 1, 0)), (17, (2, 1, 0)), (32, (2, 1, 0)), (33, (3, 1, 0)),
                              (65, (5, 1, 0)), (80, (5, 1, 0)), (81, (0, 1, 0)), (257, (0, 1, 0)))] +
                [Case("sample", "a", 9, "B4", (1, 4, 0), False)])
MASK_KINDS = (None,) + ds_ref.LAST_SETS


def tol_of(R):
    return (2 * R + 8) * 2.0 ** -23


def sample_masks(c, kind):
    """(B, R) bool array of the case, or None."""
    return None if kind is None else ds_ref.argmax_masks(batch(c.bname), c.R, ds_ref.seed_of(c), kind).numpy()


def sample_uniforms(B, seed):
    u = torch.rand(B, generator=torch.Generator().manual_seed(seed + 29))
    u[0], u[1], u[3] = 0.0, U_ONE, 0.5
    return u


def _plant(net64, x, R):
    """Set 3: every row equal.  Set 4: one row (R // 2) holds more than 0.999 of the probability."""
    x[3] = x[3, :1]
    if R == 1:
        return x
    # (row r's eight inputs climb the gradient of its float64 log-probability, in unit steps)
    r, xs = R // 2, x[4:5].double()
    for _ in range(400):
        xs.requires_grad_(True)
        lp = torch.log_softmax(net64(xs)[0], -1)[r]
        x[4] = xs.detach()[0].float()
        with torch.no_grad():
            if torch.softmax(net64(x[4:5].double())[0], -1)[r] > 0.999:
                return x
        g, = torch.autograd.grad(lp, xs)
        xs = xs.detach()
        xs[0, r] += 0.5 * g[0, r] / (g[0, r].norm() + 1e-30)
    raise AssertionError("no dominating row found for set 4")


Setup = collections.namedtuple("Setup", "case B net x u ref")


@functools.lru_cache(maxsize=2)
def setup(c):
    """The case's float32 network, inputs, uniforms and float64 reference (computed once)."""
    B, R, seed = batch(c.bname), c.R, ds_ref.seed_of(c)
    net = ds_ref.infer_agent(seed) if c.heads == "ac" else ds_ref.infer_qnet(seed)
    n64 = copy.deepcopy(net).double()
    actor64 = n64.actor if c.heads == "ac" else n64.q_network
    x = _plant(actor64, ds_ref.infer_inputs(B, R, seed), R)
    ref = {}
    with torch.no_grad():
        ref["logits"] = actor64(x.double()).numpy()
        if c.heads == "ac":
            ref["value"] = n64.critic(x.double()).numpy()
    return Setup(c, B, net, x, sample_uniforms(B, seed), ref)


# ---- output buffers with canaries ---------------------------------------------------------------
NAMES = ("actions", "actions_f32", "logprob", "value", "logits")


def alloc_outputs(B, R, heads="ac", device="cpu"):
    """Flat buffers of B (logits: B R) + PAD elements, NaN (actions: -7); value None without a critic."""
    def f(n):
        return torch.full((n + PAD,), float("nan"), dtype=torch.float32, device=device)
    return {"actions": torch.full((B + PAD,), -7, dtype=torch.int32, device=device), "actions_f32": f(B),
            "logprob": f(B), "value": f(B) if heads == "ac" else None, "logits": f(B * R)}


def as_numpy(bufs):
    return {k: None if v is None else v.detach().cpu().numpy() for k, v in bufs.items()}


def unpad(got, B, R, what):
    """The outputs without their padding, which must be untouched; every output written."""
    out = {}
    for k in NAMES:
        a = got[k]
        if a is None:
            out[k] = None
            continue
        n = B * R if k == "logits" else B
        a = np.asarray(a).reshape(-1)
        assert a.shape == (n + PAD,), f"{what}: {k} buffer of {a.shape}"
        tail = a[n:]
        assert (tail == -7).all() if k == "actions" else np.isnan(tail).all(), f"{what}: {k} written past its end"
        body = a[:n]
        assert (body != -7).all() if k == "actions" else not np.isnan(body).any(), f"{what}: {k} not fully written"
        out[k] = body.reshape(B, R) if k == "logits" else body
    return out


# ---- the checker ----------------------------------------------------------------------------------
def masked64(logits, masks):
    lg = np.asarray(logits, np.float64)
    return lg if masks is None else np.where(masks, lg, HUGE_NEG)


def check_interval(logits, masks, u, actions, what):
    """The inverse-CDF interval of every set's action under the float64 softmax of `logits`
    (the device's own); returns the worst distance outside the interval / tol (<= 1)."""
    lm = masked64(logits, masks)
    B, R = lm.shape
    a = np.asarray(actions).astype(np.int64)
    assert a.shape == (B,) and ((a >= 0) & (a < R)).all(), f"{what}: action out of range"
    p = np.exp(lm - lm.max(1, keepdims=True))
    C = np.cumsum(p / p.sum(1, keepdims=True), 1)
    C = np.concatenate([np.zeros((B, 1)), C], 1)  # C[:, k] = C64[k - 1]; C64[-1] := 0
    env = np.arange(B)
    lo, hi, u = C[env, a], C[env, a + 1], np.asarray(u, np.float64)
    tol = tol_of(R)
    miss = np.maximum(np.maximum(lo - u, u - hi), 0.0) / tol
    worst = int(miss.argmax())
    assert miss[worst] <= 1.0, (f"{what}: set {worst} took row {a[worst]}, interval [{lo[worst]!r}, {hi[worst]!r}], "
                                f"u = {u[worst]!r} (tol {tol:.3g}; {int((miss > 1).sum())} of {B} sets outside)")
    return float(miss[worst])


def check_logprob(logits, masks, actions, logprob, what):
    lm = masked64(logits, masks)
    B, R = lm.shape
    a = np.asarray(actions).astype(np.int64)
    m = lm.max(1)
    exp = lm[np.arange(B), a] - (m + np.log(np.exp(lm - m[:, None]).sum(1)))
    return ds_ref.ratio(logprob, exp, 0.0, 2e-5 + tol_of(R), what + " logprob")


def check_sample(s, masks, u, got, fwd=None):
    """got: the padded output buffers as numpy arrays (alloc_outputs' layout).  fwd: the plain
    forward's {"logits", "value"} on the same inputs (bit-equal), where there is one."""
    c, B, R = s.case, s.B, s.case.R
    what = case_id(c)
    g = unpad(got, B, R, what)
    assert (g["value"] is not None) == (c.heads == "ac"), f"{what}: value output"
    out = {"logits": ds_ref.near(g["logits"], s.ref["logits"], what + " logits")}
    if c.heads == "ac":
        out["value"] = ds_ref.near(g["value"], s.ref["value"], what + " value")
    if fwd is not None:
        assert np.array_equal(g["logits"], fwd["logits"]), f"{what}: logits differ from the plain forward's"
        if c.heads == "ac":
            assert np.array_equal(g["value"], fwd["value"]), f"{what}: value differs from the plain forward's"
    a = g["actions"].astype(np.int64)
    assert ((a >= 0) & (a < R)).all(), f"{what}: action out of range"
    assert np.array_equal(g["actions_f32"], a.astype(np.float32)), f"{what}: actions_f32 != actions"
    if masks is not None:
        bad = masks.any(1) & ~masks[np.arange(B), a]
        assert not bad.any(), f"{what}: masked row taken by sets {np.flatnonzero(bad)[:8]} (u {np.asarray(u)[bad][:8]})"
    out["action"] = check_interval(g["logits"], masks, u, a, what)
    out["logprob"] = check_logprob(g["logits"], masks, a, g["logprob"], what)
    return out
