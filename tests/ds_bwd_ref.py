"""The reference side of the fused deep-sets training backward (k_ds_train_bwd<0/1>,
k_ds_wgrad_reduce, k_ds_set_grads, k_ds_wgrad_reduce_sets, k_ds_over_sets, k_ds_over_sets_reduce
and the three pack kernels; csrc/lbk8s_ds_train.h): tests/test_gpu_ds_backward.py runs the HIP
kernels through these runners over the C ABI, tests/test_ds_bwd_ref_harness.py a float32 numpy
stand-in of the same formulas, and broken variants of it, on the CPU.

Everything here is numpy on the CPU (torch only builds the networks and the real mode's float64
activations):
  * model(): a float64 model of the contract in include/lbk8s.h ("Fused deep-sets training") and
    the header comment of lbk8s_ds_train.h, a pure function of (weights, obs, the saved activations,
    MAX1 / MAX2 / ID1 / ID2 per set, dlogits and / or dmean).  Per set GA3 / CS2, GS2, GS1, P1 (and
    up to PER_SET_MAX sets each set's own dLambda2 / dLambda1), their sums, and lb_ds_set_grads'
    outputs formed from the per-set vectors as the header lists them.  test_ds_bwd_ref_harness.py
    shows that, summed over the sets, it equals float64 autograd through the project's modules.
  * two input modes.  real: activations, maxima and first-argmax rows of the float64 network on
    ds_ref.train_inputs (no near-tie sets).  planted: synthetic activations on the recipes' grid
    (multiples of 1/32) whose set-wise maximum is planted on a chosen row per feature, strictly
    above every other row by >= 1/32, with an optional duplicate on a later row (first wins);
    features whose h2 / c2 is negative on every row (MAX2 < 0); actor features whose h1 is 0 on
    every row (MAX1 = 0, ID1 = 0, ReLU slope 0); sets whose dlogits are all zero.  The backward is
    then fed save_* and setvec built here, laid out as the header says.
  * the case tables shared by the CPU and the GPU tests, and the runners, which hand a device
    object NaN-filled outputs with GUARD floats past their end and check what comes back.

A device object (the HIP library or the stand-in) offers, on numpy arrays:
  forward(net, heads, x)                                    -> dict(save_a, save_c, setvec)
  backward(net, heads, x, save_a, save_c, dlogits, dmean, wgrad, setvec, ws_fill, set_grads)
      -> dict(wgrad, setvec, ws_guard[, set_grads]); with set_grads given it is
      lb_ds_train_backward_sets
  set_grads(setvec, dlogits, dmean, S, R, out)              -> out
  over_sets(bufs, jobs, S, out, work)                       -> (out, work)

Tolerances.  Bit-exact: pass-through fields, zeros, fills, guards, repeated calls, the merged
launch, the pack pair.  lb_ds_set_grads / lb_ds_over_sets: sum_bound(), valid for any summation
order and for FMA or separate rounding.  The backward: the project's gradient tolerance (rtol
1e-3, atol 1e-4 max|expected|) at the granularity visible: per set for the per-set vectors (plus
1e-4 of the quantity's largest |expected| over the case only for a set whose own expected values
are all below 1e-6 of it), per tensor for the summed gradients (ds_ref.check_grads' rule).
Every checker returns the worst |error| / allowance it saw (<= 1).
"""
import collections
import copy
import functools

import numpy as np
import torch

import ds_ref

F32 = np.float32
GUARD = 64
SV = 904                      # LB_DS_SETVEC_FLOATS
WG = 4608                     # LB_DS_WGRAD_FLOATS
WS_FLOATS = 1024 * 2 * WG     # LB_DS_WORKSPACE_FLOATS
SG_ACTOR, SG_CRITIC = 4736, 12800
DSV = {"MAX0": 0, "GA3": 8, "MAX2A": 72, "GS2A": 136, "MAX1A": 200, "GS1A": 264, "CS2": 328, "MAX2C": 392,
       "GS2C": 456, "MAX1C": 520, "GS1C": 584, "ID1A": 648, "ID2A": 680, "ID1C": 712, "ID2C": 744, "P1A": 776,
       "P1C": 840}
# per head: the forward's fields and the backward's (name in the model's output, setvec field)
FWD_FIELDS = {"a": ("MAX1A", "MAX2A", "ID1A", "ID2A"), "c": ("MAX1C", "MAX2C", "ID1C", "ID2C")}
BWD_FIELDS = {"a": (("G3", "GA3"), ("GS2", "GS2A"), ("GS1", "GS1A"), ("P1", "P1A")),
              "c": (("G3", "CS2"), ("GS2", "GS2C"), ("GS1", "GS1C"), ("P1", "P1C"))}
GRID_WAVES = 256 * 8          # the backward's fixed grid: set s belongs to wave s % GRID_WAVES
BLOCK_WAVES = 8
SLOTS = 256
PER_SET_MAX = 9               # up to this many sets the model keeps each set's own dLambda
OS_SPAN = 256                 # LB_DS_OVER_SETS_SPAN
U = 2.0 ** -24


# ---- buffers ------------------------------------------------------------------------------------
def nan_buf(n):
    return np.full(n + GUARD, np.nan, F32)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same_bits(a, b, what):
    a, b = bits(a), bits(b)
    assert a.shape == b.shape, f"{what}: shape {a.shape} != {b.shape}"
    bad = a != b
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ in bits; first at {np.argwhere(bad)[0]}"


def same_values(a, b, what):
    """Equal as numbers (a maximum over rows holding both -0.0 and +0.0 has no one bit pattern)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, f"{what}: shape {a.shape} != {b.shape}"
    bad = ~(a == b)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ; first at {np.argwhere(bad)[0]}"


def body(buf, n, what):
    """The first n floats of a buffer made by nan_buf(n); its guard must be untouched."""
    assert buf.size == n + GUARD, f"{what}: buffer of {buf.size} floats, expected {n + GUARD}"
    same_bits(buf[n:], np.full(GUARD, np.nan, F32), what + " guard")
    return buf[:n]


def ids_of(setvec, name):
    """[B, 64] int: a u16 ID field of setvec [B, SV] float32."""
    o = 2 * DSV[name]
    return np.ascontiguousarray(setvec).view(np.uint16).reshape(setvec.shape[0], 2 * SV)[:, o:o + 64].astype(np.int64)


def put_ids(setvec, name, ids):
    o = 2 * DSV[name]
    setvec.view(np.uint16).reshape(setvec.shape[0], 2 * SV)[:, o:o + 64] = ids.astype(np.uint16)


def vec(setvec, name, n=64):
    return setvec[:, DSV[name]:DSV[name] + n]


# ---- weights -------------------------------------------------------------------------------------
def stack_of(net, head):
    if head == "c":
        return net.critic.psi
    return net.actor.net if hasattr(net, "actor") else net.q_network.net


def prefix_of(net, head):
    if head == "c":
        return "critic.psi"
    return "actor.net" if hasattr(net, "actor") else "q_network.net"


def head_weights(net, head, dtype=np.float64):
    """[Lambda1, Gamma1, Lambda2, Gamma2, Lambda3, Gamma3], each [out][in]."""
    st = stack_of(net, head)
    return [getattr(st[j], n).weight.detach().double().numpy().astype(dtype) for j in (0, 2, 4) for n in ("Lambda", "Gamma")]


def dact(y, relu):
    """d act / d z from the activation's output: ReLU y > 0; ELU y > 0 ? 1 : y + 1."""
    return (y > 0).astype(y.dtype) if relu else np.where(y > 0, np.ones_like(y), y + 1)


# ---- the float64 model ---------------------------------------------------------------------------
def model_head(head, w, x, h1, h2, mx0, mx1, mx2, id1, id2, d):
    """One head's backward by the documented contract, in float64.  x [B,R,8]; h1, h2 [B,R,64] (the
    actor's h1 after ReLU, everything else after ELU); mx0 [B,8]; mx1, mx2 [B,64]; id1, id2 [B,64] int; d:
    dlogits [B,R] (actor) or dmean [B,64] (critic).  Layer l is z_l = in Lambda_l^T - max_set(in)
    Gamma_l^T, and the pooled gradient goes to row ID_l of each feature."""
    f8 = np.float64
    x, h1, h2, mx0, mx1, mx2, d = (np.asarray(a, f8) for a in (x, h1, h2, mx0, mx1, mx2, d))
    _, _, L2, G2, L3, G3 = (np.asarray(a, f8) for a in w)
    B, R, _ = x.shape
    rows = np.arange(R)[None, :, None]
    out = collections.defaultdict(list)
    dL2, dL1 = np.zeros((64, 64)), np.zeros((64, 8))
    for s0 in range(0, B, 256):
        sl = slice(s0, min(B, s0 + 256))
        X, H1, H2, D = x[sl], h1[sl], h2[sl], d[sl]
        if head == "a":
            g3 = D.sum(1)                                               # sum_r dlogits
            dh2 = D[:, :, None] * L3[0][None, None, :]                  # d logit[r] / d h2[r][o]
            pooled2 = g3[:, None] * G3[0][None, :]                      # through max_set h2
            out["G3"].append(np.einsum("br,bro->bo", D, H2))            # GA3
        else:
            dh2 = np.broadcast_to(((D @ L3) / R)[:, None, :], H2.shape)  # d psi = dmean / R on every row
            pooled2 = D @ G3                                            # sum_r d psi = dmean
            out["G3"].append(H2.sum(1))                                 # CS2
        dz2 = (dh2 - (rows == id2[sl][:, None, :]) * pooled2[:, None, :]) * dact(H2, False)
        gs2 = dz2.sum(1)
        V = gs2 @ G2                                                    # through max_set h1
        p1 = V * dact(mx1[sl], head == "a")
        dz1 = (dz2 @ L2) * dact(H1, head == "a") - (rows == id1[sl][:, None, :]) * p1[:, None, :]
        out["GS2"].append(gs2)
        out["P1"].append(p1)
        out["GS1"].append(dz1.sum(1))
        if B <= PER_SET_MAX:
            out["dL2_set"].append(np.einsum("bro,bri->boi", dz2, H1))
            out["dL1_set"].append(np.einsum("bro,brc->boc", dz1, X))
        dL2 += dz2.reshape(-1, 64).T @ H1.reshape(-1, 64)
        dL1 += dz1.reshape(-1, 64).T @ X.reshape(-1, 8)
    m = {k: np.concatenate(v) for k, v in out.items()}
    m["dL2"], m["dL1"] = dL2, dL1
    # lb_ds_set_grads' outputs, from the per-set vectors as include/lbk8s.h lists them
    m["dG1"] = -m["GS1"].T @ mx0
    m["dG2"] = -m["GS2"].T @ mx1
    if head == "a":
        m["dL3"] = m["G3"].sum(0)
        m["dG3"] = -(d.sum(1)[:, None] * mx2).sum(0)
    else:
        m["dL3"] = d.T @ m["G3"] / R
        m["dG3"] = -d.T @ mx2
    return m


def set_grads_flat(m, heads):
    """The model's lb_ds_set_grads output in the header's order."""
    parts = []
    for h in ("a", "c"):
        if h in heads:
            parts += [m[h][k].reshape(-1) for k in ("dG1", "dG2", "dL3", "dG3")]
    return np.concatenate(parts)


def named_grads(net, m, heads):
    """The model's summed gradients under the modules' parameter names."""
    g = {}
    for h in heads:
        p = prefix_of(net, h)
        for j, lam, gam in ((0, "dL1", "dG1"), (2, "dL2", "dG2"), (4, "dL3", "dG3")):
            shape = tuple(getattr(stack_of(net, h)[j], "Lambda").weight.shape)
            g[f"{p}.{j}.Lambda.weight"] = m[h][lam].reshape(shape)
            g[f"{p}.{j}.Gamma.weight"] = m[h][gam].reshape(shape)
    return g


# ---- cases ---------------------------------------------------------------------------------------
# mode: planted / real; heads: "ac", "a" (dmean NULL), "c" (dlogits NULL)
Case = collections.namedtuple("Case", "mode heads R B")
PLANTED_R = (1, 2, 4, 5, 8, 9, 12, 13, 16, 17, 18, 32, 33, 49, 64, 65, 80, 81, 129, 241, 256, 257)
PLANTED_B = (1, 2, 7, 8, 9)
PLANTED_CASES = [Case("planted", h, R, B) for h in ("ac", "a", "c") for R in PLANTED_R for B in PLANTED_B]
# many sets per wave (n = ceil((B - wave) / 2,048) sets on a wave): n <= 1 at 2,047 / 2,048; 2 on one wave
# at 2,049 and on every wave at 4,096 (+1: 3 on wave 0); 6,150 = 3 x 2,048 + 6: 4 on six waves
MANY_CASES = ([Case("planted", "ac", R, B) for R in (1, 9, 17) for B in (2047, 2048, 2049, 4097, 6150)] +
              [Case("planted", "ac", R, B) for R in (65, 33) for B in (2049, 4097)])
REAL_CASES = [Case("real", "ac", R, B) for R in (1, 9, 17, 65, 81, 257) for B in (3, 300)]
AUTOGRAD_CASES = [Case("real", h, R, 5) for h in ("ac", "a", "c") for R in (1, 9, 17, 65, 257)]


def case_id(c):
    return f"{c.mode}-{c.heads}-R{c.R}-B{c.B}"


def seed_of(c):
    return 100 * c.R + c.B % 97 + {"ac": 0, "a": 1, "c": 2}[c.heads]


def net_of(c):
    """The float32 network of a case (weights in multiples of 1/32): the DQN's Q network for an
    actor-only real case, the PPO agent otherwise."""
    return ds_ref._qnet(seed_of(c)) if (c.mode == "real" and c.heads == "a") else ds_ref._agent(seed_of(c))


# ---- planted inputs -------------------------------------------------------------------------------
NEG_F = (5, 37, 62)     # h2 / c2 features negative on every row
ZERO_F = (3, 40)        # actor h1 features 0 on every row
ZERO_DL_EVERY, ZERO_DL_AT = 5, 3   # sets b % 5 == 3: dlogits all zero
MARGIN = 1              # in 1/32


def named_rows(R):
    """The rows the issue names for a planted maximum, where they exist."""
    ntl = (R + 15) // 16
    return sorted({r for r in (0, R - 1, 16 * (ntl - 1), 15, 16, 255, 256) if r < R})


def _plant(rng, B, R, relu, neg_f, zero_f, shift):
    """Integer activations (in 1/32) [B,R,64], their planted maxima [B,64] and rows [B,64]."""
    if relu:
        v = np.maximum(rng.integers(-64, 97, (B, R, 64)), 0)
    else:
        v = rng.integers(-31, 65, (B, R, 64))
    neg_f, zero_f = list(neg_f), list(zero_f)
    if neg_f:
        v[:, :, neg_f] = rng.integers(-31, -2, (B, R, len(neg_f)))
    cand = np.array(sorted(set(named_rows(R)) | {R // 3, R // 2}))
    b, o = np.arange(B)[:, None], np.arange(64)[None, :]
    pr = cand[(5 * b + o + shift) % len(cand)]   # (shift: layer 2 plants on other rows than layer 1)
    lift = rng.integers(MARGIN, MARGIN + 3, (B, 64))
    if neg_f:
        lift[:, neg_f] = MARGIN
    top = v.max(1) + lift
    np.put_along_axis(v, pr[:, None, :], top[:, None, :], axis=1)
    # a duplicate of the maximum on a later row, every fourth feature (the first must win)
    later = np.where(pr < R - 1, pr + 1 + (b + o) % np.maximum(R - 1 - pr, 1), pr)
    dup = np.where(o % 4 == 1, later, pr)
    np.put_along_axis(v, dup[:, None, :], top[:, None, :], axis=1)
    if zero_f:
        v[:, :, zero_f] = 0
        top[:, zero_f] = 0
        pr[:, zero_f] = 0
    return v, top, pr


Data = collections.namedtuple("Data", "case net x act mx0 mx id dlogits dmean")
# act[h] = (h1, h2) float32 [B,R,64]; mx[h] = (MAX1, MAX2) float32; id[h] = (ID1, ID2) int


@functools.lru_cache(maxsize=2)
def planted_data(c):
    """Both heads' planted inputs of a case (a head the case does not run still fills its forward
    fields of setvec, which the backward must leave alone)."""
    rng = np.random.default_rng(seed_of(c))
    B, R = c.B, c.R
    x = (rng.integers(-16, 17, (B, R, 8)) / 4).astype(F32)
    act, mx, ids = {}, {}, {}
    for h in ("a", "c"):
        v1, t1, p1 = _plant(rng, B, R, h == "a", (), ZERO_F if h == "a" else (), 0)
        v2, t2, p2 = _plant(rng, B, R, False, NEG_F, (), 2)
        act[h] = ((v1 / 32).astype(F32), (v2 / 32).astype(F32))
        mx[h] = ((t1 / 32).astype(F32), (t2 / 32).astype(F32))
        ids[h] = (p1, p2)
    dl = rng.standard_normal((B, R)).astype(F32)
    dl[ZERO_DL_AT::ZERO_DL_EVERY] = 0
    dm = (rng.standard_normal((B, 64)) / 8).astype(F32)
    return Data(c, net_of(c), x, act, x.max(1), mx, ids, dl, dm)


def check_planted(d):
    """The recipe's own conditions (asserted on the CPU harness)."""
    R = d.case.R
    for h in ("a", "c"):
        for layer in (0, 1):
            a, top, pr = d.act[h][layer].astype(np.float64), d.mx[h][layer].astype(np.float64), d.id[h][layer]
            assert (a * 32 == np.round(a * 32)).all(), "off the 1/32 grid"
            assert (a.max(1) == top).all() and (a.argmax(1) == pr).all(), "the planted row is not the first argmax"
            at = np.take_along_axis(a, pr[:, None, :], 1)[:, 0]
            assert (at == top).all()
            others = np.where((np.arange(R)[None, :, None] == pr[:, None, :]) | (a == top[:, None, :]), -np.inf, a)
            strict = np.ones(64, bool)
            if h == "a" and layer == 0:
                strict[list(ZERO_F)] = False
                assert (a[:, :, list(ZERO_F)] == 0).all() and (pr[:, list(ZERO_F)] == 0).all()
            if R > 1:
                gap = top - others.max(1)
                assert (gap[:, strict] >= MARGIN / 32).all(), "a runner-up within the margin"
            # rows equal to the maximum are the planted row and (at most) one later duplicate
            eq = (a == top[:, None, :])
            first = eq.argmax(1)
            assert (first == pr).all() and (eq.sum(1)[:, strict] <= 2).all()
            if layer == 1:
                assert (a[:, :, list(NEG_F)] < 0).all() and (top[:, list(NEG_F)] < 0).all()
            if not (h == "a" and layer == 0):
                assert (a > -1).all(), "below an ELU's range"
        if R > 2:
            assert (d.id[h][0] != d.id[h][1]).mean() > 0.5, "layer 2's maxima sit on layer 1's rows"
    zero = ~d.dlogits.any(1)
    assert (zero == (np.arange(d.case.B) % ZERO_DL_EVERY == ZERO_DL_AT)).all()
    return {(R, int(r)) for h in ("a", "c") for layer in (0, 1) for r in np.unique(d.id[h][layer])}


def planted_setvec(d):
    """setvec as lb_ds_train_forward leaves it (MAX0, each head's MAX1 / MAX2 / ID1 / ID2), NaN elsewhere,
    in a guarded buffer."""
    B = d.case.B
    buf = nan_buf(B * SV)
    sv = buf[:B * SV].reshape(B, SV)
    sv[:, :8] = d.mx0
    for h in ("a", "c"):
        n1, n2, i1, i2 = FWD_FIELDS[h]
        vec(sv, n1)[:] = d.mx[h][0]
        vec(sv, n2)[:] = d.mx[h][1]
        put_ids(sv, i1, d.id[h][0])
        put_ids(sv, i2, d.id[h][1])
    return buf


# ---- real inputs ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def real_data(c, exact=False):
    """The float64 network's activations, maxima and first-argmax rows on ds_ref.train_inputs, dlogits
    / dmean of ds_ref.functional (dmean through the float64 rho).  exact: dlogits / dmean stay float64
    (the autograd comparison); otherwise they are rounded to the float32 the device is given."""
    net, B, R, seed = net_of(c), c.B, c.R, seed_of(c)
    x = ds_ref.train_inputs(net, B, R, seed, False)
    wl, wv = ds_ref.functional(B, R, seed)
    n64 = copy.deepcopy(net).double()
    act, mx, ids = {}, {}, {}
    dm = None
    with torch.no_grad():
        for h in c.heads:
            st = stack_of(n64, h)
            h1 = st[1](st[0](x.double()))
            h2 = st[3](st[2](h1))
            act[h] = (h1.numpy(), h2.numpy())
            mx[h] = (act[h][0].max(1), act[h][1].max(1))
            ids[h] = (act[h][0].argmax(1), act[h][1].argmax(1))
    if "c" in c.heads:
        mean = n64.critic.psi(x.double()).mean(1).detach().requires_grad_(True)
        (n64.critic.rho(mean).squeeze(-1) * wv.double()).sum().backward()
        dm = mean.grad.numpy()
    dl = wl.double().numpy()
    if not exact:
        dl, dm = dl.astype(F32), None if dm is None else dm.astype(F32)
    xn = x.numpy()
    return Data(c, net, xn, act, xn.max(1), mx, ids, dl, dm)


def autograd_grads(c):
    """float64 autograd through the project's modules of ds_ref.functional's linear functional."""
    d = real_data(c, True)
    n64 = copy.deepcopy(d.net).double()
    x = torch.from_numpy(d.x).double()
    wl, wv = ds_ref.functional(c.B, c.R, seed_of(c))
    loss = 0
    if "a" in c.heads:
        loss = loss + (stack_of(n64, "a")(x).squeeze(-1) * wl.double()).sum()
    if "c" in c.heads:
        loss = loss + (n64.critic(x) * wv.double()).sum()
    loss.backward()
    return {n: p.grad.numpy() for n, p in n64.named_parameters() if p.grad is not None and ".rho." not in n}


@functools.lru_cache(maxsize=2)
def model_of(c, exact=False):
    d = planted_data(c) if c.mode == "planted" else real_data(c, exact)
    m = {}
    for h in c.heads:
        m[h] = model_head(h, head_weights(d.net, h), d.x, d.act[h][0], d.act[h][1], d.mx0, d.mx[h][0], d.mx[h][1],
                          d.id[h][0], d.id[h][1], d.dlogits if h == "a" else d.dmean)
    return m


# ---- the backward's checkers ----------------------------------------------------------------------
def per_set_ratio(got, exp, what):
    """rtol 1e-3, atol 1e-4 max|expected| over that set's vector; a set whose expected values are all below
    1e-6 of the quantity's largest over the case gets 1e-4 of that largest instead of nothing."""
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    assert got.shape == exp.shape, f"{what}: shape {got.shape} != {exp.shape}"
    smax = np.abs(exp).reshape(exp.shape[0], -1).max(1)
    cmax = smax.max()
    atol = 1e-4 * smax + np.where(smax < 1e-6 * cmax, 1e-4 * cmax, 0.0) + 1e-300
    allow = atol.reshape((-1,) + (1,) * (exp.ndim - 1)) + 1e-3 * np.abs(exp)
    err = np.abs(got - exp) / allow
    bad = ~(err <= 1.0)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} values outside rtol 1e-3, atol 1e-4 max|set|; first "
                           f"at {np.argwhere(bad)[0].tolist()}: got {got[bad][0]!r}, expected {exp[bad][0]!r}")
    return float(err.max())


def check_backward(c, m, sv_in, out, gs1_allow=None):
    """What a backward call returned (out: wgrad, setvec guarded buffers, ws_guard) against the model m
    and the setvec it was given."""
    what = case_id(c)
    B = c.B
    shares = {}
    same_bits(out["ws_guard"], np.full(GUARD, np.nan, F32), what + " workspace guard")
    wg = body(out["wgrad"], 2 * WG, what + " wgrad_out").reshape(2, WG)
    sv = body(out["setvec"], B * SV, what + " setvec").reshape(B, SV)
    sv0 = sv_in[:B * SV].reshape(B, SV)
    same_bits(sv[:, :8], sv0[:, :8], what + " MAX0")
    for i, h in enumerate("ac"):
        for f in FWD_FIELDS[h]:
            same_bits(vec(sv, f, 32 if f.startswith("ID") else 64), vec(sv0, f, 32 if f.startswith("ID") else 64),
                      f"{what} {f} (a forward's field)")
        if h not in c.heads:
            assert (bits(wg[i]) == 0).all(), f"{what}: wgrad_out of head {h}, not asked for, is not all +0.0"
            for _, f in BWD_FIELDS[h]:
                assert np.isnan(vec(sv, f)).all(), f"{what}: {f} of head {h}, not asked for, was written"
            continue
        shares[h + " dL2"] = ds_ref.near_train(wg[i, :4096].reshape(64, 64), m[h]["dL2"], f"{what} {h} dLambda2", 1e-3, 1e-4)
        shares[h + " dL1"] = ds_ref.near_train(wg[i, 4096:].reshape(64, 8), m[h]["dL1"], f"{what} {h} dLambda1", 1e-3, 1e-4)
        if B == 1:   # one set's own dLambda2 / dLambda1, straight from wgrad_out
            shares[h + " dL2"] = max(shares[h + " dL2"], per_set_ratio(wg[i, :4096].reshape(1, 64, 64), m[h]["dL2_set"],
                                                                       f"{what} {h} the set's dLambda2"))
            shares[h + " dL1"] = max(shares[h + " dL1"], per_set_ratio(wg[i, 4096:].reshape(1, 64, 8), m[h]["dL1_set"],
                                                                       f"{what} {h} the set's dLambda1"))
        for k, f in BWD_FIELDS[h]:
            shares[f"{h} {k}"] = per_set_ratio(vec(sv, f), m[h][k], f"{what} {f}")
    return shares


def backward_args(c, d):
    a, cr = "a" in c.heads, "c" in c.heads
    stack = lambda t: None if t is None else np.stack(t).astype(F32)
    return dict(net=d.net, heads=c.heads, x=d.x, save_a=stack(d.act["a"]) if a else None,
                save_c=stack(d.act["c"]) if cr else None, dlogits=d.dlogits if a else None, dmean=d.dmean if cr else None)


def run_backward(dev, c, ws_fill=np.nan, repeat=True):
    """A planted case: lb_ds_train_backward on setvec / save_* built here; with repeat the call is made
    twice (bit-equal).  Returns (shares, outputs)."""
    d, m = planted_data(c), model_of(c)
    sv_in = planted_setvec(d)
    args = backward_args(c, d)
    call = lambda fill: dev.backward(**args, wgrad=nan_buf(2 * WG), setvec=sv_in.copy(), ws_fill=fill, set_grads=None)
    out = call(ws_fill)
    shares = check_backward(c, m, sv_in, out)
    if repeat:
        again = call(ws_fill)
        for k in ("wgrad", "setvec"):
            same_bits(again[k], out[k], f"{case_id(c)} {k}, the same call again")
    return shares, out


def check_forward_fields(c, x, fw):
    """Exact self-consistency of the forward's setvec: each MAX is the maximum over the rows of the
    kernel's own saved activation, each ID the first row equal to it, MAX0 likewise from obs."""
    what = case_id(c)
    sv = fw["setvec"][:c.B * SV].reshape(c.B, SV)
    same_values(sv[:, :8], x.max(1), what + " MAX0")
    for h in c.heads:
        save = fw["save_a" if h == "a" else "save_c"]
        for layer, (mxn, idn) in enumerate(zip(FWD_FIELDS[h][:2], FWD_FIELDS[h][2:])):
            same_values(vec(sv, mxn), save[layer].max(1), f"{what} {mxn} against the saved activation")
            got, exp = ids_of(sv, idn), save[layer].argmax(1)
            assert (got == exp).all(), f"{what} {idn}: not the first row attaining the maximum at {np.argwhere(got != exp)[0]}"


def run_real(dev, c):
    """End to end: the training forward, the backward, lb_ds_set_grads on the device's own buffers, and
    lb_ds_train_backward_sets (bit-equal to the two calls), against the float64 network's model."""
    d, m = real_data(c), model_of(c)
    what = case_id(c)
    B, R = c.B, c.R
    fw = dev.forward(d.net, c.heads, d.x)
    sv_in = body(fw["setvec"], B * SV, what + " setvec_out")
    check_forward_fields(c, d.x, fw)
    args = dict(net=d.net, heads=c.heads, x=d.x, save_a=fw.get("save_a"), save_c=fw.get("save_c"),
                dlogits=d.dlogits if "a" in c.heads else None, dmean=d.dmean if "c" in c.heads else None)
    out = dev.backward(**args, wgrad=nan_buf(2 * WG), setvec=fw["setvec"].copy(), ws_fill=np.nan, set_grads=None)
    shares = check_backward(c, m, sv_in, out)
    if "a" not in c.heads:
        return shares
    nsg = SG_ACTOR + (SG_CRITIC if "c" in c.heads else 0)
    sv_out = out["setvec"][:B * SV].reshape(B, SV)
    sg = body(dev.set_grads(sv_out, d.dlogits, args["dmean"], B, R, nan_buf(nsg)), nsg, what + " set_grads out")
    exp = named_grads(d.net, m, c.heads)
    got = unpack_grads(d.net, c.heads, out["wgrad"][:2 * WG].reshape(2, WG), sg)
    shares["grads"] = ds_ref.check_grads(got, exp, what)
    merged = dev.backward(**args, wgrad=nan_buf(2 * WG), setvec=fw["setvec"].copy(), ws_fill=np.nan, set_grads=nan_buf(nsg))
    same_bits(merged["wgrad"], out["wgrad"], what + " wgrad_out of lb_ds_train_backward_sets")
    same_bits(merged["setvec"], out["setvec"], what + " setvec of lb_ds_train_backward_sets")
    same_bits(body(merged["set_grads"], nsg, what + " set_grads_out"), sg, what + " set_grads_out of lb_ds_train_backward_sets")
    return shares


def unpack_grads(net, heads, wg, sg):
    """wgrad_out [2][WG] and lb_ds_set_grads' out under the modules' parameter names."""
    g = {}
    off = 0
    for i, h in enumerate("ac"):
        if h not in heads:
            continue
        p, st = prefix_of(net, h), stack_of(net, h)
        n3 = 64 if h == "a" else 4096
        parts = {"0.Lambda": wg[i, 4096:], "2.Lambda": wg[i, :4096], "0.Gamma": sg[off:off + 512],
                 "2.Gamma": sg[off + 512:off + 4608], "4.Lambda": sg[off + 4608:off + 4608 + n3],
                 "4.Gamma": sg[off + 4608 + n3:off + 4608 + 2 * n3]}
        for k, v in parts.items():
            j, n = k.split(".")
            g[f"{p}.{k}.weight"] = v.reshape(tuple(getattr(st[int(j)], n).weight.shape))
        off += SG_ACTOR
    return g


# ---- lb_ds_set_grads and lb_ds_over_sets ------------------------------------------------------------
def sum_bound(A, Bm, scale, S):
    """(S + 3) 2^-24 |scale| sum_s |A(s,m) B(s,n)| + 1e-37, in float64: any summation order, FMA or not."""
    return (S + 3) * U * abs(scale) * (np.abs(A).T @ np.abs(Bm)) + 1e-37


def bound_ratio(got, exp, bound, what):
    got = np.asarray(got, np.float64).reshape(exp.shape)
    err = np.abs(got - exp) / bound
    bad = ~(err <= 1.0)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} values outside the summation bound; first at "
                           f"{np.argwhere(bad)[0].tolist()}: got {got[bad][0]!r}, expected {exp[bad][0]!r}, bound {bound[bad][0]:.3g}")
    return float(err.max())


SG_S = (1, 63, 64, 65, 128, 129, 513)
SG_R = tuple(range(1, 18)) + (257,)
SG_CASES = [(S, R, cr) for S in SG_S for R in SG_R for cr in (False, True)]


def sg_id(c):
    return f"S{c[0]}-R{c[1]}-" + ("ac" if c[2] else "a")


@functools.lru_cache(maxsize=4)
def sg_inputs(spec):
    S, R, critic = spec
    rng = np.random.default_rng(7 * S + 1000 * R + critic)
    sv = rng.standard_normal((S, SV)).astype(F32)
    dl = rng.standard_normal((S, R)).astype(F32)
    dm = rng.standard_normal((S, 64)).astype(F32) if critic else None
    return sv, dl, dm


def sg_jobs(sv, dl, dm, R):
    """(A, B, scale, extra bound) per output of lb_ds_set_grads, float64 of the float32 inputs."""
    f = lambda n, k=64: vec(sv, n, k).astype(np.float64)
    S = sv.shape[0]
    dl8 = dl.astype(np.float64)
    jobs = [(f("GS1A"), f("MAX0", 8), -1.0, None), (f("GS2A"), f("MAX1A"), -1.0, None),
            (np.ones((S, 1)), f("GA3"), 1.0, None),
            (dl8.sum(1, keepdims=True), f("MAX2A"), -1.0,
             (R + 1) * U * (np.abs(dl8).sum(1, keepdims=True).T @ np.abs(f("MAX2A"))))]
    if dm is not None:
        d8 = dm.astype(np.float64)
        jobs += [(f("GS1C"), f("MAX0", 8), -1.0, None), (f("GS2C"), f("MAX1C"), -1.0, None),
                 (d8, f("CS2"), 1.0 / R, None), (d8, f("MAX2C"), -1.0, None)]
    return jobs


def run_set_grads(dev, spec):
    S, R, critic = spec
    sv, dl, dm = sg_inputs(spec)
    n = SG_ACTOR + (SG_CRITIC if critic else 0)
    what = "set_grads " + sg_id(spec)
    raw = dev.set_grads(sv, dl, dm, S, R, nan_buf(n))
    out = body(raw, n, what)
    same_bits(dev.set_grads(sv, dl, dm, S, R, nan_buf(n)), raw, what + ", the same call again")
    worst, off = 0.0, 0
    for k, (A, Bm, scale, extra) in enumerate(sg_jobs(sv, dl, dm, R)):
        exp = scale * (A.T @ Bm)
        bound = sum_bound(A, Bm, scale, S) + (0.0 if extra is None else extra)
        worst = max(worst, bound_ratio(out[off:off + exp.size], exp, bound, f"{what} output {k}"))
        off += exp.size
    assert off == n
    return worst


OS_S = (1, 3, 4, 5, 31, 32, 33, 255, 256, 257, 513, 2049, 2305)
OS_DIMS = (1, 8, 16, 17, 20, 63, 64)
_PAIRS = [(M, N) for M in OS_DIMS for N in OS_DIMS]
# an operand: (offset in floats from a 16-byte aligned base, ld); None: a NULL (M = 1)
_FORMS = ((0, 68), (1, 68), (0, 301), (0, 904), (1, 66))
# job: (a form or None, b form, M, N, scale)
OS_LISTS = {
    "L1": [((0, 64), (0, 64), 64, 64, -1.0)],
    "L4": [(None, (0, 64), 1, 64, 0.5), (None, (1, 68), 1, 17, -1.0), ((1, 68), (1, 68), 20, 63, 0.5),
           ((0, 301), (0, 301), 64, 16, -0.375)],
    "L5": [((0, 904), (0, 904), 64, 64, -1.0), ((1, 68), (0, 64), 8, 64, 0.5), (None, (0, 4), 1, 1, -2.0),
           ((0, 301), (0, 20), 17, 17, 0.5), ((0, 64), (1, 301), 63, 20, -1.0)],
}
for _i in range(3):
    OS_LISTS[f"L16{'abc'[_i]}"] = [(_FORMS[(k + _i) % 5], _FORMS[(2 * k + _i) % 5], M, N, (-1.0, 0.5)[k % 2])
                                   for k, (M, N) in enumerate(_PAIRS[16 * _i:16 * _i + 16])]
OS_CASES = [(name, S) for name in OS_LISTS for S in OS_S]


def os_operand(buf, form, S, K):
    off, ld = form
    return np.lib.stride_tricks.as_strided(buf[off:], (S, K), (4 * ld, 4))


@functools.lru_cache(maxsize=2)
def os_inputs(spec):
    """bufs: one float32 buffer per operand, (S - 1) ld + K floats past its offset (as the header sizes
    it); jobs: (a buffer index or None, a form, b buffer index, b form, M, N, scale)."""
    name, S = spec
    rng = np.random.default_rng(S + 13 * len(name) + ord(name[-1]))
    bufs, jobs = [], []
    for fa, fb, M, N, scale in OS_LISTS[name]:
        ia = None
        if fa is not None:
            ia = len(bufs)
            bufs.append(rng.standard_normal(fa[0] + (S - 1) * fa[1] + M, dtype=F32))
        jobs.append((ia, fa, len(bufs), fb, M, N, scale))
        bufs.append(rng.standard_normal(fb[0] + (S - 1) * fb[1] + N, dtype=F32))
    return bufs, jobs


def run_over_sets(dev, spec):
    name, S = spec
    bufs, jobs = os_inputs(spec)
    what = f"over_sets {name}-S{S}"
    row = sum(j[4] * j[5] for j in jobs)
    spans = (S + OS_SPAN - 1) // OS_SPAN
    raw, work = dev.over_sets(bufs, jobs, S, nan_buf(row), nan_buf(spans * row))
    out = body(raw, row, what + " out")
    body(work, spans * row, what + " workspace")
    raw2, _ = dev.over_sets(bufs, jobs, S, nan_buf(row), nan_buf(spans * row))
    same_bits(raw2, raw, what + ", the same call again")
    worst, off = 0.0, 0
    for k, (ia, fa, ib, fb, M, N, scale) in enumerate(jobs):
        A = np.ones((S, 1)) if ia is None else os_operand(bufs[ia], fa, S, M).astype(np.float64)
        Bm = os_operand(bufs[ib], fb, S, N).astype(np.float64)
        worst = max(worst, bound_ratio(out[off:off + M * N], scale * (A.T @ Bm), sum_bound(A, Bm, scale, S),
                                       f"{what} job {k} ({M} x {N})"))
        off += M * N
    return worst


# ---- the float32 stand-in ---------------------------------------------------------------------------
# `bug` names one deliberate fault (tests/test_ds_bwd_ref_harness.py): last_argmax, gs1_no_pool,
# pool_obs_at_id2, padding_counted, no_1_over_R, dl1_drops_last_row, g3_of_previous_set, other_half_unwritten,
# stale_idle_slots, rowsum_tail, os_drop_partial_step, os_first_twice, id_u8
def _standin_head(head, w, x, h1, h2, mx1, mx2, id1, id2, d, bug, nwaves):
    """The kernel's formulas in float32: sum_r dz2 in closed form, the pooled term folded into GS1 and
    dLambda1 per set.  Returns the per-set vectors and each set's dLambda2 / dLambda1."""
    _, _, L2, G2, L3, G3 = w
    B, R, _ = x.shape
    relu = head == "a"
    if bug == "last_argmax":
        id1, id2 = R - 1 - h1[:, ::-1].argmax(1), R - 1 - h2[:, ::-1].argmax(1)
    if bug == "id_u8":
        id1, id2 = id1 & 255, id2 & 255
    wrow = d if relu else np.ones((B, R), F32)
    live = R
    if bug == "padding_counted" and R % 16:
        pad = 16 - R % 16
        rep = lambda a: np.concatenate([a, np.repeat(a[:, R - 1:R], pad, 1)], 1)
        x, h1, h2, wrow = rep(x), rep(h1), rep(h2), rep(wrow)
        live = R + pad
    rows = np.arange(live)[None, :, None]
    if relu:
        g3 = d.sum(1, dtype=F32)
        if bug == "g3_of_previous_set" and B > nwaves:
            g3 = np.concatenate([g3[:nwaves], g3[:-nwaves]])
        c1 = np.broadcast_to(L3[0][None, :], (B, 64))
        c2 = g3[:, None] * G3[0][None, :]
        wsum = g3[:, None]
    else:
        c1 = (d * (F32(1) if bug == "no_1_over_R" else F32(1) / F32(R))) @ L3
        c2 = d @ G3
        wsum = F32(R)
    mn = np.minimum(h2, F32(0))
    u = wrow[:, :, None] * c1[:, None, :] - np.where(rows == id2[:, None, :], c2[:, None, :], F32(0))
    dz2 = u * mn + u
    S = (wrow[:, :, None] * mn).sum(1, dtype=F32)
    G = (wrow[:, :, None] * h2).sum(1, dtype=F32)
    gs2 = c1 * (S + wsum) - c2 * dact(mx2, False)
    p1 = (gs2 @ G2) * dact(mx1, relu)
    dz1 = (dz2 @ L2) * dact(h1, relu)
    gs1 = dz1.sum(1, dtype=F32) - (F32(0) if bug == "gs1_no_pool" else p1)
    dL2 = np.matmul(dz2.transpose(0, 2, 1), h1)
    if bug == "dl1_drops_last_row" and R % 16 == 1:
        dz1 = dz1.copy()
        dz1[:, R - 1] = 0
    at = id2 if bug == "pool_obs_at_id2" else id1
    xid = x[np.arange(B)[:, None], at]                                   # [B,64,8]: the obs row at ID1[o]
    dL1 = np.matmul(dz1.transpose(0, 2, 1), x) - p1[:, :, None] * xid
    return dict(G3=G, GS2=gs2, GS1=gs1, P1=p1), dL2.astype(F32), dL1.astype(F32)


class StandIn:
    """The device of the CPU harness: float32 numpy, laid out over the backward's grid (set s on wave
    s % nwaves, block wave // 8, one workspace slot per block, the slots summed)."""

    def __init__(self, bug=None, nwaves=GRID_WAVES):
        self.bug, self.nwaves = bug, nwaves

    def forward(self, net, heads, x):
        B, R, _ = x.shape
        out = {"setvec": nan_buf(B * SV)}
        sv = out["setvec"][:B * SV].reshape(B, SV)
        sv[:, :8] = x.max(1)
        with torch.no_grad():
            for h in heads:
                st = stack_of(net, h)
                h1 = st[1](st[0](torch.from_numpy(x)))
                h2 = st[3](st[2](h1))
                save = np.stack([h1.numpy(), h2.numpy()])
                out["save_a" if h == "a" else "save_c"] = save
                for layer, (mxn, idn) in enumerate(zip(FWD_FIELDS[h][:2], FWD_FIELDS[h][2:])):
                    vec(sv, mxn)[:] = save[layer].max(1)
                    put_ids(sv, idn, save[layer].argmax(1))
        return out

    def backward(self, net, heads, x, save_a, save_c, dlogits, dmean, wgrad, setvec, ws_fill, set_grads):
        B, R, _ = x.shape
        sv = setvec[:B * SV].reshape(B, SV)
        work = np.full((SLOTS, 2, WG), ws_fill, F32)
        blocks = (np.arange(B) % self.nwaves) // BLOCK_WAVES
        for i, h in enumerate("ac"):
            if h not in heads:
                if self.bug != "other_half_unwritten":
                    wgrad[i * WG:(i + 1) * WG] = 0
                continue
            save, d = (save_a, dlogits) if h == "a" else (save_c, dmean)
            w = head_weights(net, h, F32)
            n1, n2, i1, i2 = FWD_FIELDS[h]
            slots = np.zeros((SLOTS, WG), F32)
            for s0 in range(0, B, 512):
                sl = slice(s0, min(B, s0 + 512))
                # (g3_of_previous_set reaches nwaves sets back: whole arrays there)
                sl = slice(0, B) if self.bug == "g3_of_previous_set" else sl
                v, dL2, dL1 = _standin_head(h, w, x[sl], save[0][sl], save[1][sl], vec(sv, n1)[sl], vec(sv, n2)[sl],
                                            ids_of(sv, i1)[sl], ids_of(sv, i2)[sl], d[sl], self.bug, self.nwaves)
                for k, f in BWD_FIELDS[h]:
                    vec(sv, f)[sl] = v[k]
                np.add.at(slots, blocks[sl], np.concatenate([dL2.reshape(-1, 4096), dL1.reshape(-1, 512)], 1))
                if sl.stop - sl.start == B:
                    break
            used = np.zeros(SLOTS, bool)
            used[blocks] = True
            keep = used if self.bug == "stale_idle_slots" else np.ones(SLOTS, bool)
            work[keep, i] = slots[keep]
            wgrad[i * WG:(i + 1) * WG] = work[:, i].sum(0, dtype=F32)
        out = dict(wgrad=wgrad, setvec=setvec, ws_guard=np.full(GUARD, np.nan, F32))
        if set_grads is not None:
            out["set_grads"] = self.set_grads(sv, dlogits, dmean, B, R, set_grads)
        return out

    def set_grads(self, setvec, dlogits, dmean, S, R, out):
        f = lambda n, k=64: vec(setvec, n, k)
        keep = np.ones(R, bool)
        if self.bug == "rowsum_tail":   # the last partial group of eight rows loses its upper half
            r = np.arange(R)
            keep = ~((r % 8 >= 4) & (r >= 8 * (R // 8)))
        rs = dlogits[:, keep].sum(1, dtype=F32, keepdims=True)
        jobs = [(f("GS1A"), f("MAX0", 8), -1.0), (f("GS2A"), f("MAX1A"), -1.0), (np.ones((S, 1), F32), f("GA3"), 1.0),
                (rs, f("MAX2A"), -1.0)]
        if dmean is not None:
            jobs += [(f("GS1C"), f("MAX0", 8), -1.0), (f("GS2C"), f("MAX1C"), -1.0),
                     (dmean, f("CS2"), F32(1) / F32(R)), (dmean, f("MAX2C"), -1.0)]
        off = 0
        for A, Bm, scale in jobs:
            r = F32(scale) * (np.ascontiguousarray(A).T @ np.ascontiguousarray(Bm))
            out[off:off + r.size] = r.reshape(-1)
            off += r.size
        return out

    def over_sets(self, bufs, jobs, S, out, work):
        row = sum(j[4] * j[5] for j in jobs)
        spans = (S + OS_SPAN - 1) // OS_SPAN
        w = work[:spans * row].reshape(spans, row)
        off = 0
        for ia, fa, ib, fb, M, N, scale in jobs:
            A = np.ones((S, 1), F32) if ia is None else np.ascontiguousarray(os_operand(bufs[ia], fa, S, M))
            Bm = np.ascontiguousarray(os_operand(bufs[ib], fb, S, N))
            for z in range(spans):
                s0, s1 = z * OS_SPAN, min(S, (z + 1) * OS_SPAN)
                if self.bug == "os_drop_partial_step":
                    s1 = s0 + 4 * ((s1 - s0) // 4)
                p = A[s0:s1].T @ Bm[s0:s1]
                if self.bug == "os_first_twice":
                    p = p + np.outer(A[s0], Bm[s0])
                w[z, off:off + M * N] = p.reshape(-1)
            out[off:off + M * N] = F32(scale) * w[:, off:off + M * N].sum(0, dtype=F32)
            off += M * N
        return out, work
