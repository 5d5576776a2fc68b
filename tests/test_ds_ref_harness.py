"""The deep-sets forward family's reference harness (tests/ds_ref.py) checked on the CPU, no GPU.

The device under test here is a stand-in: torch's float32 forward / backward of the same
networks on the CPU, written out layer by layer so that single steps can be broken
(tests/test_gpu_ds_variants.py runs the same cases and checkers on the HIP kernels).

(a) The float64 reference accepts a correct float32 implementation on every case of the table:
    the tolerances and the argmax disagreement cap leave the reference itself a wide margin.
(b) The checkers catch what they claim to: each deliberately broken stand-in fails.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ds_ref
from ds_ref import ARGMAX_CASES, INFER_CASES, PAIR_CASES, TRAIN_CASES, case_id

ALL_CASES = INFER_CASES + TRAIN_CASES + ARGMAX_CASES + PAIR_CASES


# ---- the float32 stand-in -----------------------------------------------------------------------
def pool(x, bug):
    """The set-wise max (B, 1, C) of x (B, R, C), as EquivariantLayer takes it, or broken."""
    B, R, _ = x.shape
    if bug == "last_tie":  # the LAST row attaining the max gets the pooled gradient
        return torch.max(x.flip(1), dim=1, keepdim=True)[0]
    p = torch.max(x, dim=1, keepdim=True)[0]
    if bug == "swap_sets":  # set b reads the max of set b XOR 1
        return p[torch.arange(B).bitwise_xor(1).clamp(max=B - 1)]
    if bug == "zero_pad" and R % 16:  # rows R .. 16 TS - 1, zeros, take part in the max
        return p.clamp(min=0)
    return p


def stack(x, w, acts, bug):
    """Eq act Eq act Eq with w = [Lambda1, Gamma1, Lambda2, Gamma2, Lambda3, Gamma3]."""
    for i, act in enumerate(acts + (None,)):
        x = F.linear(x, w[2 * i]) - F.linear(pool(x, bug), w[2 * i + 1])
        if act is not None:
            x = act(x)
    return x


def params_of(net):
    return {n: p.detach().clone().requires_grad_() for n, p in net.named_parameters()}


def eq_weights(p, prefix):
    return [p[f"{prefix}.{j}.{m}.weight"] for j in (0, 2, 4) for m in ("Lambda", "Gamma")]


def actor(p, prefix, x, bug=None):
    return stack(x, eq_weights(p, prefix), (F.relu, F.elu), bug).squeeze(-1)


def critic(p, x, bug=None):
    psi = stack(x, eq_weights(p, "critic.psi"), (F.elu, F.elu), bug)
    R = x.shape[1]
    mean = psi.sum(1) / (16 * ((R + 15) // 16) if bug == "mean_tiles" else R)  # (the mean over 16 TS rows)
    h = F.elu(F.linear(mean, p["critic.rho.0.weight"], p["critic.rho.0.bias"]))
    return F.linear(h, p["critic.rho.2.weight"], p["critic.rho.2.bias"]).squeeze(-1)


def unwritten_tail(c, B, t, bug):
    """(c): the outputs stored from lanes col < P, left unwritten for the ragged last group."""
    t = t.detach().clone()
    if bug == "unwritten_tail" and B % c.variant[1]:
        t[B - B % c.variant[1]:] = float("nan")
    return t


def greedy(s, q, masks, bug):
    qm = q if masks is None or bug == "ignore_mask" else np.where(masks, q, np.float32(ds_ref.dqn_ref.HUGE_NEG))
    a = qm.argmax(1)
    if bug == "last_tie":  # the last index, not the first, of identical rows
        same = ds_ref.dqn_ref.same_rows(s.x.numpy(), a) & (True if masks is None else masks)
        last = s.case.R - 1 - same[:, ::-1].argmax(1)
        a = np.where(same.any(1), last, a)
    return a.astype(np.int32)


def run_case(c, bug=None):
    """The stand-in's outputs of case c through the case's checker; returns the margins."""
    s = ds_ref.setup(c)
    p = params_of(s.net)
    prefix = "actor.net" if c.heads == "ac" else "q_network.net"
    if c.family in ("infer", "train"):
        logits = actor(p, prefix, s.x, bug)
        got = {"logits": logits.detach().numpy()}
        loss = 0
        if c.family == "train":
            wl, wv = s.extra
            loss = (logits * wl).sum()
        if c.heads == "ac":
            value = critic(p, s.x, bug)
            got["value"] = unwritten_tail(c, s.B, value, bug).numpy()
            if c.family == "train":
                loss = loss + (value * wv).sum()
        if c.family == "infer":
            return ds_ref.check_infer(s, got)
        loss.backward()
        got["grads"] = {n: t.grad.numpy() for n, t in p.items()}
        return ds_ref.check_train(s, got)
    if c.family == "argmax":
        with torch.no_grad():
            q = actor(p, prefix, s.x, bug).numpy()
        # a kernel computes every row by the same instructions, so equal rows get equal Q values; a
        # CPU GEMM computes its row panels in different orders, and the stand-in restores the
        # property: a row takes the Q value of the first row of its set with the same bits
        bits = s.x.numpy().view(np.uint32)
        first = (bits[:, :, None, :] == bits[:, None, :, :]).all(-1).argmax(-1)
        q = np.take_along_axis(q, first, 1)
        out = {}
        for last in ds_ref.LAST_SETS + (None,):
            masks = None if last is None else ds_ref.argmax_masks(s.B, c.R, ds_ref.seed_of(c), last).numpy()
            a = greedy(s, q, masks, bug)
            out[last] = ds_ref.check_actions(s, masks, a, q, f"{case_id(c)} last={last}")
            if last is not None:
                assert a[5] == 0 and a[7] == 0 and a[9] == c.R - 1
                assert a[s.B - 1] == (c.R - 1 if last == "only_last" else 0)
        return out
    target, xn, a, r, d = s.extra
    with torch.no_grad():
        q_next = actor(params_of(target), prefix, xn, bug)
    q = actor(p, prefix, s.x, bug)
    td = r + ds_ref.GAMMA * q_next.max(1, keepdim=True).values * (1 - d)
    F.mse_loss(td, q.gather(1, a)).backward()
    return ds_ref.check_pair(s, {"q": q.detach().numpy(), "q_next": q_next.numpy(),
                                 "grads": {n: t.grad.numpy() for n, t in p.items()}})


# ---- (a) ------------------------------------------------------------------------------------------
def test_stand_in_is_the_modules_forward():
    """The layer-by-layer stand-in computes what the project's modules compute, bit for bit."""
    s = ds_ref.setup(INFER_CASES[3])
    p = params_of(s.net)
    with torch.no_grad():
        assert torch.equal(actor(p, "actor.net", s.x), s.net.actor(s.x))
        assert torch.equal(critic(p, s.x), s.net.critic(s.x))


def test_case_table_names_every_variant():
    """Every multi-set variant of the family is in the table, with ragged last groups."""
    assert len({case_id(c) for c in ALL_CASES}) == len(ALL_CASES)
    seen = {(c.family, c.heads, c.variant) for c in ALL_CASES}
    for fam, heads in (("infer", "ac"), ("infer", "a"), ("train", "ac"), ("train", "a")):
        assert {(fam, heads, v) for v in ((1, 4, 0), (1, 2, 0), (2, 2, 0))} <= seen
    assert {("argmax", "a", (1, 2, 0)), ("argmax", "a", (2, 2, 0))} <= seen
    assert {("pair", "a", (1, p, 0)) for p in (1, 2, 4)} <= seen
    assert ds_ref.batch("B4") % 4 == 3 and ds_ref.batch("B2") % 2 == 1 and ds_ref.batch("B8") % 4 == 1
    cus = ds_ref.device_cus()
    assert -(-ds_ref.batch("B8") // 4) > 8 * cus  # more groups of four than waves in the grid


@pytest.mark.parametrize("c", ALL_CASES, ids=case_id)
def test_reference_accepts_float32_stand_in(c):
    m = run_case(c)
    print(case_id(c), m)


# ---- (b) ------------------------------------------------------------------------------------------
def find(family, heads, R, bname, ties=False):
    (c,) = [c for c in ALL_CASES if (c.family, c.heads, c.R, c.bname, c.ties) == (family, heads, R, bname, ties)]
    return c


# mutation: the cases it must fail, with the checker's message
BUGS = {
    # (a) the pooled max of set b taken from set b XOR 1
    "swap_sets": [(find("infer", "ac", 7, "B4"), "logits"), (find("train", "a", 7, "B2", True), "logits"),
                  (find("pair", "a", 7, "B2"), " q")],
    # (b) the max over the R rows padded with zeros up to 16
    "zero_pad": [(find("infer", "ac", 3, "B4"), "logits"), (find("infer", "a", 17, "B2"), "logits"),
                 (find("train", "ac", 7, "B2"), "logits|value"), (find("argmax", "a", 7, "B2"), "q_out|below")],
    # (c) the value of the last B mod P sets left unwritten
    "unwritten_tail": [(find("infer", "ac", 7, "B4"), "value"), (find("infer", "ac", 16, "B2"), "value"),
                       (find("train", "ac", 15, "B4", True), "value")],
    # (d) the last instead of the first row on ties: the action, the pooled gradient's routing
    "last_tie": [(find("argmax", "a", 7, "B2"), "identical rows"), (find("argmax", "a", 32, "B2"), "identical rows"),
                 (find("train", "ac", 7, "B2", True), "grad"), (find("train", "a", 24, "B2"), "grad")],
    # (e) the psi mean over 16 TS rows instead of R
    "mean_tiles": [(find("infer", "ac", 7, "B4"), "value"), (find("train", "ac", 17, "B2"), "value")],
    # (f) the mask ignored
    "ignore_mask": [(find("argmax", "a", 9, "B2"), "masked action"), (find("argmax", "a", 257, "B1"), "masked action")],
}


@pytest.mark.parametrize("bug", list(BUGS))
def test_checker_catches_broken_stand_in(bug):
    for c, match in BUGS[bug]:
        with pytest.raises(AssertionError, match=match):
            run_case(c, bug)
