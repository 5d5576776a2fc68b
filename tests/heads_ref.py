"""References, recipes and checkers for the small kernels between the forwards and the
optimiser in both learners: lb_ppo_head (k_ppo_head), lb_dqn_head (k_dqn_head_block /
k_dqn_head), lb_episode_log (k_episode_log) and lb_replay_sample (k_replay_sample).

Everything here is numpy and torch float64 on the CPU.  The device under test is an object with
    ppo_head(c, bufs)                  -> bufs      (dlogits, dvalue, terms)
    dqn_head(c, bufs, block)           -> bufs      (dq, sq_err, td | None, old | None, loss | None)
    episode_log(B, done, ep_stats, reward, reward64 | None, actions, ret32, ep_r32 | None, tag,
                log, cap, count)       -> (ret32, ep_r32 | None, log, count)
    replay_sample(c, ring, bufs)       -> bufs      (obs, next_obs, actions, rewards, dones)
taking and returning numpy arrays (tests/test_gpu_heads.py: the HIP kernels through the C ABI;
tests/test_heads_ref_harness.py: float32 CPU stand-ins and deliberately broken ones).  Every
output buffer is made here, filled with NaN (integers: SENTINEL_I64) and GUARD elements longer
than the kernel may write; a checker requires every element the header names to be overwritten
and everything else, the guard included, to still hold the fill.

PPO head.  Reference: float64 autograd through envs/ppo_deepset.py:227-263's ops (masked
Categorical, clipped ratio, clipped value loss, entropy bonus); the per-set terms [M,6] and
d mean-loss / d logits, d mean-loss / d value.  clip / ent_coef / vf_coef enter the reference as
the float32 values the kernel receives.
  Smooth cases redraw every set that lies, in float64, within 1e-4 of a kink of the loss
  (|ratio - (1 +- clip)|, ||v - vold| - clip|, or |v - vold| > clip with |vu - vcl| < 1e-4 (1 + vu)),
  so float32 and float64 take the same branch and the clipped indicator is decidable;
  check_ppo asserts that no such set is left.
  Tie cases put sets exactly ON a kink, built from values float32 and float64 agree on:
    one valid row (or R = 1): log_prob = 0 exactly; with oldlogp = 0 the ratio is exactly 1 and
      pg1 == pg2 (with clip = 0 the ratio sits on both closed clamp bounds).  On such a set
      d log_prob / d logits = 0, so these pin the terms (pg = -A, kl = 0, clipped = 0) and a zero
      gradient whatever the tie rule;
    vold = 1, v = 1.25 (and 0.75), clip = 0.25: |v - vold| on the closed bound, gradient 2 (v - ret);
    ret = 1, vold = 0.5, v = 1.25 (and vold = 1.5, v = 0.75): outside the clip with vu == vcl =
      0.0625, d vt / d v = +-0.25 (torch.max's even split) -- the tie rules show in dvalue here;
    v == vold, the first epoch's common case.
  Tolerances: the means, dlogits and dvalue as tests/test_gpu_fused_train.py::
  test_ppo_head_matches_autograd (close(1e-5, 1e-6), 1e-4 for approx_kl; _check(1e-4, 1e-5) and
  _check(1e-4, 1e-6)); per-set columns 0-3 rtol 1e-5 (column 3: 1e-4) atol 1e-6; column 4 equal;
  column 5, a cancelling sum of three parts, 1e-6 + 1e-5 (|pg| + ent_coef |H| + vf_coef / 2 |vt|).
  Out of scope: a set with no valid row (-1e8 + log R has no float32; torch's own float32 loses
  it the same way) -- required there: finite outputs, dlogits == 0 on every row, six terms
  written; it is left out of the means.  A taken action that is masked (but for that set).

DQN head.  Reference: float64 F.mse_loss(r + gamma max q_next (1 - d), q.gather(1, a)) and its
autograd gradient.  td rtol / atol 1e-6; old bit-equal q[a]; dq exactly 0 off column a, rtol
1e-5 atol 1e-7 on it; loss rtol 1e-5 atol 1e-6 (tests/test_gpu_learners.py::
test_dqn_head_matches_autograd).  sq_err, for which that test sets nothing: rtol 1e-5 atol 1e-6
(d = td - old carries a few float32 roundings of O(1) values, ~2e-7 absolute, so d^2 is off by
~4e-7 |d|: relative 4e-7 / |d| for |d| > 0.1 and under the floor below).  loss_out against
float32(float64 sum of the device's own sq_err / M): one float32 ulp (1.2e-7), for the order of
the float64 sum.  For M <= 1024 both kernels run on the same inputs and must agree bit for bit.

Episode log.  Reference exact, numpy (run_eplog): ret32' = float32(float64(ret32) + r64), or
ret32 + float32 reward without reward64; a finished env appends its row and restarts at 0;
ep_r32 moves only for finished envs; *count rises by the number finished whatever cap.  Rows
compared on columns 0..20 keyed by (tag, env) -- each a finished env, none twice within a tag,
exactly min(cap, finished) of them, earlier tags first; columns 21..23 are unspecified.  Every
env's first (ret32, r64) pair is one where rounding once and twice differ.

Measured, worst error as a share of its allowance over all cases: the float32 stand-ins of
tests/test_heads_ref_harness.py 0.23 (PPO: a per-set value term) and 0.114 (DQN: td); the HIP
kernels on an MI355X 0.54 (PPO: a per-set entropy; dlogits <= 0.020, dvalue <= 0.001) and 0.114
(DQN: td), the two DQN kernels equal bit for bit at every M <= 1024, the episode log and the
replay sample equal throughout.  No case needed more than its allowance, so no tolerance here
comes from a measurement (per-case figures: DESIGN.md section 2).

Replay sample.  A ring whose every field encodes (slot, env) (and the float's index inside the
observation); the draws are oracle.replay_sample's.  An unclamped upper = 0 alone changes no
draw (w * 0 >> 32 is slot 0 either way); what the clamp protects is anything that bounds a
draw by `upper`, so the broken stand-in of that name guards its gather with slot < upper and
leaves the outputs unwritten.
"""
import types
import zlib

import numpy as np
import torch

GUARD = 64                      # elements (log: rows) past each output's end
SENTINEL_I64 = -0x5A5A5A5A5A5A5A5B
F32 = np.float32
BOUNDARY_ROWS = (63, 64, 127, 128, 191, 192, 255, 256)
MARGIN = 1e-4


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def nan_buf(n, dtype=np.float32):
    return np.full(n + GUARD, np.nan, dtype)


def _written(buf, n, what):
    """buf[:n] fully overwritten (no NaN), buf[n:] untouched; returns buf[:n]."""
    buf = np.asarray(buf)
    assert buf.shape[0] >= n + GUARD, f"{what}: buffer shorter than handed out"
    head, tail = buf[:n], buf[n:]
    bad = np.flatnonzero(np.isnan(head).reshape(n, -1).any(1)) if n else []
    assert len(bad) == 0, f"{what}: {len(bad)} elements left unwritten, first at {bad[:4]}"
    assert np.isnan(tail).all(), f"{what}: written past its end"
    return head


def _share(got, exp, rtol, atol):
    """(worst |got - exp| / (atol + rtol |exp|), its flat index)."""
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    if got.size == 0:
        return 0.0, 0
    s = np.abs(got - exp) / (atol + rtol * np.abs(exp))
    s = np.where(np.isfinite(got), s, np.inf)
    i = int(s.argmax())
    return float(s.flat[i]), i


# ================================ PPO head ====================================================

def _masked_logp64(c):
    L = torch.from_numpy(c.logits).double()
    if c.masks is not None:
        L = torch.where(torch.from_numpy(c.masks.astype(bool)), L, torch.full((), -1e8, dtype=torch.float64))
    return torch.log_softmax(L, 1).numpy()


def ppo_margins(c):
    """(M,) bool: the set lies within MARGIN of a kink of the loss, in float64."""
    clip = float(F32(c.clip))
    a = c.actions.astype(np.int64)
    nlp = _masked_logp64(c)[np.arange(c.M), a]
    ratio = np.exp(nlp - c.oldlogp.astype(np.float64))
    v, vo, rt = (x.astype(np.float64) for x in (c.value, c.vold, c.ret))
    d = v - vo
    vu = (v - rt) ** 2
    vcl = (vo + np.clip(d, -clip, clip) - rt) ** 2
    b1 = (np.abs(ratio - (1 - clip)) < MARGIN) | (np.abs(ratio - (1 + clip)) < MARGIN)
    b2 = np.abs(np.abs(d) - clip) < MARGIN
    b3 = (np.abs(d) > clip) & (np.abs(vu - vcl) < MARGIN * (1 + vu))
    return b1 | b2 | b3


def ppo_case(name, M, R, masked, clip_vloss=1, ent_coef=0.01, clip=0.2, vf_coef=0.5, rotate_last=False):
    """The inputs of tests/test_gpu_fused_train.py::test_ppo_head_matches_autograd (logits ~ 3 N,
    ~20 % masked with the taken action valid, |v - vold| and the ratio on both sides of the
    clip), plus: the actions cover rows 0, R - 1 and every existing row next to a 64-row register
    slot; in masked cases of M >= 5 set 1 has no valid row (out of scope) and sets 2 and M - 2
    exactly one; rotate_last: the last set is set 0 rotated by one row."""
    rng = _rng(name)
    c = types.SimpleNamespace(name=name, M=M, R=R, clip_vloss=int(clip_vloss), ent_coef=ent_coef, clip=clip,
                              vf_coef=vf_coef, ties=False)
    c.logits = (rng.standard_normal((M, R)) * 3).astype(F32)
    masks = (rng.random((M, R)) > 0.2) if masked else None
    actions = rng.integers(0, R, M)
    forced = sorted({0, R - 1} | {b for b in BOUNDARY_ROWS if b < R})
    first = 3 if M >= 5 + len(forced) else 0
    for k, row in enumerate(forced):
        if first + k < M:
            actions[first + k] = row
    c.forced = forced[:max(0, M - first)]
    if rotate_last:
        c.logits[M - 1] = np.roll(c.logits[0], 1)
        actions[M - 1] = (actions[0] + 1) % R
        if masked:
            masks[M - 1] = np.roll(masks[0], 1)
    c.in_scope = np.ones(M, bool)
    c.one_valid = []
    if masked:
        masks[np.arange(M), actions] = True
        if M >= 5:
            c.one_valid = [2, M - 2]
            for s in c.one_valid:
                masks[s] = False
                masks[s, actions[s]] = True
            masks[1] = False
            c.in_scope[1] = False
        c.masks = masks.astype(np.uint8)
    else:
        c.masks = None
    c.actions = actions.astype(F32)
    lpa = _masked_logp64(c)[np.arange(M), actions].astype(F32)
    for f in ("value", "ret", "vold", "adv", "oldlogp"):
        setattr(c, f, np.zeros(M, F32))
    todo = np.arange(M)
    for _ in range(64):
        n = len(todo)
        c.value[todo] = (rng.standard_normal(n) * 5).astype(F32)
        c.ret[todo] = c.value[todo] + (rng.standard_normal(n) * 2).astype(F32)
        c.vold[todo] = c.value[todo] + (rng.standard_normal(n) * 0.3).astype(F32)
        c.adv[todo] = rng.standard_normal(n).astype(F32)
        c.oldlogp[todo] = lpa[todo] + (rng.standard_normal(n) * 0.3).astype(F32)
        todo = np.flatnonzero(ppo_margins(c) & c.in_scope)
        if len(todo) == 0:
            break
    assert len(todo) == 0, f"{name}: the recipe could not leave the margins"
    if rotate_last:
        for f in ("value", "ret", "vold", "adv", "oldlogp"):
            getattr(c, f)[M - 1] = getattr(c, f)[0]
    c.tie_sets = {}
    return c


def _one_valid(c, s):
    if c.masks is not None:
        c.masks[s] = 0
        c.masks[s, int(c.actions[s])] = 1


def ppo_tie_case(name, R, clip, masked, M=12):
    """A smooth case with sets moved exactly onto the loss's kinks (module docstring); tie_sets:
    set -> kind ('ratio1', 'bound', 'vmax', 'same')."""
    c = ppo_case(name, M, R, masked, clip=clip)
    c.ties = True
    t = c.tie_sets

    def val(s, vold, v, ret, kind):
        c.vold[s], c.value[s], c.ret[s] = vold, v, ret
        t[s] = kind

    if R == 1 or masked:
        _one_valid(c, 0)
        c.oldlogp[0] = 0.0
        t[0] = "ratio1"
    if R == 1:
        c.oldlogp[1] = 0.0
        val(1, 0.5, 1.25, 1.0, "ratio1+vmax")
    if clip == 0.25 and M >= 8:
        val(3, 1.0, 1.25, 0.3, "bound")
        val(4, 0.5, 1.25, 1.0, "vmax")
        val(6, 1.0, 0.75, 2.0, "bound")
        val(7, 1.5, 0.75, 1.0, "vmax")
    if M >= 8:
        c.vold[5] = c.value[5]
        t[5] = "same"
    return c


def ppo_reference(c):
    """terms [M,6] float64, d mean-loss / d logits [M,R], d mean-loss / d value [M] (the mean
    over ALL M sets, as the kernel's 1 / M)."""
    from torch.distributions import Categorical
    if getattr(c, "_ref", None) is not None:
        return c._ref
    clip, ent_c, vf_c = float(F32(c.clip)), float(F32(c.ent_coef)), float(F32(c.vf_coef))
    d64 = lambda x: torch.from_numpy(np.asarray(x)).double()  # noqa: E731
    L = d64(c.logits).requires_grad_()
    V = d64(c.value).requires_grad_()
    Lm = L if c.masks is None else torch.where(torch.from_numpy(c.masks.astype(bool)), L,
                                               torch.full((), -1e8, dtype=torch.float64))
    dist = Categorical(logits=Lm)
    nlp = dist.log_prob(torch.from_numpy(c.actions.astype(np.int64)))
    logratio = nlp - d64(c.oldlogp)
    ratio = logratio.exp()
    A, ret, vold = d64(c.adv), d64(c.ret), d64(c.vold)
    pg = torch.max(-A * ratio, -A * torch.clamp(ratio, 1 - clip, 1 + clip))
    vu = (V - ret) ** 2
    if c.clip_vloss:
        vc = vold + torch.clamp(V - vold, -clip, clip)
        vt = torch.max(vu, (vc - ret) ** 2)
    else:
        vt = vu
    H = dist.entropy()
    kl = (ratio - 1) - logratio
    cf = ((ratio - 1).abs() > clip).double()
    loss = pg - ent_c * H + 0.5 * vf_c * vt
    loss.mean().backward()
    terms = torch.stack([pg, vt, H, kl, cf, loss], 1).detach().numpy()
    parts = (pg.abs() + ent_c * H.abs() + 0.5 * vf_c * vt.abs()).detach().numpy()
    c._ref = types.SimpleNamespace(terms=terms, dlogits=L.grad.numpy(), dvalue=V.grad.numpy(), parts=parts,
                                   ratio=ratio.detach().numpy(), nlp=nlp.detach().numpy())
    return c._ref


def ppo_buffers(c):
    return dict(dlogits=nan_buf(c.M * c.R), dvalue=nan_buf(c.M), terms=nan_buf(c.M * 6))


TERM_NAMES = ("pg", "vt", "entropy", "kl", "clipped", "loss")


def check_ppo(c, out):
    """Asserts; returns {quantity: worst error as a share of its allowance}."""
    M, R = c.M, c.R
    ref = ppo_reference(c)
    near = ppo_margins(c) & c.in_scope
    for s in c.tie_sets:
        near[s] = False
    assert not near.any(), f"{c.name}: sets {np.flatnonzero(near)[:8]} lie within the recipe's margins"
    dl = _written(out["dlogits"], M * R, f"{c.name}: dlogits").reshape(M, R)
    dv = _written(out["dvalue"], M, f"{c.name}: dvalue")
    tm = _written(out["terms"], M * 6, f"{c.name}: terms").reshape(M, 6)
    for what, x in (("dlogits", dl), ("dvalue", dv), ("terms", tm)):
        assert np.isfinite(x).all(), f"{c.name}: {what} not finite"
    sc = c.in_scope
    out_sets = np.flatnonzero(~sc)
    assert (dl[out_sets] == 0).all(), f"{c.name}: a set with no valid row got a logit gradient"
    if c.masks is not None:
        assert (dl[c.masks == 0] == 0).all(), f"{c.name}: a masked row got a gradient"
    shares = {}

    def take(key, got, exp, rtol, atol, where=None):
        s, i = _share(got, exp, rtol, atol)
        loc = i if where is None else where(i)
        assert s <= 1.0, (f"{c.name}: {key} at {loc}: got {np.asarray(got).flat[i]!r}, float64 "
                          f"{np.asarray(exp).flat[i]!r}, {s:.2f} of the allowance")
        shares[key] = s

    idx = np.flatnonzero(sc)
    per_set = lambda i: f"set {idx[i]}"  # noqa: E731
    for k, rtol in ((0, 1e-5), (1, 1e-5), (2, 1e-5), (3, 1e-4)):
        take(f"term {TERM_NAMES[k]}", tm[sc, k], ref.terms[sc, k], rtol, 1e-6, per_set)
    bad = np.flatnonzero(tm[sc, 4] != ref.terms[sc, 4])
    assert len(bad) == 0, f"{c.name}: clipped indicator differs on sets {idx[bad][:8]}"
    s5 = np.abs(tm[sc, 5].astype(np.float64) - ref.terms[sc, 5]) / (1e-6 + 1e-5 * ref.parts[sc])
    i5 = int(s5.argmax())
    assert s5[i5] <= 1.0, f"{c.name}: term loss at set {idx[i5]}: {s5[i5]:.2f} of the allowance"
    shares["term loss"] = float(s5[i5])
    gm, em = tm[sc].astype(np.float64).mean(0), ref.terms[sc].mean(0)
    for k, rtol in ((0, 1e-5), (1, 1e-5), (2, 1e-5), (3, 1e-4), (5, 1e-5)):
        scale = 0.5 if k == 1 else 1.0  # (v_loss = half the mean value term, as the learner logs it)
        take(f"mean {TERM_NAMES[k]}", scale * gm[k], scale * em[k], rtol, 1e-6)
    assert gm[4] == em[4], f"{c.name}: clipfrac {gm[4]} != {em[4]}"
    el, ev = ref.dlogits[sc], ref.dvalue[sc]
    take("dlogits", dl[sc], el, 1e-4, 1e-5 * float(np.abs(el).max()) + 1e-12,
         lambda i: f"set {idx[i // R]} row {i % R}")
    take("dvalue", dv[sc], ev, 1e-4, 1e-6 * float(np.abs(ev).max()) + 1e-12, per_set)
    return shares


def check_tie_recipe(c, ratio32=None):
    """The tie sets are ties in float64 (and, given a float32 ratio, in float32)."""
    ref = ppo_reference(c)
    clip = float(F32(c.clip))
    kinds = set()
    for s, kind in c.tie_sets.items():
        v, vo, rt = float(c.value[s]), float(c.vold[s]), float(c.ret[s])
        for k in kind.split("+"):
            kinds.add(k)
            if k == "ratio1":
                assert ref.nlp[s] == 0.0 and ref.ratio[s] == 1.0, (c.name, s)
                assert ratio32 is None or ratio32[s] == 1.0, (c.name, s)
            elif k == "bound":
                assert abs(v - vo) == clip and v != rt
            elif k == "vmax":
                assert abs(v - vo) > clip and (v - rt) ** 2 == (vo + np.clip(v - vo, -clip, clip) - rt) ** 2
            elif k == "same":
                assert v == vo and v != rt
    return kinds


def ppo_stand_in(c, bufs, bug=None):
    """The kernel's documented formula in torch float32 (explicit gradient, no autograd)."""
    M, R = c.M, c.R
    t = lambda x: torch.from_numpy(np.asarray(x, F32))  # noqa: E731
    clip, ent_c, vf_c = (float(F32(x)) for x in (c.clip, c.ent_coef, c.vf_coef))
    lo, hi = float(F32(1) - F32(c.clip)), float(F32(1) + F32(c.clip))
    inv_m = float(F32(1) / F32(M + 1 if bug == "wrong_m" else M))
    mask = torch.ones(M, R, dtype=torch.bool) if c.masks is None else torch.from_numpy(c.masks.astype(bool))
    lp = torch.log_softmax(torch.where(mask, t(c.logits), torch.full((), -1e8)), 1)
    pr = lp.exp()
    H = -(pr * lp).sum(1)
    a = torch.from_numpy(c.actions.astype(np.int64))
    pick = (a & 63) if bug == "low_bits" else a
    nlp = lp.gather(1, pick[:, None]).squeeze(1)
    logratio = nlp - t(c.oldlogp)
    ratio = logratio.exp()
    A = t(c.adv)
    rc = ratio.clamp(lo, hi)
    pg1, pg2 = -A * ratio, -A * rc
    half = 1.0 if bug == "tie_first" else 0.5
    w1 = torch.where(pg1 > pg2, 1.0, torch.where(pg1 == pg2, half, 0.0))
    inr = ((ratio > lo) & (ratio < hi)) if bug == "open_clamp" else ((ratio >= lo) & (ratio <= hi))
    g_nlp = inv_m * (w1 * -A + (1 - w1) * -A * inr.float()) * ratio
    ge = 0.0 if bug == "no_entropy_grad" else ent_c * inv_m
    onehot = torch.zeros(M, R).scatter_(1, a[:, None], 1.0)
    g = g_nlp[:, None] * (onehot - pr) + ge * pr * (lp + H[:, None])
    dl = g if bug == "masked_grad" else torch.where(mask, g, torch.zeros(()))
    v, rt, vo = t(c.value), t(c.ret), t(c.vold)
    vu = (v - rt) ** 2
    if c.clip_vloss:
        d = v - vo
        vc = vo + d.clamp(-clip, clip)
        vcl = (vc - rt) ** 2
        vt = torch.max(vu, vcl)
        wu = torch.where(vu > vcl, 1.0, torch.where(vu == vcl, half, 0.0))
        inv = ((d > -clip) & (d < clip)) if bug == "open_clamp" else ((d >= -clip) & (d <= clip))
        gv = wu * 2 * (v - rt) + (1 - wu) * 2 * (vc - rt) * inv.float()
    else:
        vt, gv = vu, 2 * (v - rt)
    dv = vf_c * 0.5 * inv_m * gv
    pgt = torch.max(pg1, pg2)
    terms = torch.stack([pgt, vt, H, (ratio - 1) - logratio, ((ratio - 1).abs() > clip).float(),
                         pgt - ent_c * H + vf_c * 0.5 * vt], 1)
    n = M - 1 if bug == "last_terms" else M
    bufs["dlogits"][:M * R] = dl.numpy().reshape(-1)
    bufs["dvalue"][:M] = dv.numpy()
    bufs["terms"][:n * 6] = terms.numpy().reshape(-1)[:n * 6]
    bufs["ratio32"] = ratio.numpy()
    return bufs


def _ppo_cases():
    cs = []
    # M = 517: 129 full blocks of 4 waves and a ragged one; (R, masked, clip_vloss, ent_coef)
    for R, masked, cv, ec in ((1, False, 1, 0.01), (2, True, 1, 0.01), (9, True, 0, 0.01), (9, False, 1, 0.0),
                              (63, True, 1, 0.01), (64, False, 1, 0.01), (64, True, 0, 0.0), (65, True, 1, 0.01),
                              (128, False, 0, 0.01), (129, True, 1, 0.0), (256, True, 1, 0.01),
                              (257, False, 1, 0.01), (257, True, 0, 0.01)):
        name = f"M517-R{R}" + ("-masks" if masked else "") + ("" if cv else "-noclipv") + ("" if ec else "-ent0")
        cs.append(ppo_case(name, 517, R, masked, cv, ec))
    for M in (1, 3, 4, 5):
        cs.append(ppo_case(f"M{M}-R9" + ("-masks" if M & 1 else ""), M, 9, bool(M & 1)))
        cs.append(ppo_case(f"M{M}-R65" + ("" if M & 1 else "-masks"), M, 65, not M & 1))
    # more sets than 8192 blocks x 4 waves: waves loop (s += nw), the tail is ragged
    cs.append(ppo_case("M32773-R3-masks-loop", 4 * 8192 + 5, 3, True, rotate_last=True))
    cs.append(ppo_tie_case("ties-R9-clip0.25-masks", 9, 0.25, True))
    cs.append(ppo_tie_case("ties-R9-clip0-masks", 9, 0.0, True))
    cs.append(ppo_tie_case("ties-R65-clip0.25-masks", 65, 0.25, True))
    cs.append(ppo_tie_case("ties-R1-clip0.25", 1, 0.25, False, M=5))
    return cs


_PPO = None


def ppo_cases():
    """name -> case; built once and shared (the float64 reference is cached on the case)."""
    global _PPO
    if _PPO is None:
        _PPO = {c.name: c for c in _ppo_cases()}
    return _PPO


PPO_CASE_NAMES = (["M517-R1", "M517-R2-masks", "M517-R9-masks-noclipv", "M517-R9-ent0", "M517-R63-masks", "M517-R64",
                   "M517-R64-masks-noclipv-ent0", "M517-R65-masks", "M517-R128-noclipv", "M517-R129-masks-ent0",
                   "M517-R256-masks", "M517-R257", "M517-R257-masks-noclipv"]
                  + [n for M in (1, 3, 4, 5) for n in (f"M{M}-R9" + ("-masks" if M & 1 else ""),
                                                       f"M{M}-R65" + ("" if M & 1 else "-masks"))]
                  + ["M32773-R3-masks-loop", "ties-R9-clip0.25-masks", "ties-R9-clip0-masks",
                     "ties-R65-clip0.25-masks", "ties-R1-clip0.25"])


def run_ppo(dev, name):
    c = ppo_cases()[name]
    return check_ppo(c, dev.ppo_head(c, ppo_buffers(c)))


# ================================ DQN head ====================================================

GAMMA = 0.99
# (M, R, dones, td/old NULL): both kernels at M <= 1024 (loss_out given / NULL), the wave kernel
# alone above; M = 4 * 65535 + 5 loops inside k_dqn_head (its grid stops at 65535 blocks)
DQN_CASES = [(1, 1, "mixed", False), (1, 257, "ones", False), (5, 2, "zeros", False), (63, 63, "mixed", False),
             (64, 64, "ones", False), (65, 65, "mixed", False), (65, 65, "mixed", True), (128, 128, "zeros", False),
             (1024, 65, "mixed", False), (1025, 63, "mixed", False), (2000, 257, "mixed", False),
             (4 * 65535 + 5, 1, "mixed", False)]


def dqn_case_id(spec):
    M, R, dones, null = spec
    return f"M{M}-R{R}-{dones}" + ("-null" if null else "")


def dqn_case(spec):
    M, R, dones, null = spec
    rng = _rng(dqn_case_id(spec))
    c = types.SimpleNamespace(name=dqn_case_id(spec), M=M, R=R, null=null, gamma=GAMMA)
    c.q = rng.standard_normal((M, R)).astype(F32)
    c.q_next = rng.standard_normal((M, R)).astype(F32)
    c.actions = rng.integers(0, R, M).astype(np.int64)
    c.actions[0] = 0
    c.actions[M - 1] = R - 1
    c.rewards = rng.standard_normal(M).astype(F32)
    c.dones = {"zeros": np.zeros(M, F32), "ones": np.ones(M, F32),
               "mixed": (rng.random(M) < 0.3).astype(F32)}[dones]
    if dones == "mixed" and M == 1:
        c.dones[:] = 0
    c.twice = np.zeros(M, bool)
    if R >= 2:  # every third set attains its q_next maximum twice
        s = np.arange(0, M, 3)
        top = c.q_next[s].argmax(1)
        c.q_next[s, (top + 1 + rng.integers(0, R - 1, len(s))) % R] = c.q_next[s, top]
        c.twice[s] = True
    c.kernels = ("block", "wave") if M <= 1024 else ("wave",)
    return c


def dqn_reference(c):
    import torch.nn.functional as F
    q = torch.from_numpy(c.q).double().requires_grad_()
    a = torch.from_numpy(c.actions)[:, None]
    td = (torch.from_numpy(c.rewards).double()
          + float(F32(c.gamma)) * torch.from_numpy(c.q_next).double().max(1)[0]
          * (1 - torch.from_numpy(c.dones).double()))
    old = q.gather(1, a).squeeze(1)
    loss = F.mse_loss(td, old)
    loss.backward()
    return types.SimpleNamespace(td=td.numpy(), old=old.detach().numpy(), sq=((td - old) ** 2).detach().numpy(),
                                 loss=float(loss.detach()), dq=q.grad.numpy())


def dqn_buffers(c, block):
    return dict(dq=nan_buf(c.M * c.R), sq_err=nan_buf(c.M), td=None if c.null else nan_buf(c.M),
                old=None if c.null else nan_buf(c.M), loss=nan_buf(1) if block else None)


def check_dqn(c, ref, out, block):
    M, R, what = c.M, c.R, f"{c.name} ({'block' if block else 'wave'} kernel)"
    dq = _written(out["dq"], M * R, f"{what}: dq").reshape(M, R)
    sq = _written(out["sq_err"], M, f"{what}: sq_err")
    shares = {}

    def take(key, got, exp, rtol, atol):
        s, i = _share(got, exp, rtol, atol)
        assert s <= 1.0, (f"{what}: {key} at {i}: got {np.asarray(got).flat[i]!r}, float64 "
                          f"{np.asarray(exp).flat[i]!r}, {s:.2f} of the allowance")
        shares[key] = s

    if not c.null:
        take("td", _written(out["td"], M, f"{what}: td"), ref.td, 1e-6, 1e-6)
        old = _written(out["old"], M, f"{what}: old")
        np.testing.assert_array_equal(old, c.q[np.arange(M), c.actions], err_msg=f"{what}: old != q[a]")
    on = np.zeros((M, R), bool)
    on[np.arange(M), c.actions] = True
    assert (dq[~on] == 0).all(), f"{what}: dq off the action's column is not 0"
    take("dq", dq[on], ref.dq[on], 1e-5, 1e-7)
    take("sq_err", sq, ref.sq, 1e-5, 1e-6)
    mean = sq.astype(np.float64).sum() / M
    if block:
        loss = _written(out["loss"], 1, f"{what}: loss")[0]
        take("loss", loss, ref.loss, 1e-5, 1e-6)
        take("loss vs own sq_err", loss, F32(mean), 1.2e-7, 0.0)
    else:
        take("loss", mean, ref.loss, 1e-5, 1e-6)
    return shares


def run_dqn(dev, spec):
    """Both kernels where both can run; returns ({kernel: shares}, bitwise: True | None)."""
    c = dqn_case(spec)
    ref = dqn_reference(c)
    outs, shares = {}, {}
    for k in c.kernels:
        outs[k] = dev.dqn_head(c, dqn_buffers(c, k == "block"), k == "block")
        shares[k] = check_dqn(c, ref, outs[k], k == "block")
    if len(outs) < 2:
        return shares, None
    for f in ("dq", "sq_err") if c.null else ("td", "old", "sq_err", "dq"):
        a, b = outs["block"][f], outs["wave"][f]
        diff = np.flatnonzero(a.view(np.uint32) != b.view(np.uint32))
        assert len(diff) == 0, (f"{c.name}: the two kernels differ in {f} at {diff[:8]}: "
                                f"{a[diff[:4]]!r} (block) / {b[diff[:4]]!r} (wave)")
    return shares, True


def dqn_stand_in(c, bufs, block, bug=None):
    M, R = c.M, c.R
    keep = F32(1) if bug == "no_done" else F32(1) - c.dones
    td = c.rewards + F32(c.gamma) * c.q_next.max(1) * keep
    old = c.q[np.arange(M), c.actions]
    g = (F32(2) / F32(M)) * (old - td)
    dq = bufs["dq"][:M * R].reshape(M, R)
    if bug != "dq_sparse":
        dq[:] = 0
    dq[np.arange(M), c.actions] = g
    bufs["sq_err"][:M] = (td - old) * (td - old)
    if bufs["td"] is not None:
        bufs["td"][:M] = td
    if bufs["old"] is not None:
        bufs["old"][:M] = old
    if block:
        bufs["loss"][0] = F32(bufs["sq_err"][:M].astype(np.float64).sum() / M)
    return bufs


# ================================ episode log =================================================

EPLOG_W, ST_K = 24, 16
COL_RET32, COL_REWARD, COL_ACTION, COL_ENV, COL_TAG = 16, 17, 18, 19, 20
CALLS = 3
EPLOG_B = (1, 63, 64, 65, 255, 256, 257, 1000)
EPLOG_PATTERNS = ("none", "all", "lane63", "last", "wave", "random")


def done_pattern(pattern, B, rng):
    """(B,) uint8 or None where B has no such env."""
    d = np.zeros(B, np.uint8)
    if pattern == "all":
        d[:] = 1
    elif pattern == "lane63":      # the last lane of the first wave alone
        if B < 64:
            return None
        d[63] = 1
    elif pattern == "last":
        d[B - 1] = 1
    elif pattern == "wave":        # wave 1 of block 0 whole, waves 0, 2 and 3 of that block empty
        if B < 256:
            return None
        d[64:128] = 1
    elif pattern == "random":
        d[:] = rng.random(B) < 0.3
    return d


def rounding_pairs(n, rng):
    """n (ret32, r64) pairs with float32(float64(ret32) + r64) != ret32 + float32(r64)."""
    ret, r64 = np.zeros(0, F32), np.zeros(0)
    while len(ret) < n:
        a = (rng.standard_normal(8 * n + 64) * 3).astype(F32)
        b = rng.standard_normal(8 * n + 64) * 0.7
        hit = (a.astype(np.float64) + b).astype(F32) != a + b.astype(F32)
        ret, r64 = np.concatenate([ret, a[hit]]), np.concatenate([r64, b[hit]])
    return ret[:n].copy(), r64[:n].copy()


def once_vs_twice(ret32, r64):
    return (ret32.astype(np.float64) + r64).astype(F32) != ret32 + r64.astype(F32)


def eplog_specs():
    """(B, pattern, reward64 given, ep_r32 given, cap mode); cap: ample / exact / short / zero."""
    specs = []
    for i, B in enumerate(EPLOG_B):
        for j, p in enumerate(EPLOG_PATTERNS):
            if done_pattern(p, B, np.random.default_rng(0)) is not None:
                specs.append((B, p, bool((i + j) & 1) or p == "random", True, "ample"))
    for B in (65, 257, 1000):
        for cap in ("exact", "short", "zero"):
            specs.append((B, "random", True, True, cap))
    specs += [(257, "all", True, True, "short"), (256, "wave", False, True, "short"),
              (257, "random", True, False, "ample"), (1000, "random", False, False, "short"),
              (1000, "random", False, True, "ample"), (64, "all", False, True, "exact")]
    return specs


def eplog_id(spec):
    B, p, r64, epr, cap = spec
    return f"B{B}-{p}-{'r64' if r64 else 'r32'}" + ("" if epr else "-noepr") + ("" if cap == "ample" else f"-{cap}")


def eplog_case(spec):
    """The CALLS calls' inputs of a case, its initial ret32 and its cap."""
    B, pattern, with64, with_epr, capmode = spec
    rng = _rng(eplog_id(spec))
    c = types.SimpleNamespace(name=eplog_id(spec), B=B, with64=with64, with_epr=with_epr, calls=[])
    c.ret32, r64_first = rounding_pairs(B, rng)   # every env rounding-sensitive at the first call
    total = 0
    for k in range(CALLS):
        r64 = r64_first if k == 0 else rng.standard_normal(B) * 0.7
        done = done_pattern(pattern, B, rng)
        total += int(done.sum())
        c.calls.append(types.SimpleNamespace(
            tag=k, done=done, r64=r64, reward=r64.astype(F32), actions=rng.integers(0, 9, B).astype(np.int32),
            ep_stats=rng.standard_normal((B, ST_K))))
    c.total = total
    c.cap = {"ample": total + 3, "exact": total, "short": total // 2, "zero": 0}[capmode]
    c.sensitive = int(once_vs_twice(c.ret32, r64_first).sum())
    return c


def run_eplog(dev, spec):
    """CALLS consecutive calls (tags 0, 1, 2; ret32 carried over, *count accumulating), each
    compared with the exact reference."""
    c = eplog_case(spec)
    B, cap = c.B, c.cap
    ret_ref = c.ret32.copy()
    ret_dev = c.ret32.copy()
    epr_ref = np.arange(B, dtype=F32) - 5000 if c.with_epr else None   # (distinct fills: a stray write shows)
    epr_dev = None if epr_ref is None else epr_ref.copy()
    log = np.full((cap + GUARD, EPLOG_W), np.nan)
    count = np.zeros(1, np.uint32)
    expected, per_tag, total = {}, [], 0
    for call in c.calls:
        what = f"{c.name} call {call.tag}"
        r32 = ((ret_ref.astype(np.float64) + call.r64).astype(F32) if c.with64 else ret_ref + call.reward)
        fin = call.done != 0
        for e in np.flatnonzero(fin):
            expected[(call.tag, int(e))] = np.concatenate(
                [call.ep_stats[e], [float(r32[e]), float(call.reward[e]), float(call.actions[e]), float(e),
                                    float(call.tag)]])
        if epr_ref is not None:
            epr_ref[fin] = r32[fin]
        ret_ref = np.where(fin, F32(0), r32).astype(F32)
        n_fin = int(fin.sum())
        per_tag.append(min(max(cap - total, 0), n_fin))
        total += n_fin
        ret_dev, epr_dev, log, count = dev.episode_log(
            B, call.done.copy(), call.ep_stats.copy(), call.reward.copy(), call.r64.copy() if c.with64 else None,
            call.actions.copy(), ret_dev, epr_dev, call.tag, log, cap, count)
        np.testing.assert_array_equal(np.asarray(ret_dev).view(np.uint32), ret_ref.view(np.uint32),
                                      err_msg=f"{what}: ret32")
        if epr_ref is not None:
            np.testing.assert_array_equal(np.asarray(epr_dev).view(np.uint32), epr_ref.view(np.uint32),
                                          err_msg=f"{what}: ep_r32")
        assert int(count[0]) == total, f"{what}: count {int(count[0])} != {total} episodes finished"
        log = np.asarray(log)
        n = min(cap, total)
        assert np.isnan(log[n:]).all(), f"{what}: a row written past min(cap, count) = {n}"
        rows = log[:n]
        assert not np.isnan(rows[:, :COL_TAG + 1]).any(), f"{what}: a row below min(cap, count) = {n} not written"
        keys = [(int(r[COL_TAG]), int(r[COL_ENV])) for r in rows]
        assert len(set(keys)) == len(keys), f"{what}: an env logged twice within a tag"
        order = sorted(range(n), key=lambda i: keys[i])
        for i in order:
            assert keys[i] in expected, f"{what}: row {i} logs {keys[i]}, which did not finish"
            np.testing.assert_array_equal(rows[i, :COL_TAG + 1], expected[keys[i]],
                                          err_msg=f"{what}: row {i} (tag, env) = {keys[i]}")
        got = [sum(1 for k in keys if k[0] == t) for t in range(len(per_tag))]
        assert got == per_tag, f"{what}: rows per tag {got} != {per_tag}"
    return c


def eplog_stand_in(B, done, ep_stats, reward, reward64, actions, ret32, ep_r32, tag, log, cap, count, bug=None):
    if reward64 is not None and bug != "two_roundings":
        r32 = (ret32.astype(np.float64) + reward64).astype(F32)
    else:
        r32 = ret32 + reward
    fin = done != 0
    for w0 in range(0, B, 64):     # one wave at a time, as the kernel reserves its rows
        envs = w0 + np.flatnonzero(fin[w0:w0 + 64])
        base = int(count[0])
        count[0] += len(envs)
        for k, e in enumerate(envs):
            slot = base + k
            if slot >= cap + (1 if bug == "past_cap" else 0):
                continue
            log[slot, :ST_K] = ep_stats[e]
            log[slot, ST_K:COL_TAG + 1] = (r32[e], reward[e], actions[e], e, tag)
    if bug == "count_capped":
        count[0] = min(int(count[0]), cap)
    if ep_r32 is not None:
        ep_r32[fin] = r32[fin]
    ret32 = r32 if bug == "no_restart" else np.where(fin, F32(0), r32).astype(F32)
    return ret32, ep_r32, log, count


# ================================ replay sample ===============================================

HI = (1 << 32) + 7
# (name, B, obs_floats, slots, batch, vstep, base_adds)
SAMPLE_CASES = [
    ("empty-B300-F72-n512", 300, 72, 6, 512, 0, 0),
    ("empty-B1-F4-n1", 1, 4, 6, 1, 0, 0),
    ("hi-part-B300-F4-n5", 300, 4, 6, 5, HI, 3 - HI),
    ("hi-part-B300-F72-n512", 300, 72, 6, 512, HI, 3 - HI),
    ("hi-full-B300-F72-n512", 300, 72, 6, 512, HI, 100),
    ("lo-part-B300-F72-n512", 300, 72, 6, 512, 7, 3 - 7),
    ("part-B1-F2056-n5", 1, 2056, 4, 5, 2, 1),
    ("full-B300-F2056-n1", 300, 2056, 4, 1, 9, 0),
    ("full-B300-F2056-n5", 300, 2056, 4, 5, 9, 0),
    ("part-B1-F72-n512", 1, 72, 6, 512, 3, 2),
    ("full-B300-F4-n512", 300, 4, 6, 512, 11, 5),
]
SAMPLE_SEED = 0x1234567899


def sample_case(spec):
    name, B, F, S, batch, vstep, base = spec
    return types.SimpleNamespace(name=name, B=B, F=F, S=S, batch=batch, vstep=vstep, base=base, seed=SAMPLE_SEED,
                                 threads=batch * (F // 2 + 1))


def sample_upper(c):
    adds = c.base + c.vstep
    return min(max(adds, 1), c.S)


_RINGS = {}


def sample_ring(c):
    """Every field of row (slot, env) encodes slot * B + env (< 2048); an observation float adds
    its index / 4096 (< 1): exact in float32, so a float taken from the wrong row or the wrong
    place in the row shows.  next_obs is the negative."""
    key = (c.B, c.F, c.S)
    if key not in _RINGS:
        assert c.S * c.B < 2048 and c.F < 4096
        rid = np.arange(c.S * c.B, dtype=np.float64).reshape(c.S, c.B)
        obs = (rid[:, :, None] + np.arange(c.F) / 4096.0).astype(F32)
        _RINGS[key] = dict(rb_obs=obs, rb_next_obs=-obs, rb_actions=rid.astype(np.int64) + 7,
                           rb_rewards=(rid + 0.25).astype(F32), rb_dones=(rid + 0.75).astype(F32))
    return _RINGS[key]


def sample_buffers(c):
    return dict(obs=nan_buf(c.batch * c.F), next_obs=nan_buf(c.batch * c.F),
                actions=np.full(c.batch + GUARD, SENTINEL_I64, np.int64), rewards=nan_buf(c.batch),
                dones=nan_buf(c.batch))


def check_sample(c, out, oracle_mod):
    n, F = c.batch, c.F
    ring = sample_ring(c)
    upper = sample_upper(c)
    slot, env = oracle_mod.replay_sample(c.seed, c.vstep, upper, c.B, n)
    assert ((slot >= 0) & (slot < upper) & (env >= 0) & (env < c.B)).all()
    obs = _written(out["obs"], n * F, f"{c.name}: obs_out").reshape(n, F)
    nxt = _written(out["next_obs"], n * F, f"{c.name}: next_obs_out").reshape(n, F)
    rew = _written(out["rewards"], n, f"{c.name}: rewards_out")
    don = _written(out["dones"], n, f"{c.name}: dones_out")
    act = np.asarray(out["actions"])
    assert (act[:n] != SENTINEL_I64).all(), f"{c.name}: actions_out left unwritten"
    assert (act[n:] == SENTINEL_I64).all(), f"{c.name}: actions_out written past its end"
    got_row = np.floor(obs[:, 0]).astype(np.int64)
    np.testing.assert_array_equal(got_row // c.B, slot, err_msg=f"{c.name}: slots drawn")
    np.testing.assert_array_equal(got_row % c.B, env, err_msg=f"{c.name}: envs drawn")
    eq = np.testing.assert_array_equal
    eq(obs, ring["rb_obs"][slot, env], err_msg=f"{c.name}: obs_out")
    eq(nxt, ring["rb_next_obs"][slot, env], err_msg=f"{c.name}: next_obs_out")
    eq(act[:n], ring["rb_actions"][slot, env], err_msg=f"{c.name}: actions_out")
    eq(rew, ring["rb_rewards"][slot, env], err_msg=f"{c.name}: rewards_out")
    eq(don, ring["rb_dones"][slot, env], err_msg=f"{c.name}: dones_out")
    return slot, env


def run_sample(dev, spec, oracle_mod):
    c = sample_case(spec)
    return check_sample(c, dev.replay_sample(c, sample_ring(c), sample_buffers(c)), oracle_mod)


def sample_stand_in(c, ring, bufs, oracle_mod, bug=None):
    n, F = c.batch, c.F
    adds = c.base + c.vstep
    upper = min(adds, c.S) if bug == "unclamped" else sample_upper(c)
    t = c.vstep & 0xFFFFFFFF if bug == "low_word" else c.vstep
    slot, env = oracle_mod.replay_sample(c.seed, t, upper, c.B, n)
    ok = slot < upper if bug == "unclamped" else np.ones(n, bool)   # (a gather bounded by the raw upper)
    i = np.flatnonzero(ok)
    bufs["obs"][:n * F].reshape(n, F)[i] = ring["rb_obs"][slot[i], env[i]]
    bufs["next_obs"][:n * F].reshape(n, F)[i] = ring["rb_next_obs"][slot[i], env[i]]
    bufs["actions"][:n][i] = ring["rb_actions"][slot[i], env[i]]
    bufs["rewards"][:n][i] = ring["rb_rewards"][slot[i], env[i]]
    bufs["dones"][:n][i] = ring["rb_dones"][slot[i], env[i]]
    return bufs
