"""The reference side of the fused deep-sets forward family (k_deepsets_fwd<TS, P, MODE, XR> and
k_ds_fwd_pair<1, P>, csrc/lbk8s_deepsets.h), for the tests that pin every variant with more than
one set per wave (P = 2, 4) to float64: tests/test_gpu_ds_variants.py runs the HIP kernels
through these checkers, tests/test_ds_ref_harness.py a float32 torch stand-in on the CPU.

Everything here is plain torch / numpy on the CPU:
  * the reference is the project's own modules (DeepSetAgent, DQNDeepSetAgent) deep-copied to
    float64; with autograd, every parameter gradient of a fixed random linear functional of the
    outputs (training) or of the DQN loss head (the paired forward);
  * the case table, shared by the CPU and the GPU tests: batch sizes follow the device's CU count
    C (the launchers halve P while ceil(B / P) < 4 C), B4 = 16 C + 3 (P = 4; the last group holds
    three live sets), B2 = 8 C + 1 (P = 2; the last group holds one), B8 = 32 C + 5 (more groups
    of four than the grid's 8 C waves: waves loop), B1 = 300 and 128 (one set per wave);
  * the input recipes;
  * the checkers, which take the device's outputs as numpy arrays.

Tolerances are the project's own: the inference forward's is tests/test_gpu_fused.near (rtol
1e-4, atol 2e-5 + 4e-6 max|expected|); the training forward's and the gradients' are
tests/test_gpu_fused_train._check (forward 1e-4 / 4e-6 max|expected|; gradients 1e-3 / 1e-4
max|expected| per tensor); the greedy action's are dqn_ref.action_tol and
dqn_ref.MAX_DISAGREE_SHARE.  A checker returns the worst |error| / allowed error it saw (<= 1).
"""
import collections
import copy
import functools

import numpy as np
import torch

import dqn_ref

FWD, FWD_TRAIN, FWD_ARGMAX, FWD_PAIR = 0, 1, 2, 3  # lb_ds_forward_kernel's `which`
GAMMA = 0.99  # the paired forward's DQN loss head


# ---- recipes shared with tests/test_gpu_fused_train.py ------------------------------------------
def _inputs(B, R, seed, ties=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, R, 8, generator=g) * torch.linspace(0.5, 3.0, 8) + 0.2
    x = torch.round(x * 4) / 4
    if ties:
        # observation-like structure: request columns equal on every row, integer zone ids,
        # duplicated rows (exact ties in every set-wise max)
        x[:, :, 5:] = x[:, :1, 5:]
        x[:, :, 0] = torch.randint(0, 4, (B, R), generator=g).float()
        if R > 2:
            x[:, 1] = x[:, 0]
    return x


def _agent(seed):
    from lbk8s.deepsets import DeepSetAgent
    torch.manual_seed(seed)
    agent = DeepSetAgent(8)
    with torch.no_grad():  # larger, asymmetric weights than the default init
        for p in agent.parameters():
            p.mul_(1.5).add_(0.01)
            p.copy_(torch.round(p * 32) / 32)
    return agent


def _qnet(seed):
    """The DQN Q network with weights in multiples of 1/32 (test_train_step_actor_only_and_many_sets)."""
    from lbk8s.deepsets import DQNDeepSetAgent
    torch.manual_seed(seed)
    q = DQNDeepSetAgent(8)
    with torch.no_grad():
        for p in q.parameters():
            p.copy_(torch.round(p * 32) / 32)
    return q


# ---- the case table ---------------------------------------------------------------------------
def device_cus():
    """The CU count the launchers weigh the batch against (256 without a device, as the library)."""
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def batch(name):
    c = device_cus()
    return {"B1": 300, "B128": 128, "B2": 8 * c + 1, "B4": 16 * c + 3, "B8": 32 * c + 5}[name]


# family: infer / train / argmax / pair; variant: the (TS, P, XR) the case must run; heads: "ac"
# (actor + critic) or "a" (actor only)
Case = collections.namedtuple("Case", "family heads R bname variant ties")


def case_id(c):
    ts, p, xr = c.variant
    return (f"{c.family}-{c.heads}-ts{ts}p{p}" + ("xr" if xr else "") + f"-R{c.R}-{c.bname}" +
            ("-ties" if c.ties else ""))


SMALL = (1, 2, 3, 7, 8, 15, 16)   # one 16-row tile: a lone row, ragged tiles, the full tile
TWO_TILES = (17, 24, 31, 32)
# (R, batch, variant) of the inference and the training forwards
_MATRIX = ([(R, "B4", (1, 4, 0)) for R in SMALL] + [(R, "B2", (1, 2, 0)) for R in SMALL] +
           [(R, "B2", (2, 2, 0)) for R in TWO_TILES] + [(R, "B8", (1, 4, 0)) for R in (9, 16)])

INFER_CASES = [Case("infer", h, R, b, v, False) for h in ("ac", "a") for R, b, v in _MATRIX]
TRAIN_CASES = [Case("train", h, R, b, v, t) for h in ("ac", "a") for R, b, v in _MATRIX for t in (False, True)]
ARGMAX_CASES = ([Case("argmax", "a", R, "B2", (1, 2, 0), False) for R in (1, 2, 7, 9, 15, 16)] +
                [Case("argmax", "a", R, "B2", (2, 2, 0), False) for R in (17, 20, 31, 32)] +
                [Case("argmax", "a", R, "B1", v, False)
                 for R, v in ((1, (1, 1, 0)), (16, (1, 1, 0)), (17, (2, 1, 0)), (32, (2, 1, 0)), (33, (3, 1, 0)),
                              (80, (5, 1, 0)), (81, (0, 1, 0)), (257, (0, 1, 0)))])
PAIR_CASES = [Case("pair", "a", R, b, (1, p, 0), False)
              for R in (1, 2, 7, 15, 16) for b, p in (("B128", 1), ("B2", 2), ("B4", 4))]
WHICH = {"infer": FWD, "train": FWD_TRAIN, "argmax": FWD_ARGMAX, "pair": FWD_PAIR}


def seed_of(c):
    return 1000 * c.R + 10 * (c.variant[1] + 5 * c.variant[0]) + len(c.bname) + (3 if c.ties else 0) + \
        (1 if c.heads == "a" else 0)


# ---- inputs and networks --------------------------------------------------------------------------
NEG_CHANNELS = (2, 6)  # all rows negative in every fourth set


def infer_inputs(B, R, seed):
    """test_gpu_fused.py's recipe, then: in every fourth set (set 0 among them) two channels are
    negative on every row, so a zero from a padded row or from a dead set would win the max; the
    last four sets (every live set of a ragged last group, P <= 4) are set 0 with its rows
    rotated, so an output selected from another set's column shows."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, R, 8, generator=g) * torch.linspace(0.5, 3.0, 8) + 0.2
    for ch in NEG_CHANNELS:
        x[0::4, :, ch] = -x[0::4, :, ch].abs() - 0.125
    for j in range(min(4, B - 1)):
        x[B - 1 - j] = torch.roll(x[0], j + 1, 0)
    return x


def _scaled(module, seed):
    torch.manual_seed(seed)
    m = module(8)
    with torch.no_grad():  # larger, asymmetric weights than the default init (test_gpu_fused.py)
        for p in m.parameters():
            p.mul_(1.5).add_(0.01)
    return m


def infer_agent(seed):
    from lbk8s.deepsets import DeepSetAgent
    return _scaled(DeepSetAgent, seed)


def infer_qnet(seed):
    from lbk8s.deepsets import DQNDeepSetAgent
    return _scaled(DQNDeepSetAgent, seed)


def argmax_inputs(B, R, seed):
    """infer_inputs, then duplicated rows in every eighth set (exact Q ties: the first row wins),
    set 5 and the batch's last set with every row equal."""
    x = infer_inputs(B, R, seed)
    if R > 1:
        x[2::8, R // 2] = x[2::8, 0]
    x[5] = x[5, :1]
    x[B - 1] = x[B - 1, :1]
    return x


def argmax_masks(B, R, seed, last):
    """(B, R) bool, ~30 % invalid; set 5 (equal rows) all valid, set 7 nothing valid, set 9 only
    row R - 1 valid; the batch's last set (alone in its group at B2) is one of the three:
    last = "equal" (all valid on its equal rows), "none" or "only_last"."""
    m = torch.rand(B, R, generator=torch.Generator().manual_seed(seed + 17)) > 0.3
    m[5] = True
    m[7] = False
    m[9] = False
    m[9, R - 1] = True
    m[B - 1] = last == "equal"
    if last == "only_last":
        m[B - 1, R - 1] = True
    return m


LAST_SETS = ("equal", "none", "only_last")


# ---- training inputs without near-ties ------------------------------------------------------------
# The pooled gradient goes to the first row attaining a set-wise max, so a parameter gradient is
# discontinuous where two different rows hold (nearly) the same hidden value: float32 and float64
# may then route one set's gradient to different rows, and one set is 1 / sqrt(B) of a gradient
# that sums B randomly signed sets -- far above the gradients' tolerance.  The quantised recipes
# rule this out where the hidden values are exact in float32 (the actor's ReLU layer); an ELU
# output is not (the critic's first layer, every second layer), and among B4 x 64 features x R
# rows a few such near-ties do occur.  The training cases therefore redraw every set in which, in
# float64, the runner-up of a pooled max lies within TIE_MARGIN (1 + |max|) of it without being
# equal to it: five times the absolute error floor the project grants the forward (4e-6 max|out|),
# of which a float32 forward uses about a tenth.  Exact ties (duplicated rows, ReLU
# zeros; to 1e-12, a float64 GEMM's own rounding between equal rows) stay: there the first row
# wins in every precision.  So does a near-tie at a max below -1 + 1e-3, an ELU output in
# saturation: the routed gradient is multiplied by the activation's slope there, max + 1 < 1e-3,
# which puts one set's share under a tenth of the gradients' absolute floor.
TIE_MARGIN = 2e-5


def _stacks(net64):
    return [net64.actor.net, net64.critic.psi] if hasattr(net64, "actor") else [net64.q_network.net]


@torch.no_grad()
def near_tie_sets(net64, x64):
    """(B,) bool: sets with a near-tie in a pooled max of a hidden layer (see above)."""
    bad = torch.zeros(x64.shape[0], dtype=torch.bool)
    for net in _stacks(net64):
        h = x64
        for j in (0, 2):
            h = net[j + 1](net[j](h))  # the input of layer j + 2, pooled there
            top = h.max(1, keepdim=True).values
            scale = 1 + top.abs()
            below = torch.where(h < top - 1e-12 * scale, h, torch.full_like(h, -float("inf")))
            second = below.max(1, keepdim=True).values
            bad |= (((top - second) <= TIE_MARGIN * scale) & (top > -1 + 1e-3)).flatten(1).any(1)
    return bad


def train_inputs(net, B, R, seed, ties):
    """_inputs(B, R, seed, ties) with every near-tie set replaced by the same set of a later draw."""
    n64 = copy.deepcopy(net).double()
    x = _inputs(B, R, seed, ties)
    todo = torch.arange(B)
    for k in range(1, 40):
        todo = todo[near_tie_sets(n64, x[todo].double())]
        if not len(todo):
            return x
        x[todo] = _inputs(B, R, seed + 7919 * k, ties)[todo]
    raise AssertionError(f"near-ties left in {len(todo)} sets")


# ---- the float64 reference ------------------------------------------------------------------------
def functional(B, R, seed):
    """The fixed random linear functional of (logits, value): weights (B, R) and (B,)."""
    g = torch.Generator().manual_seed(seed + 1000)
    return torch.randn(B, R, generator=g), torch.randn(B, generator=g)


def _np(t):
    return t.detach().cpu().double().numpy()


def _grads(module):
    return {n: _np(p.grad) for n, p in module.named_parameters()}


Setup = collections.namedtuple("Setup", "case B net x extra ref")


@functools.lru_cache(maxsize=4)
def setup(c):
    """Inputs, the float32 network and the float64 reference of a case (computed once)."""
    B, R, seed = batch(c.bname), c.R, seed_of(c)
    ref = {}
    if c.family == "infer":
        net = infer_agent(seed) if c.heads == "ac" else infer_qnet(seed)
        x = infer_inputs(B, R, seed)
        n64 = copy.deepcopy(net).double()
        with torch.no_grad():
            if c.heads == "ac":
                ref["logits"], ref["value"] = _np(n64.actor(x.double())), _np(n64.critic(x.double()))
            else:
                ref["logits"] = _np(n64.q_network(x.double()))
        return Setup(c, B, net, x, None, ref)
    if c.family == "train":
        net = _agent(seed) if c.heads == "ac" else _qnet(seed)
        x = train_inputs(net, B, R, seed, c.ties)
        wl, wv = functional(B, R, seed)
        n64 = copy.deepcopy(net).double()
        if c.heads == "ac":
            lg, v = n64.actor(x.double()), n64.critic(x.double())
            ((lg * wl.double()).sum() + (v * wv.double()).sum()).backward()
            ref["value"] = _np(v)
        else:
            lg = n64.q_network(x.double())
            (lg * wl.double()).sum().backward()
        ref["logits"], ref["grads"] = _np(lg), _grads(n64)
        return Setup(c, B, net, x, (wl, wv), ref)
    if c.family == "argmax":
        net = infer_qnet(seed)
        x = argmax_inputs(B, R, seed)
        with torch.no_grad():
            ref["q"] = _np(copy.deepcopy(net).double().q_network(x.double()))
        return Setup(c, B, net, x, None, ref)
    assert c.family == "pair"
    net, target = _qnet(seed), _qnet(seed + 1)
    x, xn = train_inputs(net, B, R, seed, True), _inputs(B, R, seed + 1, False)
    g = torch.Generator().manual_seed(seed + 2)
    a = torch.randint(0, R, (B, 1), generator=g)
    r, d = torch.rand((B, 1), generator=g), (torch.rand((B, 1), generator=g) < 0.2).float()
    n64 = copy.deepcopy(net).double()
    with torch.no_grad():
        qn = copy.deepcopy(target).double().q_network(xn.double())
    q = n64.q_network(x.double())
    td = r.double() + GAMMA * qn.max(1, keepdim=True).values * (1 - d.double())
    torch.nn.functional.mse_loss(td, q.gather(1, a)).backward()
    ref.update(q=_np(q), q_next=_np(qn), grads=_grads(n64))
    return Setup(c, B, net, x, (target, xn, a, r, d), ref)


# ---- the checkers ----------------------------------------------------------------------------------
def ratio(got, exp, rtol, atol, what):
    """assert_allclose's criterion |got - exp| <= atol + rtol |exp| as the worst ratio of the two
    sides; asserts it is <= 1 (a NaN, an unwritten output, is a failure)."""
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    assert got.shape == exp.shape, f"{what}: shape {got.shape} != {exp.shape}"
    err = np.abs(got - exp) / (atol + rtol * np.abs(exp))
    bad = ~(err <= 1.0)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} values outside rtol {rtol:g} atol {atol:.3g}; "
                           f"first at {np.argwhere(bad)[0].tolist()}: got {got[bad][0]!r}, expected {exp[bad][0]!r}")
    return float(err.max())


def near(got, exp, what):
    """tests/test_gpu_fused.near: the inference forward's tolerance."""
    return ratio(got, exp, 1e-4, 2e-5 + 4e-6 * float(np.abs(exp).max()), what)


def near_train(got, exp, what, rtol=1e-4, rel_floor=4e-6):
    """tests/test_gpu_fused_train._check: the training forward's tolerance (gradients: 1e-3, 1e-4)."""
    return ratio(got, exp, rtol, rel_floor * float(np.abs(exp).max()) + 1e-12, what)


def check_grads(got, exp, what):
    assert sorted(got) == sorted(exp), f"{what}: gradients of {sorted(got)} != {sorted(exp)}"
    return max(near_train(got[n], exp[n], f"{what} grad {n}", 1e-3, 1e-4) for n in exp)


def check_infer(s, got):
    """got: logits (B, R) and, with a critic, value (B,)."""
    what = case_id(s.case)
    m = {"logits": near(got["logits"], s.ref["logits"], what + " logits")}
    if s.case.heads == "ac":
        m["value"] = near(got["value"], s.ref["value"], what + " value")
    return m


def check_train(s, got):
    """got: logits, value (with a critic), grads {parameter name: array}."""
    what = case_id(s.case)
    m = {"logits": near_train(got["logits"], s.ref["logits"], what + " logits")}
    if s.case.heads == "ac":
        m["value"] = near_train(got["value"], s.ref["value"], what + " value")
    m["grads"] = check_grads(got["grads"], s.ref["grads"], what)
    return m


def check_pair(s, got):
    """got: q (the trained network's training forward), q_next (the target's inference forward),
    grads after the DQN loss head."""
    what = case_id(s.case)
    return {"q": near_train(got["q"], s.ref["q"], what + " q"),
            "q_next": near(got["q_next"], s.ref["q_next"], what + " q_next"),
            "grads": check_grads(got["grads"], s.ref["grads"], what)}


def check_actions(s, masks, act, q_out, what):
    """The greedy action of every set against the float64 Q values (dqn_ref's rules) and against
    the kernel's own q_out.  masks: (B, R) bool array or None; returns dict(q=..., shortfall
    / tol, disagreements, decisions)."""
    B, R, Q = s.B, s.case.R, s.ref["q"]
    act = np.asarray(act).astype(np.int64)
    mask = np.ones((B, R), bool) if masks is None else np.asarray(masks).astype(bool)
    assert act.shape == (B,) and ((act >= 0) & (act < R)).all(), f"{what}: action out of range"
    env = np.arange(B)
    some_valid = mask.any(1)
    ok = np.where(some_valid, mask[env, act], act == 0)
    assert ok.all(), f"{what}: masked action taken by sets {np.flatnonzero(~ok)[:8]}"
    dup = (dqn_ref.same_rows(s.x.numpy(), act) & (np.arange(R)[None] < act[:, None]) & mask).any(1) & some_valid
    assert not dup.any(), f"{what}: sets {np.flatnonzero(dup)[:8]} took a later one of identical rows"
    Qm = np.where(mask, Q, dqn_ref.HUGE_NEG)
    tol = dqn_ref.action_tol(float(np.abs(Q).max()))
    short = Qm.max(1) - Qm[env, act]
    worst = int(short.argmax())
    assert short[worst] <= tol, (f"{what}: set {worst} took action {act[worst]} with Q64 {short[worst]:.3e} below "
                                 f"the maximum (tol {tol:.3e})")
    disagree = int((act != Qm.argmax(1)).sum())
    assert disagree <= dqn_ref.MAX_DISAGREE_SHARE * B, f"{what}: {disagree} of {B} actions are not the float64 argmax"
    m = dict(shortfall=float(short[worst]) / tol, disagreements=disagree, decisions=B)
    if q_out is not None:
        q_out = np.asarray(q_out)
        m["q"] = near(q_out, Q, what + " q_out")
        own = np.where(mask, q_out, np.float32(dqn_ref.HUGE_NEG)).argmax(1)
        same = own == act
        assert same.all(), (f"{what}: sets {np.flatnonzero(~same)[:8]}: action {act[~same][:8]} is not the first "
                            f"argmax {own[~same][:8]} of the kernel's own q_out")
    return m
