"""Every variant of the fused deep-sets forward with more than one set per wave, against float64.

k_deepsets_fwd<TS, P, MODE, XR> and k_ds_fwd_pair<1, P> (csrc/lbk8s_deepsets.h) carry P = 4 or 2
sets per wave only when the batch fills the chip (ceil(B / P) >= 4 x CUs), so the per-R sweeps of
test_gpu_fused.py / test_gpu_fused_train.py (B = 300, 257, 1001) run P = 1.  The cases here
(tests/ds_ref.py) take their batch sizes from the device's CU count, assert through
fused.forward_kernel (lb_ds_forward_kernel, host only) that the launch takes the variant the
case's id names, and compare with the float64 reference of the project's own torch modules under
the project's own tolerances; tests/test_ds_ref_harness.py runs the same cases and checkers on a
float32 CPU stand-in and on broken ones.  Every output buffer starts as NaN (actions: -1), so a
row the kernel leaves unwritten fails.

Measured on an MI355X (256 CUs), worst |error| / tolerance per family: see DESIGN.md, "Forward
variants against float64".
"""
import contextlib
import copy

import pytest
import torch

import ds_ref
from ds_ref import ARGMAX_CASES, INFER_CASES, PAIR_CASES, TRAIN_CASES, case_id

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def nan_outputs():
    """torch.empty hands out NaN (floats) or -1 (integers) instead of whatever the allocator
    holds: the wrappers allocate their outputs with it, and a value a kernel does not write
    must not pass for one it wrote."""
    real = torch.empty

    def poisoned(*args, **kw):
        t = real(*args, **kw)
        if t.is_floating_point():
            t.fill_(float("nan"))
        elif t.dtype != torch.bool:
            t.fill_(-1)
        return t

    torch.empty = poisoned
    try:
        yield
    finally:
        torch.empty = real


def on_device(s):
    """The case's network (a copy: the cached one stays on the CPU) and inputs on the GPU; the
    launch must take the variant the case names."""
    from lbk8s import fused
    c = s.case
    assert fused.forward_kernel(ds_ref.WHICH[c.family], s.B, c.R) == c.variant, case_id(c)
    return copy.deepcopy(s.net).cuda(), s.x.cuda()


def grads_of(net):
    out = {}
    for n, p in net.named_parameters():
        assert p.grad is not None, n
        out[n] = p.grad.cpu().numpy()
    return out


@pytest.mark.parametrize("c", INFER_CASES, ids=case_id)
def test_inference_forward(c):
    """MODE 0: deepsets_forward (actor + critic) and q_forward (actor only)."""
    from lbk8s import fused
    s = ds_ref.setup(c)
    net, x = on_device(s)
    with nan_outputs():
        if c.heads == "ac":
            logits, value = fused.deepsets_forward(net, x, require=True)
            got = {"logits": logits.cpu().numpy(), "value": value.cpu().numpy()}
        else:
            got = {"logits": fused.q_forward(net, x, require=True).cpu().numpy()}
    print("ds-margin", case_id(c), ds_ref.check_infer(s, got))


@pytest.mark.parametrize("c", TRAIN_CASES, ids=case_id)
def test_training_forward_and_backward(c):
    """MODE 1: fused_train.actor_critic / actor_only; logits, value and every parameter gradient
    of a fixed random linear functional against float64 autograd."""
    from lbk8s import fused_train
    s = ds_ref.setup(c)
    net, x = on_device(s)
    wl, wv = (t.cuda() for t in s.extra)
    with nan_outputs():
        if c.heads == "ac":
            logits, value = fused_train.actor_critic(net, x)
            got = {"logits": logits.detach().cpu().numpy(), "value": value.detach().cpu().numpy()}
            ((logits * wl).sum() + (value * wv).sum()).backward()
        else:
            logits = fused_train.actor_only(net, net.q_network.net, x)
            got = {"logits": logits.detach().cpu().numpy()}
            (logits * wl).sum().backward()
        got["grads"] = grads_of(net)
    print("ds-margin", case_id(c), ds_ref.check_train(s, got))


@pytest.mark.parametrize("c", ARGMAX_CASES, ids=case_id)
def test_greedy_action(c):
    """MODE 2: q_argmax_graphable with masks (the batch's last set, alone in its group at B2, in
    turn: equal rows, nothing valid, only row R - 1 valid) and without."""
    from lbk8s import fused
    s = ds_ref.setup(c)
    net, x = on_device(s)
    B, R = s.B, c.R
    frag = fused.frag_buffer("cuda")
    out = {}
    for last in ds_ref.LAST_SETS + (None, "no q_out"):
        masks = ds_ref.argmax_masks(B, R, ds_ref.seed_of(c), last) if last in ds_ref.LAST_SETS else None
        act = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        qv = None if last == "no q_out" else torch.full((B, R), float("nan"), device="cuda")
        fused.q_argmax_graphable(net, x, None if masks is None else masks.cuda(), act, frag, q_out=qv)
        a = act.cpu().numpy()
        out[last] = ds_ref.check_actions(s, None if masks is None else masks.numpy(), a,
                                         None if qv is None else qv.cpu().numpy(), f"{case_id(c)} last={last}")
        if masks is not None:
            assert a[5] == 0 and a[7] == 0 and a[9] == R - 1, a[[5, 7, 9]]
            assert a[B - 1] == (R - 1 if last == "only_last" else 0), (last, a[B - 1])
        else:
            assert a[5] == 0 and a[B - 1] == 0
    print("ds-margin", case_id(c), out)


@pytest.mark.parametrize("c", PAIR_CASES, ids=case_id)
def test_paired_forward(c):
    """k_ds_fwd_pair<1, P>: q_train_with_target's Q(next_obs) of the target and Q(obs) of the
    trained network against float64, the gradients after dqn_head against float64 autograd,
    and everything bit for bit against the two forwards launched apart."""
    from lbk8s import fused, fused_train
    s = ds_ref.setup(c)
    net, x = on_device(s)
    P = c.variant[1]
    assert fused.forward_kernel(fused.FWD, s.B, c.R) == fused.forward_kernel(fused.FWD_TRAIN, s.B, c.R) == (1, P, 0)
    target, xn, a, r, d = s.extra
    target = copy.deepcopy(target).cuda()
    xn, a, r, d = xn.cuda(), a.cuda(), r.cuda(), d.cuda()
    runs = []
    for paired in (True, False):
        net.zero_grad(set_to_none=True)
        with nan_outputs():
            if paired:
                q, q_next = fused_train.q_train_with_target(net, net.q_network.net, x, target, xn)
            else:
                q_next = fused.q_forward(target, xn, require=True)
                q = fused_train.actor_only(net, net.q_network.net, x)
            loss, _, _ = fused_train.dqn_head(q, q_next, a, r, d, ds_ref.GAMMA)
            loss.backward(fused_train.unit_seed(loss.device))
        runs.append({"q": q.detach().cpu().numpy(), "q_next": q_next.cpu().numpy(), "grads": grads_of(net)})
    print("ds-margin", case_id(c), ds_ref.check_pair(s, runs[0]))
    assert (runs[0]["q"] == runs[1]["q"]).all() and (runs[0]["q_next"] == runs[1]["q_next"]).all()
    for n, g in runs[0]["grads"].items():
        assert (g == runs[1]["grads"][n]).all(), n
