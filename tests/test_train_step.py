"""lbk8s.train_step.TrainStep on the CPU (a tiny nn.Linear, Adam(eps=1e-5); no GPU, no native
library): the warm-up's undo, the flat gradient bucket's round trip and the hook's place."""
import pytest
import torch
from torch import nn, optim

from lbk8s.train_step import TrainStep


def _setup(steps_before, seed=0, **kw):
    """(net, optimizer, TrainStep, body) after `steps_before` real steps on fixed data."""
    torch.manual_seed(seed)
    net = nn.Linear(5, 3)
    opt = optim.Adam(net.parameters(), lr=1e-2, eps=1e-5)
    x, y = torch.randn(16, 5), torch.randn(16, 3)
    ts = TrainStep(net, opt, "cpu", **kw)

    def body():
        loss = ((net(x) - y) ** 2).mean()
        ts.backward(loss)
        return loss

    for _ in range(steps_before):
        body()
        ts.apply()
    return net, opt, ts, body


def _state(net, opt):
    params = [p.detach().clone() for p in net.parameters()]
    adam = [{k: v.detach().clone() for k, v in opt.state[p].items() if isinstance(v, torch.Tensor)}
            for p in net.parameters() if p in opt.state]
    return params, adam


def _zeroing_undo(ts, snap):
    """The rule TrainStep replaced: parameters restored, every Adam state tensor zeroed."""
    with torch.no_grad():
        for p, q in zip(ts.params, snap[0]):
            p.copy_(q)
        for st in ts.optimizer.state.values():
            for v in st.values():
                if isinstance(v, torch.Tensor):
                    v.zero_()


@pytest.mark.parametrize("steps_before", [0, 3])
def test_warmup_is_undone(steps_before):
    """A 2-step warm-up leaves the parameters and every Adam state tensor as they were (a fresh
    optimizer: step 0 and zero moments), and the next real step is the untouched twin's, bit for
    bit.  Zeroing the Adam state instead does so only for a fresh optimizer."""
    net, opt, ts, body = _setup(steps_before)
    twin_net, twin_opt, twin_ts, twin_body = _setup(steps_before)
    params, adam = _state(net, opt)
    assert len(adam) == (2 if steps_before else 0)
    ts.warmup(body, n=2)
    after_params, after_adam = _state(net, opt)
    assert len(after_adam) == 2
    for a, b in zip(after_params, params):
        assert torch.equal(a, b)
    for i, st in enumerate(after_adam):
        assert set(st) >= {"step", "exp_avg", "exp_avg_sq"}
        for k, v in st.items():
            assert torch.equal(v, adam[i][k] if adam else torch.zeros_like(v)), k
    for b, t in ((body, ts), (twin_body, twin_ts)):
        b()
        t.apply()
    for a, b in zip(net.parameters(), twin_net.parameters()):
        assert torch.equal(a, b)
    for p, q in zip(net.parameters(), twin_net.parameters()):
        for k, v in opt.state[p].items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(twin_opt.state[q][k])), k

    # the zeroing stand-in, on a third copy
    znet, zopt, zts, zbody = _setup(steps_before)
    _zeroing_undo(zts, zts._warm(zbody, 2))
    zbody()
    zts.apply()
    same = all(torch.equal(a, b) for a, b in zip(znet.parameters(), twin_net.parameters()))
    assert same == (steps_before == 0)


def test_bucket_round_trip():
    """Bucket forced on at world size 1: pack, average, unpack leaves every gradient bit-equal,
    and the bucket holds the gradients flattened in parameters() order."""
    torch.manual_seed(1)
    net = nn.Sequential(nn.Linear(5, 3), nn.Linear(3, 7, bias=False), nn.Linear(7, 1))
    opt = optim.Adam(net.parameters(), eps=1e-5)
    ts = TrainStep(net, opt, "cpu", bucket=True)
    assert ts.multi and ts.world == 1
    shapes = [tuple(p.shape) for p in net.parameters()]
    assert shapes == [(3, 5), (3,), (7, 3), (1, 7), (1,)]
    assert ts.gflat.shape == (sum(p.numel() for p in net.parameters()),)
    ts.backward(net(torch.randn(4, 5)).sum())  # (packs)
    grads = [p.grad.detach().clone() for p in net.parameters()]
    assert torch.equal(ts.gflat, torch.cat([g.reshape(-1) for g in grads]))
    off = 0
    for p, g in zip(net.parameters(), grads):  # (the offsets, parameter by parameter)
        assert torch.equal(ts.gflat[off:off + p.numel()].view_as(p), g)
        off += p.numel()
    for p in net.parameters():  # (unpack must write every gradient from the bucket)
        p.grad.fill_(float("nan"))
    ts.allreduce()
    ts.unpack()
    for p, g in zip(net.parameters(), grads):
        assert torch.equal(p.grad, g)
    assert TrainStep(net, opt, "cpu").gflat is None  # (one process: no bucket)


@pytest.mark.parametrize("bucket", [False, True])
def test_hook_runs_between_unpack_and_optimizer_step(bucket):
    """apply(): unpack, then the hook, then optimizer.step() -- the hook sees the gradients out of
    the bucket and the step takes what the hook left."""
    calls = []

    def hook():
        calls.append(("hook", [p.grad.detach().clone() for p in net.parameters()],
                      [p.detach().clone() for p in net.parameters()]))
        for p in net.parameters():
            p.grad.mul_(0.25)

    net, opt, ts, body = _setup(0, hook=hook, bucket=bucket)
    twin_net, twin_opt, twin_ts, twin_body = _setup(0)
    before = [p.detach().clone() for p in net.parameters()]
    body()
    grads = [p.grad.detach().clone() for p in net.parameters()]
    if bucket:  # (what the hook must see comes out of the bucket)
        for p in net.parameters():
            p.grad.zero_()
    step = opt.step
    opt.step = lambda *a, **k: (calls.append(("step", [p.grad.detach().clone() for p in net.parameters()])),
                                step(*a, **k))[1]
    ts.apply()
    assert [c[0] for c in calls] == ["hook", "step"]
    for seen, g, p_seen, p0 in zip(calls[0][1], grads, calls[0][2], before):
        assert torch.equal(seen, g) and torch.equal(p_seen, p0)  # unpacked already, not yet stepped
    for seen, g in zip(calls[1][1], grads):
        assert torch.equal(seen, g * 0.25)
    # the twin steps on the rescaled gradients: the same parameters
    twin_body()
    for p in twin_net.parameters():
        p.grad.mul_(0.25)
    twin_opt.step()
    for a, b in zip(net.parameters(), twin_net.parameters()):
        assert torch.equal(a, b)
