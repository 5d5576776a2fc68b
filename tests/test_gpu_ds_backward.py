"""lb_ds_train_backward, lb_ds_train_backward_sets, lb_ds_set_grads, lb_ds_over_sets and the pack
kernels pinned to the float64 model of tests/ds_bwd_ref.py (tests/test_ds_bwd_ref_harness.py shows
on the CPU that the model equals float64 autograd to 1e-10, that the runners accept a float32
stand-in of the kernels' formulas on every case here, and that they refuse thirteen broken ones).

The kernels are called through the C ABI (_native.lib()), where the Python wrappers hide a path:
dlogits NULL (critic only), a head not asked for, a workspace that is not zero, the set sums on
buffers no training step produces.  Every output arrives filled with NaN with 64 guard floats past
its end; the backward's workspace is NaN over all LB_DS_WORKSPACE_FLOATS (1e30 in one test) with
a guard of its own; every call is made twice and must repeat bit for bit.

Cases (ds_bwd_ref.PLANTED_CASES, MANY_CASES, REAL_CASES, SG_CASES, OS_CASES):
  * planted backward, no forward launch: R over every count of live 4-row groups in the last tile,
    the one-row last tile at 1, 2, 5 and 17 tiles, full last tiles; B = 1, 2, 7, 8, 9 (fewer sets
    than a block has waves; B = 1 shows one set's dLambda2 / dLambda1); both heads, actor only,
    critic only; maxima planted on rows 0, R - 1, the last tile's first row, 15 / 16, 255 / 256;
  * 1 .. 4 sets per wave (B = 2,047 .. 6,150) at R = 1, 9, 17 and, B = 2,049 / 4,097, at 33 and 65;
  * end to end on the float64 network's inputs: pack pair, training forward (its setvec exactly
    consistent with its own saved activations), backward, lb_ds_set_grads, and
    lb_ds_train_backward_sets bit-equal to the two calls, R up to 257 with the critic;
  * lb_ds_set_grads: one chunk, the chunk edges, nine chunks; every residue of the row sum;
  * lb_ds_over_sets: set counts around the prefetch depth, one span and eight spans; 1, 4, 5 and
    16 jobs; all of {1, 8, 16, 17, 20, 63, 64}^2; a NULL, aligned, offset and odd-stride operands;
  * the refusals, which must leave every output as it was.
The backward's tolerances needed no measured allowance (per-set GS1 included); the worst shares of
the allowances seen on the MI355X, beside the CPU stand-in's, are in DESIGN.md section 2.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import ds_bwd_ref as br

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _up(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


class HipDevice:
    def __init__(self):
        from lbk8s import _native, fused
        self.native, self.fused, self.L = _native, fused, _native.lib()
        self._net = self._img = None

    def _call(self, rc):
        self.native.check(rc)
        torch.cuda.synchronize()

    def weights(self, net):
        """(struct lb_ds_weights of a device copy of net, the tensors it points to)."""
        import copy
        dn = copy.deepcopy(net).cuda()
        if hasattr(dn, "actor"):
            return self.fused._weights_struct(dn.actor.net, dn.critic)
        return self.fused._weights_struct(dn.q_network.net, None)

    def images(self, net):
        """lb_ds_pack_pair's two images of net (packed once per network)."""
        if self._net is not net:
            w, keep = self.weights(net)
            frag = torch.full((self.native.LB_DS_FRAG_FLOATS,), NAN, device="cuda")
            bfrag = torch.full((self.native.LB_DS_BWD_FLOATS,), NAN, device="cuda")
            self._call(self.L.lb_ds_pack_pair(C.byref(w), frag.data_ptr(), bfrag.data_ptr(), None))
            self._net, self._img = net, (frag, bfrag)
        return self._img

    def forward(self, net, heads, x):
        frag, _ = self.images(net)
        B, R, _ = x.shape
        xs = _up(x)
        new = lambda *s: torch.full(s, NAN, device="cuda")
        logits, save_a = (new(B, R), new(2, B, R, 64)) if "a" in heads else (None, None)
        mean, save_c = (new(B, 64), new(2, B, R, 64)) if "c" in heads else (None, None)
        sv = _up(br.nan_buf(B * br.SV))
        self._call(self.L.lb_ds_train_forward(frag.data_ptr(), xs.data_ptr(), B, R, _ptr(logits), _ptr(mean),
                                              _ptr(save_a), _ptr(save_c), sv.data_ptr(), None))
        out = {"setvec": sv.cpu().numpy()}
        if save_a is not None:
            out["save_a"] = save_a.cpu().numpy()
        if save_c is not None:
            out["save_c"] = save_c.cpu().numpy()
        return out

    def backward(self, net, heads, x, save_a, save_c, dlogits, dmean, wgrad, setvec, ws_fill, set_grads):
        _, bfrag = self.images(net)
        B, R, _ = x.shape
        assert setvec.size == B * br.SV + br.GUARD and wgrad.size == 2 * br.WG + br.GUARD
        assert save_a is None or save_a.shape == (2, B, R, 64)
        assert save_c is None or save_c.shape == (2, B, R, 64)
        assert dlogits is None or dlogits.shape == (B, R)
        assert dmean is None or dmean.shape == (B, 64)
        xs, sa, sc, dl, dm, wg, sv, sg = (_up(a) for a in (x, save_a, save_c, dlogits, dmean, wgrad, setvec, set_grads))
        work = torch.full((br.WS_FLOATS + br.GUARD,), float(ws_fill), device="cuda")
        work[br.WS_FLOATS:] = NAN
        args = (bfrag.data_ptr(), xs.data_ptr(), B, R, _ptr(sa), _ptr(sc), _ptr(dl), _ptr(dm), wg.data_ptr(),
                work.data_ptr(), sv.data_ptr())
        if sg is None:
            self._call(self.L.lb_ds_train_backward(*args, None))
        else:
            self._call(self.L.lb_ds_train_backward_sets(*args, sg.data_ptr(), None))
        out = dict(wgrad=wg.cpu().numpy(), setvec=sv.cpu().numpy(), ws_guard=work[br.WS_FLOATS:].cpu().numpy())
        if sg is not None:
            out["set_grads"] = sg.cpu().numpy()
        return out

    def set_grads(self, setvec, dlogits, dmean, S, R, out):
        assert setvec.shape == (S, br.SV) and dlogits.shape == (S, R) and (dmean is None or dmean.shape == (S, 64))
        assert out.size == br.SG_ACTOR + (br.SG_CRITIC if dmean is not None else 0) + br.GUARD
        sv, dl, dm, o = (_up(a) for a in (setvec, dlogits, dmean, out))
        self._call(self.L.lb_ds_set_grads(sv.data_ptr(), dl.data_ptr(), _ptr(dm), S, R, o.data_ptr(), None))
        return o.cpu().numpy()

    def set_jobs(self, dbufs, jobs, o):
        arr, off = [], 0
        for ia, fa, ib, fb, M, N, scale in jobs:
            a = None if ia is None else dbufs[ia].data_ptr() + 4 * fa[0]
            arr.append(self.native.LBSetJobC(a, 0 if ia is None else fa[1], dbufs[ib].data_ptr() + 4 * fb[0], fb[1], M, N,
                                             float(scale), o.data_ptr() + 4 * off))
            off += M * N
        return (self.native.LBSetJobC * max(len(arr), 1))(*arr)

    def over_sets(self, bufs, jobs, S, out, work):
        dbufs = [_up(b) for b in bufs]
        for ia, fa, ib, fb, M, N, _ in jobs:   # every operand as large as the header says
            assert bufs[ib].size >= fb[0] + (S - 1) * fb[1] + N
            assert ia is None or bufs[ia].size >= fa[0] + (S - 1) * fa[1] + M
        o, w = _up(out), _up(work)
        self._call(self.L.lb_ds_over_sets(self.set_jobs(dbufs, jobs, o), len(jobs), S, w.data_ptr(),
                                          work.size - br.GUARD, None))
        return o.cpu().numpy(), w.cpu().numpy()


@pytest.fixture(scope="module")
def dev():
    return HipDevice()


def _fmt(shares):
    return f"worst {max(shares.values()):.3f} | " + " ".join(f"{k}={v:.3f}" for k, v in shares.items())


@pytest.mark.parametrize("c", br.PLANTED_CASES, ids=br.case_id)
def test_backward_planted(dev, c):
    shares, _ = br.run_backward(dev, c)
    print(f"bwd {br.case_id(c)}: {_fmt(shares)}")


@pytest.mark.parametrize("c", br.MANY_CASES, ids=br.case_id)
def test_backward_many_sets_per_wave(dev, c):
    shares, _ = br.run_backward(dev, c)
    print(f"bwd {br.case_id(c)}: {_fmt(shares)}")


@pytest.mark.parametrize("c", [br.Case("planted", "ac", 17, 9), br.Case("planted", "ac", 9, 2049)], ids=br.case_id)
def test_backward_ignores_what_the_workspace_held(dev, c):
    _, a = br.run_backward(dev, c, repeat=False)
    _, b = br.run_backward(dev, c, ws_fill=1e30, repeat=False)
    for k in ("wgrad", "setvec"):
        br.same_bits(a[k], b[k], f"{br.case_id(c)} {k}, workspace 1e30 against NaN")


@pytest.mark.parametrize("c", br.REAL_CASES, ids=br.case_id)
def test_train_step_end_to_end(dev, c):
    shares = br.run_real(dev, c)
    print(f"real {br.case_id(c)}: {_fmt(shares)}")


@pytest.mark.parametrize("spec", br.SG_CASES, ids=br.sg_id)
def test_set_grads_within_the_summation_bound(dev, spec):
    print(f"set_grads {br.sg_id(spec)}: worst {br.run_set_grads(dev, spec):.3f}")


@pytest.mark.parametrize("spec", br.OS_CASES, ids=lambda s: f"{s[0]}-S{s[1]}")
def test_over_sets_within_the_summation_bound(dev, spec):
    print(f"over_sets {spec[0]}-S{spec[1]}: worst {br.run_over_sets(dev, spec):.3f}")


@pytest.mark.parametrize("heads", ["ac", "a"])
def test_pack_pair_equals_the_two_packs(dev, heads):
    net = br.net_of(br.Case("real", heads, 9, 5))
    w, keep = dev.weights(net)
    nf, nb = dev.native.LB_DS_FRAG_FLOATS, dev.native.LB_DS_BWD_FLOATS
    f2, b2, f1, b1 = (_up(br.nan_buf(n)) for n in (nf, nb, nf, nb))
    dev._call(dev.L.lb_ds_pack_pair(C.byref(w), f2.data_ptr(), b2.data_ptr(), None))
    dev._call(dev.L.lb_ds_pack(C.byref(w), f1.data_ptr(), None))
    dev._call(dev.L.lb_ds_pack_backward(C.byref(w), b1.data_ptr(), None))
    f2, b2, f1, b1 = (t.cpu().numpy() for t in (f2, b2, f1, b1))
    br.body(f1, nf, "lb_ds_pack")
    br.body(f2, nf, "lb_ds_pack_pair frag_out")
    assert not np.isnan(br.body(b1, nb, "lb_ds_pack_backward")).any(), "the backward image has unwritten floats"
    br.body(b2, nb, "lb_ds_pack_pair bwd_frag_out")
    br.same_bits(f2, f1, "lb_ds_pack_pair's forward image against lb_ds_pack")
    br.same_bits(b2, b1, "lb_ds_pack_pair's backward image against lb_ds_pack_backward")


# ---- refusals: decided on the host, before any launch -----------------------------------------------
class _Refusal:
    """Valid device buffers of a small call, NaN-filled outputs; refused(rc, reason) checks the return
    code, lb_last_error and that no output changed."""

    def __init__(self, dev, B=4, R=9):
        self.dev, self.B, self.R = dev, B, R
        z = lambda *s: torch.zeros(s, device="cuda")
        self.bfrag, self.x, self.save, self.dl, self.dm = z(dev.native.LB_DS_BWD_FLOATS), z(B, R, 8), z(2, B, R, 64), z(B, R), z(B, 64)
        self.outs = {k: torch.full((n,), NAN, device="cuda") for k, n in
                     (("wgrad", 2 * br.WG), ("work", br.WS_FLOATS), ("setvec", B * br.SV),
                      ("sg", br.SG_ACTOR + br.SG_CRITIC), ("os_out", 64 * 64), ("os_work", 64 * 64))}

    def backward_args(self, **kw):
        a = dict(bfrag=self.bfrag.data_ptr(), x=self.x.data_ptr(), B=self.B, R=self.R, sa=self.save.data_ptr(),
                 sc=self.save.data_ptr(), dl=self.dl.data_ptr(), dm=self.dm.data_ptr(), wg=self.outs["wgrad"].data_ptr(),
                 work=self.outs["work"].data_ptr(), sv=self.outs["setvec"].data_ptr())
        a.update(kw)
        return list(a.values())

    def refused(self, rc, reason):
        torch.cuda.synchronize()
        msg = self.dev.L.lb_last_error().decode()
        assert rc < 0 and reason in msg, f"rc {rc}, lb_last_error {msg!r}: expected a refusal naming {reason!r}"
        for k, t in self.outs.items():
            assert bool(torch.isnan(t).all()), f"a refused call wrote to {k}"


@pytest.fixture(scope="module")
def ref(dev):
    return _Refusal(dev)


@pytest.mark.parametrize("kw,reason", [(dict(R=0), "num_elements must be in [1, 257]"),
                                       (dict(R=258), "num_elements must be in [1, 257]"),
                                       (dict(B=0), "num_envs < 1"),
                                       (dict(sa=None), "activation buffer is NULL"),
                                       (dict(dm=None, sc=None, sa=None), "activation buffer is NULL")],
                         ids=["R0", "R258", "B0", "dlogits-without-save_actor", "actor-only-without-save_actor"])
def test_backward_refusals(ref, kw, reason):
    ref.refused(ref.dev.L.lb_ds_train_backward(*ref.backward_args(**kw), None), reason)
    ref.refused(ref.dev.L.lb_ds_train_backward_sets(*ref.backward_args(**kw), ref.outs["sg"].data_ptr(), None), reason)


def test_backward_sets_refusals(ref):
    L, sg = ref.dev.L, ref.outs["sg"].data_ptr()
    ref.refused(L.lb_ds_train_backward_sets(*ref.backward_args(dl=None), sg, None), "set_grads_out and dlogits are required")
    ref.refused(L.lb_ds_train_backward_sets(*ref.backward_args(), None, None), "set_grads_out and dlogits are required")


def test_set_grads_refusals(ref):
    L, o = ref.dev.L, ref.outs
    sv, dl, dm, sg = o["setvec"].data_ptr(), ref.dl.data_ptr(), ref.dm.data_ptr(), o["sg"].data_ptr()
    ref.refused(L.lb_ds_set_grads(sv, dl, dm, 0, ref.R, sg, None), "num_sets < 1")
    ref.refused(L.lb_ds_set_grads(sv, None, dm, ref.B, ref.R, sg, None), "setvec/dlogits/out NULL")
    ref.refused(L.lb_ds_set_grads(sv, dl, dm, ref.B, 0, sg, None), "num_elements must be in [1, 257]")
    ref.refused(L.lb_ds_set_grads(sv, dl, dm, ref.B, 258, sg, None), "num_elements must be in [1, 257]")


def test_over_sets_refusals(ref):
    dev, L = ref.dev, ref.dev.L
    S = 4
    a = torch.zeros(S * 68, device="cuda")
    out, work = ref.outs["os_out"], ref.outs["os_work"]
    job = lambda M, N, null_a=False: (None if null_a else 0, (0, 68), 0, (0, 68), M, N, 1.0)
    call = lambda jobs, n, floats: L.lb_ds_over_sets(dev.set_jobs([a], jobs, out), n, S, work.data_ptr(), floats, None)
    ref.refused(call([job(8, 8)], 0, 4096), "num_jobs not in [1, 16]")
    ref.refused(call([job(2, 2)] * 17, 17, 4096), "num_jobs not in [1, 16]")
    ref.refused(call([job(65, 8)], 1, 4096), "1 <= M, N <= 64")
    ref.refused(call([job(8, 65)], 1, 4096), "1 <= M, N <= 64")
    ref.refused(call([job(2, 8, null_a=True)], 1, 4096), "M == 1 when a is NULL")
    ref.refused(call([job(8, 8), job(64, 60)], 2, 8 * 8 + 64 * 60 - 1), "workspace too small")
