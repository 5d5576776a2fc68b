"""The learners' train step -- loss.backward, gradient all_reduce, optimizer step -- and its
capture as replayable HIP graphs (PPO's minibatch step, DQN's train step and train periods).

With several ranks the gradients travel in ONE flat bucket: packed after the backward,
summed by one all_reduce, averaged and copied back before the optimizer step.  A captured
step is then two graphs around the all_reduce, which stays eager on the same stream (so any
backend works); on one rank it is one graph.

A capture is preceded by throw-away steps (gradients, Adam state and workspaces get allocated
outside the graph's pool) and these are undone: the parameters and the optimizer state get
their values from before back, and state the steps created (a fresh optimizer) is zeroed --
step 0, zero moments.  A graphed run so trains exactly as an eager one, wherever in a run the
capture happens.
"""
import contextlib

import torch

from . import dist as lbdist
from . import fused_train


class TrainStep:
    def __init__(self, module, optimizer, device, hook=None, bucket=None):
        """hook: called between the averaged gradients and optimizer.step() (PPO's clip_grad_norm).
        bucket: the flat gradient bucket on or off (default: on with several ranks)."""
        self.params = list(module.parameters())
        self.optimizer, self.device, self.hook = optimizer, torch.device(device), hook
        self.multi = lbdist.is_multi() if bucket is None else bool(bucket)
        self.world = torch.distributed.get_world_size() if lbdist.is_multi() else 1
        self.gflat = torch.zeros(sum(p.numel() for p in self.params), device=self.device) if self.multi else None
        self._seed = None

    def pack(self):
        if self.multi:
            torch.cat([p.grad.reshape(-1) for p in self.params], out=self.gflat)

    def allreduce(self):
        if self.multi:
            lbdist.all_reduce_sum(self.gflat)

    def unpack(self):
        if self.multi:
            self.gflat /= self.world
            off = 0
            for p in self.params:
                n = p.numel()
                p.grad.copy_(self.gflat[off:off + n].view_as(p))
                off += n

    def backward(self, loss):
        """The gradients of `loss`; with several ranks they end packed in the bucket."""
        # (also inside a captured step: autograd then allocates the gradients from the graph's
        # pool, at the same addresses every replay, and no zero fill + accumulate per parameter
        # is recorded)
        self.optimizer.zero_grad(set_to_none=True)
        # (a fixed unit seed: loss.backward() fills a new one each step, and the fused loss
        # heads return their saved gradients as they are when they see this one)
        if self._seed is None or self._seed.device != loss.device or self._seed.dtype != loss.dtype:
            self._seed = fused_train.unit_seed(loss.device, loss.dtype)
        loss.backward(self._seed)
        self.pack()

    def apply(self):
        """Averaged gradients (several ranks) -> hook -> optimizer step."""
        self.unpack()
        if self.hook is not None:
            self.hook()
        self.optimizer.step()

    def _warm(self, body, n):
        """n throw-away steps (body() = loss and self.backward) on a side stream; returns what
        _undo needs."""
        snap = ([p.detach().clone() for p in self.params],
                {p: {k: v.detach().clone() for k, v in st.items() if isinstance(v, torch.Tensor)}
                 for p, st in self.optimizer.state.items()})
        side = None
        if self.device.type == "cuda":
            side = torch.cuda.Stream(self.device)
            side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
            for _ in range(n):
                body()
                self.allreduce()
                self.apply()
        if side is not None:
            torch.cuda.current_stream(self.device).wait_stream(side)
        return snap

    def _undo(self, snap):
        with torch.no_grad():
            for p, q in zip(self.params, snap[0]):
                p.copy_(q)
            for p, st in self.optimizer.state.items():
                old = snap[1].get(p, {})
                for k, v in st.items():
                    if isinstance(v, torch.Tensor):
                        if k in old:
                            v.copy_(old[k])
                        else:
                            v.zero_()

    def warmup(self, body, n=2):
        """n throw-away steps, undone: what a caller that captures its own graphs runs first."""
        self._undo(self._warm(body, n))

    def capture(self, body, n=2):
        """Capture body() + the optimizer step after n throw-away steps (undone) -> (graphs for
        replay(), body's result): one graph on one rank, two around the all_reduce on several."""
        snap = self._warm(body, n)
        ga = torch.cuda.CUDAGraph()
        with torch.cuda.graph(ga):
            out = body()
            if not self.multi:
                self.apply()
        graphs = (ga,)
        if self.multi:
            gb = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gb):
                self.apply()
            graphs = (ga, gb)
        self._undo(snap)
        return graphs, out

    def replay(self, graphs):
        graphs[0].replay()
        if len(graphs) > 1:
            self.allreduce()  # eager collective on the current stream, between the two graphs
            graphs[1].replay()
