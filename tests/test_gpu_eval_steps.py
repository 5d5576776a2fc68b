"""lb_eval_steps (csrc/lbk8s_eval.h): a greedy evaluation's vector steps in ONE launch == steps x
(lb_ds_q_argmax, lb_step, lb_ppo_record), bit for bit, through the C ABI.  The yardstick is the
three existing launches, each pinned to its own reference (tests/test_gpu_fused.py,
tests/test_gpu_parity.py, tests/test_gpu_ppo_tail.py).

Per case two envs are built from the same seed and brought out of phase (one random step, then a
reset of the odd envs; with auto-reset off every env stays at its episode's start and the launch
plays exactly the episode), and one seeded actor-only image is packed: a DQNDeepSetAgent's Q
network or a DeepSetAgent's actor.  Every output buffer starts as NaN (integers: a sentinel) with
64 guard elements past its end: the guards must survive, everything the header says is written
must be overwritten, and an output passed as NULL leaves its buffer as it was.  Shapes: R = 1,
run.py's own (8 envs, E = 6), a ragged last group (130 = 65 groups of two), R = 16 with and
without the reject row, a batch at which lb_ds_q_argmax itself takes two envs per wave (8 CUs'
worth of SIMDs + 1) next to one where it takes one (130).  Episode length 5 with 1, 4, 5 and 13
steps: nothing ends, an episode ends on the last step, several end per env inside the launch.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import dqn_ref

pytestmark = pytest.mark.gpu

PAD = 64
W = 24  # LB_EPLOG_W
L_EP = 5
INT = {torch.float32: torch.int32, torch.float64: torch.int64}
TRACES = ("actions_all", "rewards_all", "dones_all")


def _bits(t):
    return t.view(INT[t.dtype]) if t.dtype in INT else t


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _nan(n, dtype=torch.float32):
    return torch.full((n + PAD,), float("nan"), dtype=dtype, device="cuda")


def _fill(n, value, dtype):
    return torch.full((n + PAD,), value, dtype=dtype, device="cuda")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _env(B, E, rej, L, auto=True, seed=11):
    """A reset env; with auto-reset its envs are out of phase: the even ones one step into their
    episode."""
    from lbk8s import LBVecEnv
    env = LBVecEnv(B, seed=seed, as_tensors=True, auto_reset=auto, num_endpoints=E, rejection_allowed=rej,
                   episode_length=L, reward_function="multi")
    env.reset()
    if auto and L > 1:
        env.step_device(None)
        env.reset_masked((torch.arange(B, device="cuda") % 2).to(torch.uint8))
    return env


_frags = {}


def _frag(kind):
    """One seeded agent's actor-only weight image per kind ("dqn": the Q network, "ppo": the
    actor), left unchanged."""
    from lbk8s import evaluate
    from lbk8s.deepsets import DeepSetAgent, DQNDeepSetAgent
    if kind not in _frags:
        torch.manual_seed(5)
        agent = (DQNDeepSetAgent if kind == "dqn" else DeepSetAgent)(8).cuda()
        _frags[kind] = (agent, evaluate.eval_image(agent, torch.device("cuda"))[1])
    return _frags[kind][1]


class Bufs:
    """One side's buffers of a `steps`-step sequence."""
    ALL = ("obs", "actions_all", "rewards_all", "dones_all", "actions_out", "reward_out", "done_out", "ep_stats",
           "ep_sum", "ep_cnt", "ret32", "ep_r32", "log", "count")

    def __init__(self, env, steps, cap):
        B, R = env.num_envs, env.cfg.obs_rows
        self.B, self.R, self.steps, self.cap = B, R, steps, cap
        self.n = dict(obs=B * R * 8, actions_all=steps * B, rewards_all=steps * B, dones_all=steps * B, actions_out=B,
                      reward_out=B, done_out=B, ep_stats=B * 16, ep_sum=B, ep_cnt=B, ret32=B, ep_r32=B,
                      log=max(cap, 1) * W, count=1)
        n = self.n
        self.obs = _nan(n["obs"])
        self.obs[:n["obs"]] = env.obs.reshape(-1)
        self.actions_all = _fill(n["actions_all"], -77, torch.int32)
        self.rewards_all = _nan(n["rewards_all"])
        self.dones_all = _fill(n["dones_all"], 0xAB, torch.uint8)
        self.actions_out = _fill(B, -77, torch.int32)
        self.reward_out = _nan(B)
        self.done_out = _fill(B, 0xAB, torch.uint8)
        self.ep_stats = _nan(n["ep_stats"], torch.float64)
        self.ep_sum, self.ep_cnt = _nan(B, torch.float64), _nan(B, torch.float64)
        self.ep_sum[:B] = (torch.arange(B, dtype=torch.float64) * 0.25 + 1.5).cuda()   # preloaded, non-zero
        self.ep_cnt[:B] = (torch.arange(B, dtype=torch.float64) % 3 + 1.0).cuda()
        self.ret32, self.ep_r32 = _nan(B), _nan(B)
        self.ret32[:B] = torch.randn(B, generator=torch.Generator().manual_seed(B)).cuda()
        self.log = _nan(n["log"], torch.float64)
        self.count = torch.zeros(1 + PAD, dtype=torch.int32, device="cuda")
        self.init = {k: getattr(self, k).clone() for k in self.ALL}

    def restore(self):
        for k in self.ALL:
            getattr(self, k).copy_(self.init[k])

    def guards_intact(self):
        for k in self.ALL:
            assert _same(getattr(self, k)[self.n[k]:], self.init[k][self.n[k]:]), k

    def written(self, traces=TRACES, with_log=True, with_sums=True):
        """Everything the header says is written holds a value; what was passed as NULL is as it was."""
        B, n = self.B, self.n
        assert not torch.isnan(self.obs[:n["obs"]]).any()
        assert not torch.isnan(self.reward_out[:B]).any()
        assert (self.actions_out[:B] >= 0).all() and (self.actions_out[:B] < self.R).all()
        assert (self.done_out[:B] <= 1).all()
        for k in TRACES:
            if k not in traces:
                assert _same(getattr(self, k), self.init[k]), k
        if "actions_all" in traces:
            a = self.actions_all[:n["actions_all"]]
            assert (a >= 0).all() and (a < self.R).all()
        if "rewards_all" in traces:
            assert not torch.isnan(self.rewards_all[:n["rewards_all"]]).any()
        if "dones_all" in traces:
            assert (self.dones_all[:n["dones_all"]] <= 1).all()
        if not with_log:
            for k in ("ret32", "ep_r32", "log", "count"):
                assert _same(getattr(self, k), self.init[k]), k
        else:
            assert not torch.isnan(self.ret32[:B]).any()
        if not with_sums:
            assert _same(self.ep_sum, self.init["ep_sum"]) and _same(self.ep_cnt, self.init["ep_cnt"])

    def rows(self):
        n = min(int(self.count[0].item()), self.cap)
        r = self.log[:n * W].view(n, W).cpu().numpy()
        return r[np.lexsort((r[:, 19], r[:, 20]))]


def _np_bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _log_args(b, with_log, tag0):
    if not with_log:
        return (None, None, 0, None, 0, None)
    return (_ptr(b.ret32), _ptr(b.ep_r32), tag0, _ptr(b.log), b.cap, _ptr(b.count))


def _row(buf, i, n):
    return buf.data_ptr() + buf.element_size() * i * n


def _fused(env, frag, b, masks, steps=None, step0=0, tag0=3, traces=TRACES, with_log=True, with_sums=True,
           stream=None):
    """lb_eval_steps of the steps step0 .. step0 + steps - 1 of b's sequence."""
    from lbk8s import _native
    B, R = b.B, b.R
    steps = b.steps if steps is None else steps
    tr = [_row(getattr(b, k), step0, B) if k in traces else None for k in TRACES]
    _native.check(_native.lib().lb_eval_steps(
        frag.data_ptr(), b.obs.data_ptr(), env.state.data_ptr(), C.byref(env._c), B, R, _ptr(masks), steps, *tr,
        b.actions_out.data_ptr(), b.reward_out.data_ptr(), b.done_out.data_ptr(), b.ep_stats.data_ptr(),
        _ptr(b.ep_sum) if with_sums else None, _ptr(b.ep_cnt) if with_sums else None,
        *_log_args(b, with_log, tag0 + step0), stream))


def _three(env, frag, b, masks, tag0=3, traces=TRACES, with_log=True, with_sums=True):
    """The yardstick: steps x (lb_ds_q_argmax, lb_step, lb_ppo_record), each step's actions,
    rewards and dones copied to its trace row."""
    from lbk8s import _native
    L = _native.lib()
    B, R = b.B, b.R
    cfg, state = C.byref(env._c), env.state.data_ptr()
    scratch = torch.empty(B, device="cuda")
    for i in range(b.steps):
        _native.check(L.lb_ds_q_argmax(frag.data_ptr(), b.obs.data_ptr(), B, R, _ptr(masks), None,
                                       b.actions_out.data_ptr(), None))
        _native.check(L.lb_step(state, cfg, B, b.actions_out.data_ptr(), b.obs.data_ptr(), b.reward_out.data_ptr(),
                                b.done_out.data_ptr(), None, b.ep_stats.data_ptr(), None, None))
        lg = _log_args(b, with_log, tag0 + i)
        _native.check(L.lb_ppo_record(B, b.done_out.data_ptr(), b.ep_stats.data_ptr(), scratch.data_ptr(),
                                      _ptr(b.ep_sum) if with_sums else None, _ptr(b.ep_cnt) if with_sums else None,
                                      b.reward_out.data_ptr() if with_log else None, env._rew64 if with_log else None,
                                      b.actions_out.data_ptr() if with_log else None,
                                      lg[0], lg[1], lg[2], lg[3], lg[4], lg[5], None))
        for k, src in zip(TRACES, (b.actions_out, b.reward_out, b.done_out)):
            if k in traces:
                getattr(b, k)[i * B:(i + 1) * B].copy_(src[:B])


def _rew64(env):
    off = env._rew64.value - env.state.data_ptr()
    return env.state[off:off + 8 * env.num_envs].view(torch.float64)


def _same_env(a, b):
    from lbk8s import _native
    assert _same(_rew64(a), _rew64(b))
    assert _same(a.stats(), b.stats())
    for f in _native.LB_FIELD:
        assert _same(a.field(f), b.field(f)), f
    assert torch.equal(a.state, b.state)  # the whole blob: counters, scenario, tables


def _compare(fa, fb, cap_all=True):
    for k in Bufs.ALL:
        if k == "log":  # (rows are unordered within a call: compared sorted, below)
            continue
        assert _same(getattr(fa, k), getattr(fb, k)), k
    if cap_all:
        ra, rb = fa.rows(), fb.rows()
        # (bit patterns: with auto-reset off lb_step writes no ep_stats row, and the log row copies the buffer's NaN)
        assert ra.shape == rb.shape and np.array_equal(_np_bits(ra[:, :21]), _np_bits(rb[:, :21]))


def _masks(B, R):
    return torch.from_numpy(dqn_ref.random_masks(B, R, seed=B)).cuda()


def _run_pair(B, E, rej, steps, L=L_EP, auto=True, masks=False, kind="dqn", cap=None, **opt):
    ea, eb = _env(B, E, rej, L, auto), _env(B, E, rej, L, auto)
    assert torch.equal(ea.state, eb.state) and torch.equal(ea.obs, eb.obs)
    R = ea.cfg.obs_rows
    assert ea.eval_steps_supported(R)
    frag = _frag(kind)
    m = _masks(B, R) if masks else None
    cap = 4 * B if cap is None else cap
    fa, fb = Bufs(ea, steps, cap), Bufs(eb, steps, cap)
    _fused(ea, frag, fa, m, **opt)
    _three(eb, frag, fb, m, **opt)
    torch.cuda.synchronize()
    return ea, eb, fa, fb, frag, m


def _check_pair(ea, eb, fa, fb, m, steps, L=L_EP, auto=True, **opt):
    opt = {k: v for k, v in opt.items() if k in ("traces", "with_log", "with_sums")}
    B, R = fa.B, fa.R
    _compare(fa, fb)
    fa.guards_intact()
    fa.written(**opt)
    _same_env(ea, eb)
    traces = opt.get("traces", TRACES)
    if "actions_all" in traces:
        a = fa.actions_all[:steps * B].view(steps, B)
        assert torch.equal(a[-1], fa.actions_out[:B])
        if m is not None:
            # env 0 has no valid row and takes action 0, env 1 only its last; no other env takes a masked row
            assert (a[:, 0] == 0).all()
            if B > 1:
                assert (a[:, 1] == R - 1).all()
            taken = m.bool()[torch.arange(B, device="cuda")[None].expand(steps, B), a.long()]
            assert (taken | ~m.bool().any(1)[None]).all()
    if "rewards_all" in traces:
        assert _same(fa.rewards_all[(steps - 1) * B:steps * B], fa.reward_out[:B])
    if "dones_all" in traces:
        d = fa.dones_all[:steps * B].view(steps, B)
        assert torch.equal(d[-1], fa.done_out[:B])
        if opt.get("with_sums", True):
            ended = fa.ep_cnt[:B] - fa.init["ep_cnt"][:B]
            assert torch.equal(d.sum(0).double(), ended)
            if opt.get("with_log", True):
                assert int(fa.count[0].item()) == int(ended.sum().item())
        if auto:  # even envs are one step into their episode of L, odd ones at its start
            ev = torch.arange(B, device="cuda") % 2 == 0
            for i in range(steps):
                want = (ev & ((i + 2) % L == 0)) | (~ev & ((i + 1) % L == 0))
                assert torch.equal(d[i].bool(), want), i
        else:
            assert steps == L and not d[:-1].any() and d[-1].all()


# name: (B, E, rejection, steps, options); B None: 8 CUs' worth of SIMDs + 1
CASES = {
    "r1": (1, 1, False, 13, {}),
    "r1_masks": (1, 1, False, 4, dict(masks=True)),
    "run_py_1": (8, 6, True, 1, {}),                      # no episode ends
    "run_py_4": (8, 6, True, 4, dict(masks=True)),        # the even envs' episode ends on the last step
    "run_py_5": (8, 6, True, 5, dict(kind="ppo")),        # the odd envs' too
    "run_py_13": (8, 6, True, 13, dict(masks=True, kind="ppo")),   # several episodes per env
    "ragged": (130, 8, True, 13, dict(masks=True)),
    "ragged_no_masks": (130, 8, True, 4, {}),
    "two_per_wave": (None, 8, True, 5, dict(masks=True)),
    "r16": (67, 16, False, 5, dict(masks=True)),
    "r16_reject": (67, 15, True, 13, dict(kind="ppo")),
    "no_reset_run_py": (8, 6, True, L_EP, dict(auto=False)),     # run_test's: auto-reset off, steps == L
    "no_reset_ragged": (131, 8, True, L_EP, dict(auto=False, masks=True, kind="ppo")),
    "no_traces": (130, 8, True, 13, dict(traces=())),
    "actions_alone": (8, 6, True, 13, dict(traces=("actions_all",), masks=True)),
    "rewards_alone": (8, 6, True, 13, dict(traces=("rewards_all",))),
    "dones_alone": (131, 8, True, 5, dict(traces=("dones_all",))),
    "no_log": (130, 8, True, 13, dict(with_log=False, masks=True)),
    "no_sums": (8, 6, True, 13, dict(with_sums=False)),
    "no_log_no_sums_no_traces": (67, 16, False, 13, dict(with_log=False, with_sums=False, traces=())),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_eval_steps_equals_three_launches(name):
    from lbk8s import fused
    B, E, rej, steps, opt = CASES[name]
    if B is None:
        # lb_ds_q_argmax itself takes two envs per wave here and one at 130: lb_eval_steps' forward
        # (always two) must give either's bits
        B = 8 * torch.cuda.get_device_properties(0).multi_processor_count + 1
        assert fused.forward_kernel(fused.FWD_ARGMAX, B, 9)[:2] == (1, 2)
        assert fused.forward_kernel(fused.FWD_ARGMAX, 130, 9)[:2] == (1, 1)
    ea, eb, fa, fb, _, m = _run_pair(B, E, rej, steps, **opt)
    _check_pair(ea, eb, fa, fb, m, steps, **opt)
    if opt.get("with_sums", True) and opt.get("auto", True):
        ended = fa.ep_cnt[:B] - fa.init["ep_cnt"][:B]
        if steps == 13:
            assert ended.min().item() >= 2  # every env ended at least twice inside the launch
        elif steps == 1:
            assert ended.sum().item() == 0 and fa.rows().shape[0] == 0


def test_eval_steps_full_log_counts_dropped_rows():
    """cap = half the finished episodes: *count is the full count, cap rows are stored, each a
    distinct row of the uncapped three-launch run."""
    B, E, rej, steps = 130, 8, True, 13
    _, _, _, ref, _, _ = _run_pair(B, E, rej, steps, masks=True)
    full = int(ref.count[0].item())
    assert full >= 2 * B
    cap = full // 2
    ea, eb, fa, fb, _, _ = _run_pair(B, E, rej, steps, masks=True, cap=cap)
    assert int(fa.count[0].item()) == full == int(fb.count[0].item())
    _compare(fa, fb, cap_all=False)
    fa.guards_intact()
    _same_env(ea, eb)
    want = {(r[20], r[19]): r for r in ref.rows()}
    got = fa.rows()
    assert got.shape[0] == cap and len({(r[20], r[19]) for r in got}) == cap
    for r in got:
        assert np.array_equal(r[:21], want[(r[20], r[19])][:21])


def test_two_launches_equal_one():
    """6 + 7 steps == 13 steps: the state, the observations, ret32 and the sums carry across
    launches."""
    B, E, rej, steps = 130, 8, True, 13
    ea, eb, fa, fb, frag, m = _run_pair(B, E, rej, steps, masks=True)
    _compare(fa, fb)
    ec = _env(B, E, rej, L_EP)
    fc = Bufs(ec, steps, fa.cap)
    _fused(ec, frag, fc, m, steps=6, step0=0)
    _fused(ec, frag, fc, m, steps=7, step0=6)
    torch.cuda.synchronize()
    _compare(fc, fa)
    fc.guards_intact()
    _same_env(ec, ea)


def test_graph_replay_writes_the_same_bits():
    """The launch captured in a graph (one kernel node) and replayed once == the eager launch."""
    B, E, rej, steps = 8, 6, True, 13
    ea, eb, fa, fb, frag, m = _run_pair(B, E, rej, steps, masks=True)
    _compare(fa, fb)
    ec = _env(B, E, rej, L_EP)
    snap = ec.state.clone()
    fc = Bufs(ec, steps, fa.cap)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _fused(ec, frag, fc, m, stream=torch.cuda.current_stream().cuda_stream)
    ec.state.copy_(snap)
    fc.restore()
    g.replay()
    torch.cuda.synchronize()
    _compare(fc, fa)
    fc.guards_intact()
    _same_env(ec, ea)


def test_vec_env_eval_steps_matches_the_abi_and_checks_its_arguments():
    """LBVecEnv.eval_steps writes the env's own buffers and the caller's trace as the C call does."""
    B, E, rej, steps = 8, 6, True, 13
    ea, eb, fa, fb, frag, m = _run_pair(B, E, rej, steps, masks=True, with_log=False)
    env = _env(B, E, rej, L_EP)
    R = env.cfg.obs_rows
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda")
    good = dict(frag=frag, obs=env.obs, steps=steps, masks=m.bool(), actions_all=z(steps, B, dt=torch.int32),
                rewards_all=z(steps, B), dones_all=z(steps, B, dt=torch.uint8), ep_sum=z(B, dt=torch.float64),
                ep_cnt=z(B, dt=torch.float64))
    for kw in (dict(actions_all=z(steps, B, dt=torch.int64)), dict(rewards_all=z(B, steps).t()),
               dict(dones_all=z(steps, B + 1, dt=torch.uint8)), dict(masks=m), dict(ep_sum=None), dict(ep_cnt=z(B)),
               dict(obs=z(B, R, 4)), dict(frag=frag.cpu()), dict(steps=0), dict(actions_all=z(steps - 1, B, dt=torch.int32))):
        with pytest.raises(ValueError, match="eval_steps"):
            env.eval_steps(**dict(good, **kw))
    assert torch.equal(env.state, _env(B, E, rej, L_EP).state)  # a refused call launched nothing
    assert env.eval_steps(**good) is env.obs
    torch.cuda.synchronize()
    assert _same(env.obs.reshape(-1), fa.obs[:B * R * 8])
    assert torch.equal(good["actions_all"].reshape(-1), fa.actions_all[:steps * B])
    assert _same(good["rewards_all"].reshape(-1), fa.rewards_all[:steps * B])
    assert torch.equal(good["dones_all"].reshape(-1), fa.dones_all[:steps * B])
    assert torch.equal(env.actions, fa.actions_out[:B]) and _same(env.rewards, fa.reward_out[:B])
    assert torch.equal(env.dones, fa.done_out[:B])
    ended = good["dones_all"].sum(0).double()
    assert torch.equal(good["ep_cnt"], ended) and ended.min().item() >= 2
    _same_env(env, ea)
