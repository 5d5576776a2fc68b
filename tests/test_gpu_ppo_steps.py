"""lb_ppo_steps (csrc/lbk8s_ppo.h): a PPO rollout's vector steps in ONE launch == steps x
(lb_ds_sample, lb_step, lb_ppo_record), bit for bit, through the C ABI.  The yardstick is the
three existing launches, each pinned to its own reference (tests/test_gpu_ds_sample.py,
tests/test_gpu_parity.py, tests/test_gpu_ppo_tail.py).

Per case two envs are built from the same seed and brought out of phase (one random step, then a
reset of the odd envs), and one seeded DeepSetAgent image is packed.  Every output buffer starts
as NaN (integers: a sentinel) with 64 guard elements past its end: the guards must survive and
everything the header says is written must be overwritten.  Shapes: R = 1, run.py's own (8 envs,
E = 6), a ragged last group (130 = 65 groups of two), R = 16 with and without the reject row, a
batch at which lb_ds_sample itself takes two envs per wave (8 CUs' worth of SIMDs + 1) next to
one where it takes one (130), and a one-step launch in which nothing ends.
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PAD = 64
W = 24  # LB_EPLOG_W
INT = {torch.float32: torch.int32, torch.float64: torch.int64}


def _bits(t):
    return t.view(INT[t.dtype]) if t.dtype in INT else t


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _nan(n, dtype=torch.float32):
    return torch.full((n + PAD,), float("nan"), dtype=dtype, device="cuda")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _env(B, E, rej, L, seed=11):
    """A reset env whose envs are out of phase: the even ones one step into their episode."""
    from lbk8s import LBVecEnv
    env = LBVecEnv(B, seed=seed, as_tensors=True, num_endpoints=E, rejection_allowed=rej, episode_length=L,
                   reward_function="multi")
    env.reset()
    if L > 1:
        env.step_device(None)
        env.reset_masked((torch.arange(B, device="cuda") % 2).to(torch.uint8))
    return env


_frags = {}


def _frag(env):
    """One seeded DeepSetAgent's weight image per observation shape, left unchanged."""
    from lbk8s import fused
    from lbk8s.deepsets import DeepSetAgent
    R = env.cfg.obs_rows
    if R not in _frags:
        torch.manual_seed(5)
        agent = DeepSetAgent(env).cuda()
        _frags[R] = (agent, fused.packed(agent, agent.actor.net, agent.critic).clone())
    return _frags[R][1]


class Bufs:
    """One side's buffers of a `steps`-step sequence with `S` stored rows."""
    F32 = ("actions_f32", "logprobs", "values", "rewards", "obs_next", "dones_next", "last_obs", "last_done", "ret32",
           "ep_r32")
    F64 = ("ep_stats", "ep_sum", "ep_cnt", "log")
    ALL = F32 + F64 + ("actions_out", "done_out", "count")

    def __init__(self, B, R, steps, S, cap):
        self.B, self.R, self.steps, self.S, self.cap = B, R, steps, S, cap
        self.n = dict(actions_f32=steps * B, logprobs=steps * B, values=steps * B, rewards=steps * B,
                      obs_next=S * B * R * 8, dones_next=S * B, last_obs=B * R * 8, last_done=B, ret32=B, ep_r32=B,
                      ep_stats=B * 16, ep_sum=B, ep_cnt=B, log=max(cap, 1) * W, actions_out=B, done_out=B, count=1)
        for k in self.F32:
            setattr(self, k, _nan(self.n[k]))
        for k in self.F64:
            setattr(self, k, _nan(self.n[k], torch.float64))
        g = torch.Generator().manual_seed(B)
        self.ret32[:B] = torch.randn(B, generator=g).cuda()
        self.ep_sum[:B] = (torch.arange(B, dtype=torch.float64) * 0.25).cuda()
        self.ep_cnt[:B] = (torch.arange(B, dtype=torch.float64) % 3).cuda()
        self.actions_out = torch.full((B + PAD,), -77, dtype=torch.int32, device="cuda")
        self.done_out = torch.full((B + PAD,), 0xAB, dtype=torch.uint8, device="cuda")
        self.count = torch.zeros(1 + PAD, dtype=torch.int32, device="cuda")
        self.init = {k: getattr(self, k).clone() for k in self.ALL}

    def restore(self):
        for k in self.ALL:
            getattr(self, k).copy_(self.init[k])

    def guards_intact(self):
        for k in self.ALL:
            assert _same(getattr(self, k)[self.n[k]:], self.init[k][self.n[k]:]), k

    def written(self, with_log=True):
        """Everything the header says is written holds a value."""
        S, B = self.S, self.B
        for k in ("actions_f32", "logprobs", "values", "rewards", "obs_next", "dones_next"):
            assert not torch.isnan(getattr(self, k)[:self.n[k]]).any(), k
        if S < self.steps:
            assert not torch.isnan(self.last_obs[:self.n["last_obs"]]).any()
            assert not torch.isnan(self.last_done[:B]).any()
        else:
            assert torch.isnan(self.last_obs).all() and torch.isnan(self.last_done).all()
        assert (self.actions_out[:B] >= 0).all() and (self.actions_out[:B] < self.R).all()
        assert (self.done_out[:B] <= 1).all()
        if not with_log:
            for k in ("ret32", "ep_r32", "log", "count"):
                assert _same(getattr(self, k), self.init[k]), k

    def rows(self):
        n = min(int(self.count[0].item()), self.cap)
        r = self.log[:n * W].view(n, W).cpu().numpy()
        return r[np.lexsort((r[:, 19], r[:, 20]))]


def _log_args(b, with_log, tag0):
    if not with_log:
        return (None, None, 0, None, 0, None)
    return (_ptr(b.ret32), _ptr(b.ep_r32), tag0, _ptr(b.log), b.cap, _ptr(b.count))


def _row(buf, i, n):
    return buf.data_ptr() + 4 * i * n


def _fused(env, frag, obs, u, b, steps=None, S=None, step0=0, tag0=0, with_log=True, stream=None):
    """lb_ppo_steps of the steps step0 .. step0 + steps - 1 of b's sequence."""
    from lbk8s import _native
    B, R = b.B, b.R
    steps = b.steps if steps is None else steps
    S = b.S - step0 if S is None else S
    _native.check(_native.lib().lb_ppo_steps(
        frag.data_ptr(), obs, env.state.data_ptr(), C.byref(env._c), B, R, steps, S, _row(u, step0, B),
        _row(b.actions_f32, step0, B), _row(b.logprobs, step0, B), _row(b.values, step0, B), _row(b.rewards, step0, B),
        _row(b.obs_next, step0, B * R * 8), _row(b.dones_next, step0, B), _ptr(b.last_obs), _ptr(b.last_done),
        b.actions_out.data_ptr(), b.done_out.data_ptr(), b.ep_stats.data_ptr(), b.ep_sum.data_ptr(),
        b.ep_cnt.data_ptr(), *_log_args(b, with_log, tag0 + step0), stream))


def _three(env, frag, obs, u, b, with_log=True):
    """The yardstick: steps x (lb_ds_sample, lb_step, lb_ppo_record)."""
    from lbk8s import _native
    L = _native.lib()
    B, R = b.B, b.R
    cfg, state = C.byref(env._c), env.state.data_ptr()
    for i in range(b.steps):
        stored = i < b.S
        nobs = _row(b.obs_next, i, B * R * 8) if stored else b.last_obs.data_ptr()
        ndone = _row(b.dones_next, i, B) if stored else b.last_done.data_ptr()
        _native.check(L.lb_ds_sample(frag.data_ptr(), obs, B, R, None, _row(u, i, B), None, b.actions_out.data_ptr(),
                                     _row(b.actions_f32, i, B), _row(b.logprobs, i, B), _row(b.values, i, B), None))
        _native.check(L.lb_step(state, cfg, B, b.actions_out.data_ptr(), nobs, _row(b.rewards, i, B),
                                b.done_out.data_ptr(), None, b.ep_stats.data_ptr(), None, None))
        lg = _log_args(b, with_log, i)
        _native.check(L.lb_ppo_record(B, b.done_out.data_ptr(), b.ep_stats.data_ptr(), ndone, b.ep_sum.data_ptr(),
                                      b.ep_cnt.data_ptr(), _row(b.rewards, i, B) if with_log else None,
                                      env._rew64 if with_log else None, b.actions_out.data_ptr() if with_log else None,
                                      lg[0], lg[1], lg[2], lg[3], lg[4], lg[5], None))
        obs = nobs


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
        assert ra.shape == rb.shape and np.array_equal(ra[:, :21], rb[:, :21])


def _uniforms(steps, B):
    g = torch.Generator().manual_seed(steps * 1000 + B)
    u = torch.rand((steps, B), generator=g).cuda()
    u[0, 0] = 0.0  # the CDF's first row
    return u


def _run_pair(B, E, rej, L, steps, S=None, with_log=True, cap=None):
    S = steps - 1 if S is None else S
    ea, eb = _env(B, E, rej, L), _env(B, E, rej, L)
    assert torch.equal(ea.state, eb.state) and torch.equal(ea.obs, eb.obs)
    R = ea.cfg.obs_rows
    assert ea.ppo_steps_supported(R)
    frag = _frag(ea)
    u = _uniforms(steps, B)
    cap = 3 * B if cap is None else cap
    fa, fb = Bufs(B, R, steps, S, cap), Bufs(B, R, steps, S, cap)
    _fused(ea, frag, ea.obs.data_ptr(), u, fa, with_log=with_log)
    _three(eb, frag, eb.obs.data_ptr(), u, fb, with_log=with_log)
    torch.cuda.synchronize()
    return ea, eb, fa, fb, u, frag


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


CASES = {"r1": (1, 1, False, 2, 5), "run_py": (8, 6, True, 3, 7), "ragged": (130, 8, True, 4, 9),
         "r16": (67, 16, False, 2, 5), "r16_reject": (67, 15, True, 2, 5), "two_per_wave": (None, 8, True, 5, 3),
         "one_step": (64, 8, True, 100, 1)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_ppo_steps_equals_three_launches(name):
    from lbk8s import fused
    B, E, rej, L, steps = CASES[name]
    if B is None:
        # lb_ds_sample itself takes two envs per wave here and one at 130: lb_ppo_steps' forward
        # (always two) must give either's bits
        B = 8 * _cus() + 1
        assert fused.forward_kernel(fused.FWD_SAMPLE, B, 9)[:2] == (1, 2)
        assert fused.forward_kernel(fused.FWD_SAMPLE, 130, 9)[:2] == (1, 1)
    ea, eb, fa, fb, _, _ = _run_pair(B, E, rej, L, steps)
    _compare(fa, fb)
    fa.guards_intact()
    fa.written()
    _same_env(ea, eb)
    ended = fa.ep_cnt[:B] - fa.init["ep_cnt"][:B]
    assert int(fa.count[0].item()) == int(ended.sum().item())
    if L < steps:
        assert ended.max().item() >= 2  # an env ended twice inside the launch
        assert ended.min().item() >= 1
    elif name == "one_step":
        assert ended.sum().item() == 0 and fa.rows().shape[0] == 0


def test_ppo_steps_without_log_and_with_all_rows_stored():
    """log = NULL: ret32, ep_r32, the log and the counter are not touched; store_rows = steps: the
    last step's rows go to the storage too and last_* stay as they were."""
    B, E, rej, L, steps = CASES["run_py"]
    ea, eb, fa, fb, _, _ = _run_pair(B, E, rej, L, steps, S=steps, with_log=False)
    _compare(fa, fb)
    fa.guards_intact()
    fa.written(with_log=False)
    _same_env(ea, eb)
    assert (fa.ep_cnt[:B] - fa.init["ep_cnt"][:B]).max().item() >= 2


def test_ppo_steps_full_log_counts_dropped_rows():
    """cap = half the finished episodes: *count is the full count, cap rows are stored, each a
    distinct row of the uncapped three-launch run."""
    B, E, rej, L, steps = CASES["ragged"]
    _, _, _, ref, _, _ = _run_pair(B, E, rej, L, steps)
    full = int(ref.count[0].item())
    assert full >= 2 * B
    cap = full // 2
    ea, eb, fa, fb, _, _ = _run_pair(B, E, rej, L, steps, cap=cap)
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
    """4 + 5 steps (store_rows = steps on the first: its last observations are the second's
    input) == 9 steps."""
    B, E, rej, L, steps = CASES["ragged"]
    ea, eb, fa, fb, u, frag = _run_pair(B, E, rej, L, steps)
    _compare(fa, fb)
    ec = _env(B, E, rej, L)
    fc = Bufs(B, fa.R, steps, steps - 1, fa.cap)
    _fused(ec, frag, ec.obs.data_ptr(), u, fc, steps=4, S=4, step0=0)
    _fused(ec, frag, _row(fc.obs_next, 3, B * fa.R * 8), u, fc, steps=5, S=4, step0=4)
    torch.cuda.synchronize()
    _compare(fc, fa)
    fc.guards_intact()
    _same_env(ec, ea)


def test_graph_replay_writes_the_same_bits():
    B, E, rej, L, steps = CASES["run_py"]
    ea, eb, fa, fb, u, frag = _run_pair(B, E, rej, L, steps)
    _compare(fa, fb)
    ec = _env(B, E, rej, L)
    snap = ec.state.clone()
    fc = Bufs(B, fa.R, steps, steps - 1, fa.cap)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _fused(ec, frag, ec.obs.data_ptr(), u, fc, stream=torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        ec.state.copy_(snap)
        fc.restore()
        g.replay()
        torch.cuda.synchronize()
        _compare(fc, fa)
        fc.guards_intact()
        _same_env(ec, ea)


def test_vec_env_ppo_steps_argument_checks():
    env = _env(8, 6, True, 3)
    frag = _frag(env)
    B, R, T = 8, 7, 4
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda")
    good = dict(frag=frag, obs=env.obs, uniforms=z(T, B), actions_f32=z(T, B), logprobs=z(T, B), values=z(T, B),
                rewards=z(T, B), obs_next=z(T - 1, B, R, 8), dones_next=z(T - 1, B), last_obs=z(B, R, 8), last_done=z(B),
                actions=z(B, dt=torch.int32), dones=z(B, dt=torch.uint8), ep_sum=z(B, dt=torch.float64),
                ep_cnt=z(B, dt=torch.float64))
    env.ppo_steps(**good)
    for kw in (dict(values=z(T, B, dt=torch.float64)), dict(rewards=z(B, T).t()), dict(logprobs=z(T, B + 1)),
               dict(actions=z(B, dt=torch.int64)), dict(last_obs=None), dict(obs_next=z(T - 2, B, R, 8)),
               dict(dones_next=z(T, B)), dict(ep_sum=z(B)), dict(uniforms=z(T, B).cpu()), dict(obs=z(B, R, 4))):
        with pytest.raises(ValueError, match="ppo_steps"):
            env.ppo_steps(**dict(good, **kw))
    torch.cuda.synchronize()


# ---- the learner ----------------------------------------------------------------------------------
def _learner_run(monkeypatch, flags, env_kw, B, T, monitor_file, want_rollout):
    """One rollout() + update() on a seeded env and agent, under a counting clock (the monitor
    file's time column is the host time of each step)."""
    from lbk8s import LBVecEnv, ppo, vec_env
    ticks = iter(range(1, 1 << 20))
    monkeypatch.setattr(vec_env, "time", types.SimpleNamespace(time=lambda: float(next(ticks))))
    seen = []
    real = ppo.lbdist.mean_episode_return

    def spy(ep_sum, ep_cnt, group=None):
        seen.append((ep_sum.detach().cpu().numpy().copy(), ep_cnt.detach().cpu().numpy().copy()))
        return real(ep_sum, ep_cnt, group)

    monkeypatch.setattr(ppo.lbdist, "mean_episode_return", spy)
    env = LBVecEnv(B, seed=3, as_tensors=True, monitor_file=monitor_file, **env_kw)
    algo = ppo.PPO_DeepSets(env, num_steps=T, n_minibatches=4, update_epochs=1, seed=2, use_graphs=False, **flags)
    assert algo.fused_rollout is want_rollout and algo.fused_bookkeeping
    next_obs = env.reset()
    next_done = torch.zeros(B, device="cuda")
    next_obs, next_done = algo.rollout(next_obs, next_done)
    algo.update(next_obs, next_done)
    torch.cuda.synchronize()
    out = {k: getattr(algo, k).detach().cpu().numpy().copy()
           for k in ("obs", "actions", "logprobs", "rewards", "dones", "values", "advantages", "returns")}
    out["next_done"] = next_done.cpu().numpy().copy()
    out["next_obs"] = next_obs.cpu().numpy().copy()
    env.close()
    csv = open(env._monitor.path, "rb").read() if monitor_file else None
    return out, csv, seen[0], algo.episode_returns


THREE = dict(fused_act=True, fused_bookkeeping=True)
E64 = dict(num_endpoints=64, rejection_allowed=True, episode_length=2, reward_function="multi", latency_weight=1.0,
           cpu_weight=0.0, gini_weight=0.0)


@pytest.mark.parametrize("name,env_kw,B,T,flags,want", (
    ("e8", dict(episode_length=3), 64, 8, dict(fused_rollout=True), True),
    # run.py's shape over several monitor flushes (every min(64, L) = 7 steps: 15 launches)
    ("run_py", dict(num_endpoints=6, rejection_allowed=True, episode_length=7, reward_function="multi"), 8, 100,
     dict(fused_rollout=True), True),
    ("e64", E64, 16, 4, dict(THREE, fused_rollout=True), False)), ids=("e8", "run_py_chunked", "e64_not_supported"))
def test_fused_rollout_learner_matches_three_launches(monkeypatch, tmp_path, name, env_kw, B, T, flags, want):
    runs = []
    for i, fl in enumerate((THREE, flags)):
        with monkeypatch.context() as mp:
            runs.append(_learner_run(mp, fl, env_kw, B, T, str(tmp_path / f"run{i}"), want and i == 1))
    (a, csv_a, (sum_a, cnt_a), ret_a), (b, csv_b, (sum_b, cnt_b), ret_b) = runs
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a["dones"][1:].sum() > 0 and np.isfinite(b["advantages"]).all()
    assert sum_a.shape == sum_b.shape == (B,)
    assert np.array_equal(sum_a, sum_b) and np.array_equal(cnt_a, cnt_b) and cnt_b.sum() > 0
    assert ret_a == ret_b and len(ret_b) == 1
    assert csv_a == csv_b and csv_a.count(b"\n") == 2 + int(cnt_b.sum())
