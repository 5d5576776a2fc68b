"""lb_gae and lb_ppo_record (ABI 17) on the MI355X against the numpy models of
tests/ppo_tail_ref.py (pinned to the reference on the CPU by tests/test_ppo_tail_ref.py), and
PPO_DeepSets(fused_bookkeeping=True) against the default learner.

Everything but the logged mean return is compared for bit equality: lb_gae is the float32
recurrence op for op, lb_ppo_record's sums are sequential per env.  Shapes are the smallest that
reach each path: one env, a partial wave, one wave and a block tail (64-thread GAE blocks,
256-thread record blocks), T on both sides of the GAE loop's unroll of 4 (1, 2, 5, 24, 128),
and 4099 envs (several blocks, a ragged last one).  Output buffers are longer than the kernels
may write and arrive filled with NaN.
"""
import inspect
import types

import numpy as np
import pytest
import torch

import ppo_tail_ref as pr

pytestmark = pytest.mark.gpu

PAD = 64


def _up(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _padded(n, dtype=torch.float32):
    """A NaN-filled buffer of n + PAD elements."""
    return torch.full((n + PAD,), float("nan"), dtype=dtype, device="cuda")


def _tail_untouched(buf, n):
    return bool(torch.isnan(buf[n:]).all())


# ---- lb_gae ---------------------------------------------------------------------------------------
def _run_gae(x, gamma, lam):
    from lbk8s.ppo import gae_device
    T, B = x["rewards"].shape
    t = {k: _up(v) for k, v in x.items()}
    adv, ret = _padded(T * B), _padded(T * B)
    out = (adv[:T * B].view(T, B), ret[:T * B].view(T, B))
    got = gae_device(t["rewards"], t["values"], t["dones"], t["next_value"], t["next_done"], gamma, lam, out=out)
    torch.cuda.synchronize()
    assert got[0] is out[0] and got[1] is out[1]
    assert _tail_untouched(adv, T * B) and _tail_untouched(ret, T * B)
    return out[0].cpu().numpy(), out[1].cpu().numpy(), t


@pytest.mark.parametrize("p_done", (0.0, 1.0, 0.2))
@pytest.mark.parametrize("T,B", ((1, 1), (1, 65), (2, 64), (5, 257), (128, 4099)))
def test_gae_matches_numpy_model_bitwise(T, B, p_done):
    x = pr.gae_inputs(T, B, p_done, seed=7 * T + B)
    gamma, lam = 0.95, 0.97
    want_adv, want_ret = pr.gae_ref(gamma=gamma, gae_lambda=lam, **x)
    adv, ret, _ = _run_gae(x, gamma, lam)
    assert np.array_equal(adv, want_adv)
    assert np.array_equal(ret, want_ret)


def test_gae_matches_reference_learn_bitwise():
    """(24, 4): the reference's own learn() tensors, against the model and the fixture's results."""
    d = pr.gae_fixture()
    x = {k: d[k].astype(np.float32) for k in ("rewards", "values", "dones")}
    x["next_value"] = d["next_value"].astype(np.float32).reshape(-1)
    x["next_done"] = d["next_done"].astype(np.float32).reshape(-1)
    assert x["rewards"].shape == (24, 4)
    gamma, lam = float(d["gamma"]), float(d["gae_lambda"])
    want_adv, want_ret = pr.gae_ref(gamma=gamma, gae_lambda=lam, **x)
    adv, ret, _ = _run_gae(x, gamma, lam)
    assert np.array_equal(adv, want_adv) and np.array_equal(ret, want_ret)
    assert np.array_equal(adv, d["advantages"]) and np.array_equal(ret, d["returns"])


def test_gae_graph_replay_writes_the_same_bits():
    """One launch on one stream, captured with torch.cuda.graph and replayed twice."""
    from lbk8s.ppo import gae_device
    T, B = 5, 257
    x = pr.gae_inputs(T, B, 0.2, seed=11)
    adv, ret, t = _run_gae(x, 0.95, 0.97)
    out = (torch.full((T, B), float("nan"), device="cuda"), torch.full((T, B), float("nan"), device="cuda"))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gae_device(t["rewards"], t["values"], t["dones"], t["next_value"], t["next_done"], 0.95, 0.97, out=out)
    for _ in range(2):
        out[0].fill_(float("nan"))
        out[1].fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out[0].cpu().numpy(), adv) and np.array_equal(out[1].cpu().numpy(), ret)


def test_gae_device_argument_checks():
    from lbk8s.ppo import gae_device
    x = {k: _up(v) for k, v in pr.gae_inputs(4, 6, 0.2, seed=0).items()}
    names = ("rewards", "values", "dones", "next_value", "next_done")
    call = lambda out=None, **kw: gae_device(*[dict(x, **kw)[k] for k in names], 0.95, 0.97, out=out)
    for kw in (dict(values=x["values"].double()), dict(dones=x["dones"].t().contiguous().t()),
               dict(next_done=x["next_done"][:5]), dict(rewards=x["rewards"].cpu()), dict(next_value=x["next_value"].cpu())):
        with pytest.raises(ValueError, match="gae_device"):
            call(**kw)
    with pytest.raises(ValueError, match="gae_device"):
        call(out=(torch.zeros(4, 6, device="cuda"), torch.zeros(4, 5, device="cuda")))
    with pytest.raises(RuntimeError, match="lb_gae"):  # an output that is an input: refused by the library
        call(out=(x["rewards"], torch.zeros(4, 6, device="cuda")))
    adv, ret = call(next_value=x["next_value"].view(1, 6))  # (update()'s shape; buffers allocated here)
    assert adv.shape == ret.shape == (4, 6)


# ---- lb_ppo_record --------------------------------------------------------------------------------
PATTERNS = ("none", "all", ("one", 0), ("one", 63), ("one", 64), ("p", 0.3))
TAGS = (5, 6, 9)


class _Bufs:
    """One set of device buffers of a record / episode-log sequence, NaN-padded."""

    def __init__(self, B, ret32, cap):
        self.B, self.cap = B, cap
        self.next_done = _padded(B)
        self.ep_sum = _padded(B, torch.float64)
        self.ep_cnt = _padded(B, torch.float64)
        self.ep_sum[:B] = 0
        self.ep_cnt[:B] = 0
        self.ret32 = _padded(B)
        self.ret32[:B] = _up(ret32)
        self.ep_r32 = _padded(B)
        self.log = _padded(max(cap, 1) * pr.LB_EPLOG_W, torch.float64)
        self.count = torch.zeros(1 + PAD, dtype=torch.int32, device="cuda")

    def rows(self):
        n = min(int(self.count[0].item()), self.cap)
        return self.log[:n * pr.LB_EPLOG_W].view(n, pr.LB_EPLOG_W).cpu().numpy()

    def check_tails(self, stored=None):
        B = self.B
        for name in ("next_done", "ep_sum", "ep_cnt", "ret32", "ep_r32"):
            assert _tail_untouched(getattr(self, name), B), name
        n = min(int(self.count[0].item()), self.cap) if stored is None else stored
        assert _tail_untouched(self.log, n * pr.LB_EPLOG_W)
        assert not self.count[1:].any()


def _record(L, native, B, done, st, b, step, with_log, use_r64, use_epr):
    rew, r64, act, tag = step
    native.check(L.lb_ppo_record(
        B, done.data_ptr(), st.data_ptr(), b.next_done.data_ptr(), b.ep_sum.data_ptr(), b.ep_cnt.data_ptr(),
        _ptr(rew) if with_log else None, _ptr(r64) if with_log and use_r64 else None, _ptr(act) if with_log else None,
        _ptr(b.ret32) if with_log else None, _ptr(b.ep_r32) if with_log and use_epr else None, tag,
        _ptr(b.log) if with_log else None, b.cap if with_log else 0, _ptr(b.count) if with_log else None, None))


@pytest.mark.parametrize("B", (1, 63, 64, 65, 257, 4099))
def test_ppo_record_matches_model_and_episode_log(B):
    from lbk8s import _native
    L = _native.lib()
    rng = np.random.default_rng(100 + B)
    for first in range(len(PATTERNS)):
        use_r64, use_epr = first % 2 == 0, first % 3 != 2
        ret0 = rng.standard_normal(B).astype(np.float32)
        rec, nolog, eplog = _Bufs(B, ret0, B * 3), _Bufs(B, ret0, B * 3), _Bufs(B, ret0, B * 3)
        m_sum, m_cnt = np.zeros(B), np.zeros(B)
        model = dict(ret32=ret0.copy(), ep_r32=np.full(B, np.nan, np.float32) if use_epr else None, rows=[], count=0)
        for call, tag in enumerate(TAGS):
            done = pr.done_pattern(PATTERNS[(first + call) % len(PATTERNS)], B, rng)
            st = rng.standard_normal((B, pr.LB_ST_K)) * 50
            rew64 = rng.standard_normal(B)
            rew, act = rew64.astype(np.float32), rng.integers(0, 9, B).astype(np.int32)
            model.update(reward=rew, reward64=rew64 if use_r64 else None, actions=act, tag=tag)
            want_nd = pr.ppo_record_ref(done, st, m_sum, m_cnt, model)
            d_done, d_st = _up(done), _up(st)
            step = (_up(rew), _up(rew64), _up(act), tag)
            for b in (rec, nolog, eplog):
                b.next_done[:B] = float("nan")
            _record(L, _native, B, d_done, d_st, rec, step, True, use_r64, use_epr)
            _record(L, _native, B, d_done, d_st, nolog, step, False, use_r64, use_epr)
            _native.check(L.lb_episode_log(B, d_done.data_ptr(), d_st.data_ptr(), step[0].data_ptr(),
                                           _ptr(step[1]) if use_r64 else None, step[2].data_ptr(),
                                           eplog.ret32.data_ptr(), _ptr(eplog.ep_r32) if use_epr else None, tag,
                                           eplog.log.data_ptr(), eplog.cap, eplog.count.data_ptr(), None))
            torch.cuda.synchronize()
            for b in (rec, nolog):  # the per-step outputs, with and without a log
                assert np.array_equal(b.next_done[:B].cpu().numpy(), want_nd)
                assert np.array_equal(b.ep_sum[:B].cpu().numpy(), m_sum)
                assert np.array_equal(b.ep_cnt[:B].cpu().numpy(), m_cnt)
            for b in (rec, eplog):  # the log: the model's, and lb_episode_log's on the same inputs
                assert np.array_equal(b.ret32[:B].cpu().numpy(), model["ret32"])
                assert int(b.count[0].item()) == model["count"]
                if use_epr:
                    assert np.array_equal(b.ep_r32[:B].cpu().numpy(), model["ep_r32"], equal_nan=True)
                else:
                    assert bool(torch.isnan(b.ep_r32).all())
                assert np.array_equal(pr.sort_rows(b.rows())[:, :21], pr.sort_rows(model["rows"])[:, :21])
        # log = NULL: the log's buffers untouched
        assert np.array_equal(nolog.ret32[:B].cpu().numpy(), ret0)
        assert bool(torch.isnan(nolog.ep_r32).all()) and bool(torch.isnan(nolog.log).all())
        assert not nolog.count.any()
        rec.check_tails()
        eplog.check_tails()
        nolog.check_tails(stored=0)


@pytest.mark.parametrize("B,envs", ((64, (0, 7, 31, 32, 63)), (257, (3, 70, 130, 200, 256))))
def test_ppo_record_full_log_counts_dropped_rows(B, envs):
    """cap = 2 with 5 finished envs (in one wave; in five waves of two blocks): *count == 5 and
    the two stored rows are distinct rows of finished envs."""
    from lbk8s import _native
    L = _native.lib()
    rng = np.random.default_rng(B)
    done = np.zeros(B, np.uint8)
    done[list(envs)] = 1
    st = rng.standard_normal((B, pr.LB_ST_K))
    rew64 = rng.standard_normal(B)
    rew, act = rew64.astype(np.float32), rng.integers(0, 9, B).astype(np.int32)
    ret0 = rng.standard_normal(B).astype(np.float32)
    b = _Bufs(B, ret0, 2)
    m_sum, m_cnt = np.zeros(B), np.zeros(B)
    model = dict(reward=rew, reward64=rew64, actions=act, ret32=ret0.copy(), ep_r32=np.full(B, np.nan, np.float32),
                 tag=3, rows=[], count=0)
    want_nd = pr.ppo_record_ref(done, st, m_sum, m_cnt, model)
    _record(L, _native, B, _up(done), _up(st), b, (_up(rew), _up(rew64), _up(act), 3), True, True, True)
    torch.cuda.synchronize()
    assert int(b.count[0].item()) == 5 == model["count"]
    assert np.array_equal(b.next_done[:B].cpu().numpy(), want_nd)
    assert np.array_equal(b.ep_sum[:B].cpu().numpy(), m_sum) and np.array_equal(b.ep_cnt[:B].cpu().numpy(), m_cnt)
    assert np.array_equal(b.ret32[:B].cpu().numpy(), model["ret32"])
    assert np.array_equal(b.ep_r32[:B].cpu().numpy(), model["ep_r32"], equal_nan=True)
    rows = b.rows()
    assert rows.shape[0] == 2
    stored = [int(e) for e in rows[:, pr.LB_EPLOG_ENV]]
    assert stored[0] != stored[1] and set(stored) <= set(envs)
    by_env = {int(r[pr.LB_EPLOG_ENV]): r for r in model["rows"]}
    for r in rows:
        assert np.array_equal(r[:21], by_env[int(r[pr.LB_EPLOG_ENV])][:21])
    b.check_tails()


# ---- the learner ----------------------------------------------------------------------------------
def _learner_run(monkeypatch, fused_bookkeeping, env_kw, B, T, monitor_file):
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
    algo = ppo.PPO_DeepSets(env, num_steps=T, n_minibatches=4, update_epochs=1, seed=2, fused_act=True,
                            fused_bookkeeping=fused_bookkeeping, use_graphs=False)
    assert algo.fused_act and algo.fused_bookkeeping == fused_bookkeeping
    next_obs = env.reset()
    next_done = torch.zeros(B, device="cuda")
    next_obs, next_done = algo.rollout(next_obs, next_done)
    algo.update(next_obs, next_done)
    torch.cuda.synchronize()
    out = {k: getattr(algo, k).detach().cpu().numpy().copy()
           for k in ("obs", "actions", "logprobs", "rewards", "dones", "values", "advantages", "returns")}
    out["next_done"] = next_done.cpu().numpy().copy()
    env.close()
    csv = open(env._monitor.path, "rb").read() if monitor_file else None
    return out, csv, seen[0], algo.episode_returns


@pytest.mark.parametrize("name,env_kw,B,T,monitored", (
    ("e8", dict(episode_length=3), 64, 8, True),
    ("e64_rejection", dict(num_endpoints=64, rejection_allowed=True, episode_length=2, reward_function="multi",
                           latency_weight=1.0, cpu_weight=0.0, gini_weight=0.0), 16, 4, False)),
    ids=("e8_monitored", "e64_rejection"))
def test_fused_bookkeeping_learner_matches_default(monkeypatch, tmp_path, name, env_kw, B, T, monitored):
    from lbk8s.ppo import PPO_DeepSets
    assert inspect.signature(PPO_DeepSets).parameters["fused_bookkeeping"].default is False
    runs = []
    for fb in (False, True):
        with monkeypatch.context() as mp:
            runs.append(_learner_run(mp, fb, env_kw, B, T, str(tmp_path / f"fb{int(fb)}") if monitored else None))
    (a, csv_a, (sum_a, cnt_a), ret_a), (b, csv_b, (sum_b, cnt_b), ret_b) = runs
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a["dones"][1:].sum() > 0 and np.isfinite(b["advantages"]).all()
    if monitored:
        assert csv_a == csv_b and csv_a.count(b"\n") == 2 + int(cnt_b.sum())
    # the same finished episodes; the per-env accumulators against the default's two scalars
    assert sum_a.shape == () and sum_b.shape == (B,)
    n = float(cnt_b.sum())
    assert n == float(cnt_a) > 0
    assert len(ret_a) == len(ret_b) == 1
    # both means are float64 sums of the same n returns in another order, over n: the difference
    # is bounded by the summation error of the B per-env sums x_i, B * 2^-53 * sum|x_i|, over n
    bound = B * 2.0 ** -53 * np.abs(sum_b).sum() / n
    diff = abs(ret_a[0] - ret_b[0])
    print(f"fused-bookkeeping {name}: episodes={n:.0f} mean={ret_b[0]!r} |diff|={diff:.3e} bound={bound:.3e}")
    assert diff <= bound
