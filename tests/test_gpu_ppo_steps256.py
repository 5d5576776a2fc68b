"""lb_ppo_steps256 (csrc/lbk8s_ppo256.h): a PPO rollout's vector steps in ONE launch for envs of 65 to
256 endpoints == steps x (lb_ds_sample, lb_step, lb_ppo_record), bit for bit, through the C ABI.
The yardstick is the three existing launches, as in tests/test_gpu_ppo_steps.py, whose buffers
(NaN / sentinel filled, 64 guard elements), envs out of phase, seeded agent image and comparisons
(every storage row, last_obs / last_done, the whole state blob; log rows sorted) are used here as
they are; lb_ds_sample's chunked kernel itself is pinned to the float64 definition at these row
counts by tests/test_gpu_ds_sample_big.py.

Shapes: every kernel instance at its first and last row count -- <2, false> at R = 65 (E = 65 on two
endpoints per lane), 66 and 80; <2, true> at R = 81, 96, 97 (a chunk boundary and one row past it),
128 and 129; <4, true> at R = 129 without the reject row, 181 (the evaluation sweep's largest
size), 193 (the first row of ds_sample_wave's fourth slot), 256 and 257 -- with envs that end
several times inside the launch, a one-step launch in which nothing ends, and more envs than
resident waves (the gi += nwaves loop, a ragged last block) on the first and the last instance.
Uniforms: the seeded table with env 0 drawing u = 0 and env 1 drawing 1 - 2^-24 at step 0 (the
first-row and last-row paths of the draw).
"""
import types

import numpy as np
import pytest
import torch

from test_gpu_ppo_steps import THREE, Bufs, _compare, _cus, _env, _frag, _row, _same_env, _three, _uniforms
from test_gpu_ppo_steps64 import _fused64

pytestmark = pytest.mark.gpu

FN = "lb_ppo_steps256"


def _uniforms256(steps, B):
    u = _uniforms(steps, B)
    assert u[0, 0].item() == 0.0  # the CDF's first row
    if B > 1:
        u[0, 1] = 1.0 - 2.0 ** -24  # its last
    return u


def _run_pair(B, E, rej, L, steps, S=None, with_log=True, cap=None, other=None):
    """lb_ppo_steps256 on one env, the three launches (other: that entry point) on its twin."""
    S = steps - 1 if S is None else S
    ea, eb = _env(B, E, rej, L), _env(B, E, rej, L)
    assert torch.equal(ea.state, eb.state) and torch.equal(ea.obs, eb.obs)
    R = ea.cfg.obs_rows
    assert ea.ppo_steps256_supported(R)
    frag = _frag(ea)
    u = _uniforms256(steps, B)
    cap = 3 * B if cap is None else cap
    fa, fb = Bufs(B, R, steps, S, cap), Bufs(B, R, steps, S, cap)
    _fused64(ea, frag, ea.obs.data_ptr(), u, fa, with_log=with_log, fn=FN)
    if other is None:
        _three(eb, frag, eb.obs.data_ptr(), u, fb, with_log=with_log)
    else:
        _fused64(eb, frag, eb.obs.data_ptr(), u, fb, with_log=with_log, fn=other)
    torch.cuda.synchronize()
    return ea, eb, fa, fb, u, frag


# (B, E, reject, L, steps); B as a string: a multiple of the CU count plus a rest
CASES = {"a_r65_epl2": (9, 65, False, 2, 5), "b_r66": (67, 65, True, 2, 5), "c_r80": (17, 80, False, 3, 7),
         "d_r81": (19, 80, True, 2, 5), "e_r96": (5, 96, False, 2, 5), "f_r97": (7, 96, True, 3, 7),
         "g_r128": (16, 128, False, 2, 5), "h_r129_epl2": (16, 128, True, 2, 9), "i_r129_epl4": (9, 129, False, 2, 5),
         "j_r181": (16, 180, True, 3, 7), "k_r193_slot4": (5, 192, True, 2, 5), "l_r256": (5, 256, False, 2, 5),
         "m_r257": (16, 256, True, 2, 9), "n_one_step": (1, 256, True, 100, 1),
         "o_more_envs_than_waves_r66": ("8c+3", 65, True, 2, 3), "p_more_envs_than_waves_r257": ("8c+3", 256, True, 2, 3)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_ppo_steps256_equals_three_launches(name):
    B, E, rej, L, steps = CASES[name]
    if B == "8c+3":
        B = 8 * _cus() + 3
    ea, eb, fa, fb, u, _ = _run_pair(B, E, rej, L, steps)
    assert not ea.ppo_steps64_supported(fa.R)  # a shape of the new kernels
    _compare(fa, fb)
    fa.guards_intact()
    fa.written()
    _same_env(ea, eb)
    ended = fa.ep_cnt[:B] - fa.init["ep_cnt"][:B]
    assert int(fa.count[0].item()) == int(ended.sum().item())
    if L < steps:
        assert ended.max().item() >= 2  # an env ended twice inside the launch
        assert ended.min().item() >= 1
    elif name == "n_one_step":
        assert ended.sum().item() == 0 and fa.rows().shape[0] == 0
    if name == "m_r257":
        assert ended.min().item() >= 4  # 9 steps of 2-step episodes
    # u = 0 takes the first row with e > 0: row 0 (no masks, and the seeded agent's logits lie far
    # closer together than the 87 at which exp underflows)
    assert u[0, 0].item() == 0.0 and fa.actions_f32[0].item() == 0.0


def test_ppo_steps256_without_log_and_with_all_rows_stored():
    """log = NULL: ret32, ep_r32, the log and the counter are not touched; store_rows = steps: the
    last step's rows go to the storage too and last_* stay as they were."""
    B, E, rej, L, steps = CASES["j_r181"]
    ea, eb, fa, fb, _, _ = _run_pair(B, E, rej, L, steps, S=steps, with_log=False)
    assert not ea.ppo_steps64_supported(fa.R)
    _compare(fa, fb)
    fa.guards_intact()
    fa.written(with_log=False)
    _same_env(ea, eb)
    assert (fa.ep_cnt[:B] - fa.init["ep_cnt"][:B]).max().item() >= 2


def test_ppo_steps256_full_log_counts_dropped_rows():
    """cap = half the finished episodes: *count is the full count, cap rows are stored, each a
    distinct row of the uncapped three-launch run."""
    B, E, rej, L, steps = CASES["m_r257"]
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


@pytest.mark.parametrize("name", ("d_r81", "m_r257"))
def test_two_launches_equal_one(name):
    """4 + 5 steps (store_rows = steps on the first: its last observations are the second's
    input) == 9 steps."""
    B, E, rej, L, _ = CASES[name]
    steps = 9
    ea, eb, fa, fb, u, frag = _run_pair(B, E, rej, L, steps)
    assert not ea.ppo_steps64_supported(fa.R)
    _compare(fa, fb)
    ec = _env(B, E, rej, L)
    fc = Bufs(B, fa.R, steps, steps - 1, fa.cap)
    _fused64(ec, frag, ec.obs.data_ptr(), u, fc, steps=4, S=4, step0=0, fn=FN)
    _fused64(ec, frag, _row(fc.obs_next, 3, B * fa.R * 8), u, fc, steps=5, S=4, step0=4, fn=FN)
    torch.cuda.synchronize()
    _compare(fc, fa)
    fc.guards_intact()
    _same_env(ec, ea)


def test_graph_replay_writes_the_same_bits():
    B, E, rej, L, steps = 9, 129, True, 2, 5  # R = 130
    ea, eb, fa, fb, u, frag = _run_pair(B, E, rej, L, steps)
    assert fa.R == 130 and not ea.ppo_steps64_supported(fa.R)
    _compare(fa, fb)
    ec = _env(B, E, rej, L)
    snap = ec.state.clone()
    fc = Bufs(B, fa.R, steps, steps - 1, fa.cap)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _fused64(ec, frag, ec.obs.data_ptr(), u, fc, stream=torch.cuda.current_stream().cuda_stream, fn=FN)
    for _ in range(2):
        ec.state.copy_(snap)
        fc.restore()
        g.replay()
        torch.cuda.synchronize()
        _compare(fc, fa)
        fc.guards_intact()
        _same_env(ec, ea)


@pytest.mark.parametrize("B,E,other", ((16, 64, "lb_ppo_steps64"), (8, 6, "lb_ppo_steps")), ids=("e64", "e6"))
def test_narrower_shapes_equal_the_narrower_entry_points(B, E, other):
    """On a shape lb_ppo_steps64 (lb_ppo_steps) supports, lb_ppo_steps256 runs its kernel: the same bits."""
    ea, eb, fa, fb, _, _ = _run_pair(B, E, True, 3, 7, other=other)
    assert getattr(ea, other[3:] + "_supported")(fa.R) and ea.ppo_steps64_supported(fa.R)
    _compare(fa, fb)
    fa.guards_intact()
    fa.written()
    _same_env(ea, eb)


def test_vec_env_ppo_steps256_argument_checks():
    env = _env(4, 180, True, 3)
    frag = _frag(env)
    B, R, T = 4, 181, 4
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda")
    good = dict(frag=frag, obs=env.obs, uniforms=z(T, B), actions_f32=z(T, B), logprobs=z(T, B), values=z(T, B),
                rewards=z(T, B), obs_next=z(T - 1, B, R, 8), dones_next=z(T - 1, B), last_obs=z(B, R, 8), last_done=z(B),
                actions=z(B, dt=torch.int32), dones=z(B, dt=torch.uint8), ep_sum=z(B, dt=torch.float64),
                ep_cnt=z(B, dt=torch.float64))
    env.ppo_steps256(**good)
    with pytest.raises(RuntimeError, match="ppo_steps64: .*ppo_steps64_supported"):
        env.ppo_steps64(**good)  # (the narrower entry points keep refusing the shape)
    with pytest.raises(RuntimeError, match="ppo_steps: .*ppo_steps_supported"):
        env.ppo_steps(**good)
    for kw in (dict(values=z(T, B, dt=torch.float64)), dict(rewards=z(B, T).t()), dict(logprobs=z(T, B + 1)),
               dict(actions=z(B, dt=torch.int64)), dict(last_obs=None), dict(obs_next=z(T - 2, B, R, 8)),
               dict(dones_next=z(T, B)), dict(ep_sum=z(B)), dict(uniforms=z(T, B).cpu()), dict(obs=z(B, R, 4))):
        with pytest.raises(ValueError, match="ppo_steps256:"):
            env.ppo_steps256(**dict(good, **kw))
    torch.cuda.synchronize()


# ---- the learner ----------------------------------------------------------------------------------
E80 = dict(num_endpoints=80, rejection_allowed=False, episode_length=2, reward_function="multi", latency_weight=1.0,
           cpu_weight=0.0, gini_weight=0.0)


def _learn_twice(monkeypatch, flags, B, T, monitor_file, want_rollout):
    """Two rollout() + update() rounds on a seeded env and agent, under a counting clock (the
    monitor file's time column is the host time of each step)."""
    from lbk8s import LBVecEnv, ppo, vec_env
    ticks = iter(range(1, 1 << 20))
    monkeypatch.setattr(vec_env, "time", types.SimpleNamespace(time=lambda: float(next(ticks))))
    env = LBVecEnv(B, seed=3, as_tensors=True, monitor_file=monitor_file, **E80)
    algo = ppo.PPO_DeepSets(env, num_steps=T, n_minibatches=4, update_epochs=1, seed=2, use_graphs=False, **flags)
    assert algo.fused_rollout is want_rollout and algo.fused_rollout_e256 is want_rollout and algo.fused_bookkeeping
    assert not algo.fused_rollout_e64
    next_obs = env.reset()
    next_done = torch.zeros(B, device="cuda")
    for _ in range(2):
        next_obs, next_done = algo.rollout(next_obs, next_done)
        algo.update(next_obs, next_done)
    torch.cuda.synchronize()
    out = {k: getattr(algo, k).detach().cpu().numpy().copy()
           for k in ("obs", "actions", "logprobs", "rewards", "dones", "values", "advantages", "returns")}
    params = [p.detach().cpu().numpy().copy() for p in algo.agent.parameters()]
    env.close()
    return out, params, open(env._monitor.path, "rb").read(), list(algo.episode_returns)


def test_fused_rollout_e256_learner_matches_three_launches(monkeypatch, tmp_path):
    """PPO_DeepSets(fused_rollout_e256=True) at 16 envs of 80 endpoints: the one-launch rollout is on
    and after two updates leaves the parameters, the storage and the monitor rows of the
    three-launch learner."""
    B, T = 16, 4
    runs = []
    for i, fl in enumerate((THREE, dict(THREE, fused_rollout_e256=True))):
        with monkeypatch.context() as mp:
            runs.append(_learn_twice(mp, fl, B, T, str(tmp_path / f"run{i}"), i == 1))
    (a, pa, csv_a, ret_a), (b, pb, csv_b, ret_b) = runs
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a["dones"][1:].sum() > 0 and np.isfinite(b["advantages"]).all()
    assert len(pa) == len(pb) > 0
    for x, y in zip(pa, pb):
        assert np.array_equal(x, y)
    assert ret_a == ret_b and len(ret_b) == 2
    assert csv_a == csv_b and csv_a.count(b"\n") > 2  # (the header's two lines, then the episodes' rows)
