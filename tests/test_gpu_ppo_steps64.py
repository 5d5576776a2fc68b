"""lb_ppo_steps64 (csrc/lbk8s_steps64.h): a PPO rollout's vector steps in ONE launch for envs of up
to 64 endpoints == steps x (lb_ds_sample, lb_step, lb_ppo_record), bit for bit, through the C ABI.
The yardstick is the three existing launches, as in tests/test_gpu_ppo_steps.py, whose buffers
(NaN / sentinel filled, 64 guard elements), envs out of phase, seeded agent image and comparisons
(the whole state blob; log rows sorted) are used here as they are.

Shapes: every (W, TS) kernel -- R = 17 on 16 lanes (one live row in tile 2), W = 32 at its first and
last R of two tiles and at R = 33 (the first VALU-image shape), W = 64 at TS = 3, 4, 5 up to config
4's R = 65 with envs that end several times inside the launch, a one-step launch in which nothing
ends, more envs than resident waves (the gi += nwaves loop, a ragged last block), and a batch at
which lb_ds_sample itself takes two envs per wave next to one where it takes one.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_ppo_steps import (E64, THREE, Bufs, _compare, _cus, _env, _frag, _learner_run, _log_args, _ptr, _row,
                                _same_env, _three, _uniforms)

pytestmark = pytest.mark.gpu


def _fused64(env, frag, obs, u, b, steps=None, S=None, step0=0, tag0=0, with_log=True, stream=None, fn="lb_ppo_steps64"):
    """lb_ppo_steps64 (fn) of the steps step0 .. step0 + steps - 1 of b's sequence."""
    from lbk8s import _native
    B, R = b.B, b.R
    steps = b.steps if steps is None else steps
    S = b.S - step0 if S is None else S
    _native.check(getattr(_native.lib(), fn)(
        frag.data_ptr(), obs, env.state.data_ptr(), C.byref(env._c), B, R, steps, S, _row(u, step0, B),
        _row(b.actions_f32, step0, B), _row(b.logprobs, step0, B), _row(b.values, step0, B), _row(b.rewards, step0, B),
        _row(b.obs_next, step0, B * R * 8), _row(b.dones_next, step0, B), _ptr(b.last_obs), _ptr(b.last_done),
        b.actions_out.data_ptr(), b.done_out.data_ptr(), b.ep_stats.data_ptr(), b.ep_sum.data_ptr(),
        b.ep_cnt.data_ptr(), *_log_args(b, with_log, tag0 + step0), stream))


def _run_pair(B, E, rej, L, steps, S=None, with_log=True, cap=None):
    S = steps - 1 if S is None else S
    ea, eb = _env(B, E, rej, L), _env(B, E, rej, L)
    assert torch.equal(ea.state, eb.state) and torch.equal(ea.obs, eb.obs)
    R = ea.cfg.obs_rows
    assert ea.ppo_steps64_supported(R)
    frag = _frag(ea)
    u = _uniforms(steps, B)
    cap = 3 * B if cap is None else cap
    fa, fb = Bufs(B, R, steps, S, cap), Bufs(B, R, steps, S, cap)
    _fused64(ea, frag, ea.obs.data_ptr(), u, fa, with_log=with_log)
    _three(eb, frag, eb.obs.data_ptr(), u, fb, with_log=with_log)
    torch.cuda.synchronize()
    return ea, eb, fa, fb, u, frag


# (B, E, reject, L, steps); B as a string: a multiple of the CU count plus a rest
CASES = {"a_r17_w16": (67, 16, True, 2, 5), "b_w32": (5, 17, False, 3, 7), "c_r32": (67, 32, False, 2, 5),
         "d_r33_valu": (33, 32, True, 2, 5), "e_w64": (9, 33, False, 3, 7), "f_r49_ts4": (19, 48, True, 2, 5),
         "g_r64": (17, 64, False, 2, 5), "h_r65_config4": (16, 64, True, 2, 9), "i_one_step": (1, 64, True, 100, 1),
         "j_more_groups_than_waves": ("8c+3", 64, True, 2, 3), "k_two_per_wave": ("8c+1", 20, True, 2, 3)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_ppo_steps64_equals_three_launches(name):
    from lbk8s import fused
    B, E, rej, L, steps = CASES[name]
    if B == "8c+3":
        B = 8 * _cus() + 3
    elif B == "8c+1":
        # lb_ds_sample itself takes two envs per wave here and one at 130: lb_ppo_steps64's forward
        # (always one) must give either's bits
        B = 8 * _cus() + 1
        assert fused.forward_kernel(fused.FWD_SAMPLE, B, 21)[:2] == (2, 2)
        assert fused.forward_kernel(fused.FWD_SAMPLE, 130, 21)[:2] == (2, 1)
    ea, eb, fa, fb, _, _ = _run_pair(B, E, rej, L, steps)
    assert not ea.ppo_steps_supported(fa.R)  # a shape of the new kernels
    _compare(fa, fb)
    fa.guards_intact()
    fa.written()
    _same_env(ea, eb)
    ended = fa.ep_cnt[:B] - fa.init["ep_cnt"][:B]
    assert int(fa.count[0].item()) == int(ended.sum().item())
    if L < steps:
        assert ended.max().item() >= 2  # an env ended twice inside the launch
        assert ended.min().item() >= 1
    elif name == "i_one_step":
        assert ended.sum().item() == 0 and fa.rows().shape[0] == 0
    if name == "h_r65_config4":
        assert ended.min().item() >= 4  # 9 steps of 2-step episodes


def test_two_per_wave_forward_at_130_envs():
    """Case k's other side: at 130 envs lb_ds_sample takes one env per wave at R = 21."""
    ea, eb, fa, fb, _, _ = _run_pair(130, 20, True, 2, 3)
    _compare(fa, fb)
    fa.guards_intact()
    _same_env(ea, eb)


def test_ppo_steps64_without_log_and_with_all_rows_stored():
    """log = NULL: ret32, ep_r32, the log and the counter are not touched; store_rows = steps: the
    last step's rows go to the storage too and last_* stay as they were."""
    B, E, rej, L, steps = CASES["h_r65_config4"]
    ea, eb, fa, fb, _, _ = _run_pair(B, E, rej, L, steps, S=steps, with_log=False)
    _compare(fa, fb)
    fa.guards_intact()
    fa.written(with_log=False)
    _same_env(ea, eb)
    assert (fa.ep_cnt[:B] - fa.init["ep_cnt"][:B]).max().item() >= 2


def test_ppo_steps64_full_log_counts_dropped_rows():
    """cap = half the finished episodes: *count is the full count, cap rows are stored, each a
    distinct row of the uncapped three-launch run."""
    B, E, rej, L, steps = CASES["h_r65_config4"]
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


@pytest.mark.parametrize("name", ("h_r65_config4", "c_r32"))
def test_two_launches_equal_one(name):
    """4 + 5 steps (store_rows = steps on the first: its last observations are the second's
    input) == 9 steps."""
    B, E, rej, L, _ = CASES[name]
    steps = 9
    ea, eb, fa, fb, u, frag = _run_pair(B, E, rej, L, steps)
    _compare(fa, fb)
    ec = _env(B, E, rej, L)
    fc = Bufs(B, fa.R, steps, steps - 1, fa.cap)
    _fused64(ec, frag, ec.obs.data_ptr(), u, fc, steps=4, S=4, step0=0)
    _fused64(ec, frag, _row(fc.obs_next, 3, B * fa.R * 8), u, fc, steps=5, S=4, step0=4)
    torch.cuda.synchronize()
    _compare(fc, fa)
    fc.guards_intact()
    _same_env(ec, ea)


def test_graph_replay_writes_the_same_bits():
    B, E, rej, L, steps = CASES["h_r65_config4"]
    ea, eb, fa, fb, u, frag = _run_pair(B, E, rej, L, steps)
    _compare(fa, fb)
    ec = _env(B, E, rej, L)
    snap = ec.state.clone()
    fc = Bufs(B, fa.R, steps, steps - 1, fa.cap)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _fused64(ec, frag, ec.obs.data_ptr(), u, fc, stream=torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        ec.state.copy_(snap)
        fc.restore()
        g.replay()
        torch.cuda.synchronize()
        _compare(fc, fa)
        fc.guards_intact()
        _same_env(ec, ea)


def test_16_lane_shape_equals_lb_ppo_steps():
    """On a shape lb_ppo_steps supports, lb_ppo_steps64 runs its kernel: the same bits."""
    B, E, rej, L, steps = 8, 6, True, 3, 7
    ea, eb = _env(B, E, rej, L), _env(B, E, rej, L)
    R = ea.cfg.obs_rows
    assert ea.ppo_steps_supported(R) and ea.ppo_steps64_supported(R)
    frag, u = _frag(ea), _uniforms(steps, B)
    fa, fb = Bufs(B, R, steps, steps - 1, 3 * B), Bufs(B, R, steps, steps - 1, 3 * B)
    _fused64(ea, frag, ea.obs.data_ptr(), u, fa)
    _fused64(eb, frag, eb.obs.data_ptr(), u, fb, fn="lb_ppo_steps")
    torch.cuda.synchronize()
    _compare(fa, fb)
    fa.guards_intact()
    fa.written()
    _same_env(ea, eb)


def test_vec_env_ppo_steps64_argument_checks():
    env = _env(4, 64, True, 3)
    frag = _frag(env)
    B, R, T = 4, 65, 4
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda")
    good = dict(frag=frag, obs=env.obs, uniforms=z(T, B), actions_f32=z(T, B), logprobs=z(T, B), values=z(T, B),
                rewards=z(T, B), obs_next=z(T - 1, B, R, 8), dones_next=z(T - 1, B), last_obs=z(B, R, 8), last_done=z(B),
                actions=z(B, dt=torch.int32), dones=z(B, dt=torch.uint8), ep_sum=z(B, dt=torch.float64),
                ep_cnt=z(B, dt=torch.float64))
    env.ppo_steps64(**good)
    with pytest.raises(RuntimeError, match="ppo_steps: .*ppo_steps_supported"):
        env.ppo_steps(**good)  # (the 16-lane entry point keeps refusing the shape)
    for kw in (dict(values=z(T, B, dt=torch.float64)), dict(rewards=z(B, T).t()), dict(logprobs=z(T, B + 1)),
               dict(actions=z(B, dt=torch.int64)), dict(last_obs=None), dict(obs_next=z(T - 2, B, R, 8)),
               dict(dones_next=z(T, B)), dict(ep_sum=z(B)), dict(uniforms=z(T, B).cpu()), dict(obs=z(B, R, 4))):
        with pytest.raises(ValueError, match="ppo_steps64:"):
            env.ppo_steps64(**dict(good, **kw))
    torch.cuda.synchronize()


def test_fused_rollout_e64_learner_matches_three_launches(monkeypatch, tmp_path):
    """PPO_DeepSets(fused_rollout_e64=True) at config 4's shape: the one-launch rollout is on and
    leaves the storage, advantages, returns, episode sums, episode_returns and monitor file of the
    three-launch learner (the mirror of test_fused_rollout_learner_matches_three_launches)."""
    B, T = 16, 4
    runs = []
    for i, fl in enumerate((THREE, dict(THREE, fused_rollout_e64=True))):
        with monkeypatch.context() as mp:
            runs.append(_learner_run(mp, fl, E64, B, T, str(tmp_path / f"run{i}"), i == 1))
    (a, csv_a, (sum_a, cnt_a), ret_a), (b, csv_b, (sum_b, cnt_b), ret_b) = runs
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a["dones"][1:].sum() > 0 and np.isfinite(b["advantages"]).all()
    assert sum_a.shape == sum_b.shape == (B,)
    assert np.array_equal(sum_a, sum_b) and np.array_equal(cnt_a, cnt_b) and cnt_b.sum() > 0
    assert ret_a == ret_b and len(ret_b) == 1
    assert csv_a == csv_b and csv_a.count(b"\n") == 2 + int(cnt_b.sum())
