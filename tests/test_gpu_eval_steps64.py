"""lb_eval_steps64 (csrc/lbk8s_steps64.h): a greedy evaluation's vector steps in ONE launch for envs
of up to 64 endpoints == steps x (lb_ds_q_argmax, lb_step, lb_ppo_record), bit for bit, through the
C ABI.  The yardstick is the three existing launches, as in tests/test_gpu_eval_steps.py, whose
buffers (NaN / sentinel filled, 64 guard elements), envs out of phase, seeded images, random masks
and checks are used here as they are.

Shapes: tests/test_gpu_ppo_steps64.py's list (every (W, TS) kernel, R = 17 on 16 lanes up to
R = 65, one env to more envs than resident waves); over it masks on and off, a DQN image and a PPO
actor's, auto-reset on and off, the trace buffers given and NULL.  Episode length 5 with 1, 4, 5
and 13 steps, as there.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_eval_steps import (L_EP, TRACES, Bufs, _check_pair, _compare, _env, _frag, _log_args, _masks, _ptr, _row,
                                 _same, _same_env, _three)

pytestmark = pytest.mark.gpu


def _fused64(env, frag, b, masks, steps=None, step0=0, tag0=3, traces=TRACES, with_log=True, with_sums=True,
             stream=None, fn="lb_eval_steps64"):
    """lb_eval_steps64 (fn) of the steps step0 .. step0 + steps - 1 of b's sequence."""
    from lbk8s import _native
    B, R = b.B, b.R
    steps = b.steps if steps is None else steps
    tr = [_row(getattr(b, k), step0, B) if k in traces else None for k in TRACES]
    _native.check(getattr(_native.lib(), fn)(
        frag.data_ptr(), b.obs.data_ptr(), env.state.data_ptr(), C.byref(env._c), B, R, _ptr(masks), steps, *tr,
        b.actions_out.data_ptr(), b.reward_out.data_ptr(), b.done_out.data_ptr(), b.ep_stats.data_ptr(),
        _ptr(b.ep_sum) if with_sums else None, _ptr(b.ep_cnt) if with_sums else None,
        *_log_args(b, with_log, tag0 + step0), stream))


def _run_pair(B, E, rej, steps, L=L_EP, auto=True, masks=False, kind="dqn", cap=None, **opt):
    ea, eb = _env(B, E, rej, L, auto), _env(B, E, rej, L, auto)
    assert torch.equal(ea.state, eb.state) and torch.equal(ea.obs, eb.obs)
    R = ea.cfg.obs_rows
    assert ea.eval_steps64_supported(R)
    frag = _frag(kind)
    m = _masks(B, R) if masks else None
    cap = 4 * B if cap is None else cap
    fa, fb = Bufs(ea, steps, cap), Bufs(eb, steps, cap)
    _fused64(ea, frag, fa, m, **opt)
    _three(eb, frag, fb, m, **opt)
    torch.cuda.synchronize()
    return ea, eb, fa, fb, frag, m


# name: (B, E, rejection, steps, options); B as a string: a multiple of the CU count plus a rest
CASES = {
    "a_r17_w16": (67, 16, True, 13, dict(masks=True)),
    "a_r17_w16_ppo": (67, 16, True, 5, dict(kind="ppo")),
    "b_w32": (5, 17, False, 13, dict(masks=True, kind="ppo")),
    "c_r32": (67, 32, False, 5, dict(masks=True)),
    "c_r32_no_reset": (67, 32, False, L_EP, dict(auto=False, kind="ppo")),
    "d_r33_valu": (33, 32, True, 13, {}),
    "d_r33_valu_masks_ppo": (33, 32, True, 4, dict(masks=True, kind="ppo")),
    "e_w64": (9, 33, False, 13, dict(masks=True)),
    "f_r49_ts4": (19, 48, True, 13, dict(kind="ppo")),
    "f_r49_ts4_no_traces": (19, 48, True, 13, dict(traces=(), masks=True)),
    "g_r64": (17, 64, False, 5, dict(masks=True)),
    "g_r64_no_reset": (17, 64, False, L_EP, dict(auto=False, masks=True)),
    "h_r65": (16, 64, True, 13, dict(masks=True)),
    "h_r65_ppo": (16, 64, True, 13, dict(kind="ppo")),
    "h_r65_no_reset": (16, 64, True, L_EP, dict(auto=False)),
    "h_r65_actions_alone": (16, 64, True, 13, dict(traces=("actions_all",), masks=True)),
    "h_r65_dones_alone": (16, 64, True, 5, dict(traces=("dones_all",))),
    "h_r65_no_log": (16, 64, True, 13, dict(with_log=False, masks=True)),
    "h_r65_no_log_no_sums_no_traces": (16, 64, True, 13, dict(with_log=False, with_sums=False, traces=())),
    "i_one_step": (1, 64, True, 1, {}),
    "j_more_groups_than_waves": ("8c+3", 64, True, 5, dict(masks=True)),
    "k_two_per_wave": ("8c+1", 20, True, 5, dict(masks=True)),
    "k_one_per_wave": (130, 20, True, 13, dict(masks=True, kind="ppo")),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_eval_steps64_equals_three_launches(name):
    from lbk8s import fused
    B, E, rej, steps, opt = CASES[name]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if B == "8c+3":
        B = 8 * cus + 3
    elif B == "8c+1":
        # lb_ds_q_argmax itself takes two envs per wave here and one at 130: lb_eval_steps64's
        # forward (always one) must give either's bits
        B = 8 * cus + 1
        assert fused.forward_kernel(fused.FWD_ARGMAX, B, 21)[:2] == (2, 2)
        assert fused.forward_kernel(fused.FWD_ARGMAX, 130, 21)[:2] == (2, 1)
    ea, eb, fa, fb, _, m = _run_pair(B, E, rej, steps, **opt)
    assert not ea.eval_steps_supported(fa.R)  # a shape of the new kernels
    _check_pair(ea, eb, fa, fb, m, steps, **opt)
    if opt.get("with_sums", True) and opt.get("auto", True):
        ended = fa.ep_cnt[:B] - fa.init["ep_cnt"][:B]
        if steps == 13:
            assert ended.min().item() >= 2  # every env ended at least twice inside the launch
        elif steps == 1:
            assert ended.sum().item() == 0 and fa.rows().shape[0] == 0


def test_eval_steps64_full_log_counts_dropped_rows():
    """cap = half the finished episodes: *count is the full count, cap rows are stored, each a
    distinct row of the uncapped three-launch run."""
    B, E, rej, steps = 16, 64, True, 13
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


@pytest.mark.parametrize("B,E,rej", ((16, 64, True), (67, 32, False)))
def test_two_launches_equal_one(B, E, rej):
    """6 + 7 steps == 13 steps: the state, the observations, ret32 and the sums carry across
    launches."""
    steps = 13
    ea, eb, fa, fb, frag, m = _run_pair(B, E, rej, steps, masks=True)
    _compare(fa, fb)
    ec = _env(B, E, rej, L_EP)
    fc = Bufs(ec, steps, fa.cap)
    _fused64(ec, frag, fc, m, steps=6, step0=0)
    _fused64(ec, frag, fc, m, steps=7, step0=6)
    torch.cuda.synchronize()
    _compare(fc, fa)
    fc.guards_intact()
    _same_env(ec, ea)


def test_graph_replay_writes_the_same_bits():
    """The launch captured in a graph (one kernel node) and replayed once == the eager launch."""
    B, E, rej, steps = 16, 64, True, 13
    ea, eb, fa, fb, frag, m = _run_pair(B, E, rej, steps, masks=True)
    _compare(fa, fb)
    ec = _env(B, E, rej, L_EP)
    snap = ec.state.clone()
    fc = Bufs(ec, steps, fa.cap)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _fused64(ec, frag, fc, m, stream=torch.cuda.current_stream().cuda_stream)
    ec.state.copy_(snap)
    fc.restore()
    g.replay()
    torch.cuda.synchronize()
    _compare(fc, fa)
    fc.guards_intact()
    _same_env(ec, ea)


def test_16_lane_shape_equals_lb_eval_steps():
    """On a shape lb_eval_steps supports, lb_eval_steps64 runs its kernel: the same bits."""
    B, E, rej, steps = 8, 6, True, 13
    ea, eb = _env(B, E, rej, L_EP), _env(B, E, rej, L_EP)
    R = ea.cfg.obs_rows
    assert ea.eval_steps_supported(R) and ea.eval_steps64_supported(R)
    frag, m = _frag("dqn"), _masks(B, R)
    fa, fb = Bufs(ea, steps, 4 * B), Bufs(eb, steps, 4 * B)
    _fused64(ea, frag, fa, m)
    _fused64(eb, frag, fb, m, fn="lb_eval_steps")
    torch.cuda.synchronize()
    _compare(fa, fb)
    fa.guards_intact()
    fa.written()
    _same_env(ea, eb)


def test_vec_env_eval_steps64_matches_the_abi_and_checks_its_arguments():
    """LBVecEnv.eval_steps64 writes the env's own buffers and the caller's trace as the C call does."""
    B, E, rej, steps = 16, 64, True, 13
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
        with pytest.raises(ValueError, match="eval_steps64:"):
            env.eval_steps64(**dict(good, **kw))
    with pytest.raises(RuntimeError, match="eval_steps: .*eval_steps_supported"):
        env.eval_steps(**good)  # (the 16-lane entry point keeps refusing the shape)
    assert torch.equal(env.state, _env(B, E, rej, L_EP).state)  # a refused call launched nothing
    assert env.eval_steps64(**good) is env.obs
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
