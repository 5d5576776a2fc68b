"""lb_eval_steps256 (csrc/lbk8s_steps256.h): a greedy evaluation's vector steps in ONE launch for envs
of 65 to 256 endpoints == steps x (lb_ds_q_argmax, lb_step, lb_ppo_record), bit for bit, through the
C ABI.  The yardstick is the three existing launches, as in tests/test_gpu_eval_steps.py, whose
buffers (NaN / sentinel filled, 64 guard elements), envs out of phase, seeded images, random masks
and checks are used here as they are: obs, the three trace buffers, actions / reward / done,
ep_stats, ep_sum / ep_cnt, ret32 / ep_r32, the sorted log rows and the whole state blob; what the
header says is unwritten keeps its fill.

Shapes (R rows: E endpoints, +1 with the reject row), each at B = 3 (fewer envs than a block's
waves) and B = 67:
    R = 66   EPL = 2, the forward of 5 set tiles, one live lane pair past 64
    R = 80   the last size of that forward
    R = 81   the first chunked size: 3 chunks, 17 rows in the last
    R = 96   whole chunks;  R = 97
    R = 128  EPL = 2 full;  R = 129: the reject row alone in chunk 5
    R = 130  EPL = 4 first
    R = 193  both sides of a 64-row slot
    R = 256, R = 257
8 steps at episode length 3, so every env ends at least twice inside a launch.
"""
import ctypes as C

import pytest
import torch

from test_gpu_eval_steps import (TRACES, Bufs, _check_pair, _compare, _env, _frag, _log_args, _masks, _ptr, _row, _same,
                                 _same_env, _three)

pytestmark = pytest.mark.gpu

L3 = 3      # episode length
STEPS = 8


def _fused256(env, frag, b, masks, steps=None, step0=0, tag0=3, traces=TRACES, with_log=True, with_sums=True,
              stream=None, fn="lb_eval_steps256"):
    """lb_eval_steps256 (fn) of the steps step0 .. step0 + steps - 1 of b's sequence."""
    from lbk8s import _native
    B, R = b.B, b.R
    steps = b.steps if steps is None else steps
    tr = [_row(getattr(b, k), step0, B) if k in traces else None for k in TRACES]
    _native.check(getattr(_native.lib(), fn)(
        frag.data_ptr(), b.obs.data_ptr(), env.state.data_ptr(), C.byref(env._c), B, R, _ptr(masks), steps, *tr,
        b.actions_out.data_ptr(), b.reward_out.data_ptr(), b.done_out.data_ptr(), b.ep_stats.data_ptr(),
        _ptr(b.ep_sum) if with_sums else None, _ptr(b.ep_cnt) if with_sums else None,
        *_log_args(b, with_log, tag0 + step0), stream))


def _run_pair(B, E, rej, steps, L=L3, auto=True, masks=False, kind="dqn", cap=None, **opt):
    ea, eb = _env(B, E, rej, L, auto), _env(B, E, rej, L, auto)
    assert torch.equal(ea.state, eb.state) and torch.equal(ea.obs, eb.obs)
    R = ea.cfg.obs_rows
    assert ea.eval_steps256_supported(R)
    frag = _frag(kind)
    m = _masks(B, R) if masks else None
    cap = 4 * B if cap is None else cap
    fa, fb = Bufs(ea, steps, cap), Bufs(eb, steps, cap)
    _fused256(ea, frag, fa, m, **opt)
    _three(eb, frag, fb, m, **opt)
    torch.cuda.synchronize()
    return ea, eb, fa, fb, frag, m


# R: (E, rejection)
SHAPES = {66: (65, True), 80: (80, False), 81: (80, True), 96: (96, False), 97: (96, True), 128: (128, False),
          129: (128, True), 130: (129, True), 193: (192, True), 256: (256, False), 257: (256, True)}

# name: (B, R, steps, options)
CASES = {}
for _i, _R in enumerate(SHAPES):
    CASES[f"r{_R:03d}_b03"] = (3, _R, STEPS, dict(masks=_i % 2 == 0, kind="ppo" if _i % 3 == 0 else "dqn"))
    CASES[f"r{_R:03d}_b67"] = (67, _R, STEPS, dict(masks=_i % 2 == 1, kind="dqn" if _i % 3 == 0 else "ppo"))
CASES.update({
    "r066_no_reset": (5, 66, L3, dict(auto=False, masks=True)),
    "r081_no_reset": (5, 81, L3, dict(auto=False, kind="ppo")),
    "r257_no_reset": (5, 257, L3, dict(auto=False, masks=True)),
    "r080_no_log": (9, 80, STEPS, dict(with_log=False, masks=True)),
    "r129_no_log_no_sums_no_traces": (9, 129, STEPS, dict(with_log=False, with_sums=False, traces=())),
    "r193_no_traces": (9, 193, STEPS, dict(traces=(), masks=True)),
    "r066_actions_alone": (9, 66, STEPS, dict(traces=("actions_all",))),
    "r130_dones_alone": (9, 130, STEPS, dict(traces=("dones_all",), masks=True)),
    "r081_one_step": (1, 81, 1, {}),
})


@pytest.mark.parametrize("name", sorted(CASES))
def test_eval_steps256_equals_three_launches(name):
    B, R, steps, opt = CASES[name]
    E, rej = SHAPES[R]
    ea, eb, fa, fb, _, m = _run_pair(B, E, rej, steps, **opt)
    assert fa.R == R and not ea.eval_steps64_supported(R)  # a shape of the new kernels
    _check_pair(ea, eb, fa, fb, m, steps, L=L3, **opt)
    if opt.get("with_sums", True) and opt.get("auto", True) and steps == STEPS:
        ended = fa.ep_cnt[:B] - fa.init["ep_cnt"][:B]
        assert ended.min().item() >= 2  # every env ended at least twice inside the launch


def test_more_envs_than_resident_waves():
    """R = 81 with 8 CUs + 5 envs: a wave takes a second env after its first."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B, steps = 8 * cus + 5, 3
    ea, eb, fa, fb, _, m = _run_pair(B, 80, True, steps, masks=True)
    _check_pair(ea, eb, fa, fb, m, steps, L=L3, masks=True)


@pytest.mark.parametrize("R", (80, 129, 257))
def test_two_launches_equal_one(R):
    """3 + 5 steps == 8 steps: the state, the observations, ret32 and the sums carry across
    launches."""
    E, rej = SHAPES[R]
    B = 11
    ea, eb, fa, fb, frag, m = _run_pair(B, E, rej, STEPS, masks=True)
    _compare(fa, fb)
    ec = _env(B, E, rej, L3)
    fc = Bufs(ec, STEPS, fa.cap)
    _fused256(ec, frag, fc, m, steps=3, step0=0)
    _fused256(ec, frag, fc, m, steps=5, step0=3)
    torch.cuda.synchronize()
    _compare(fc, fa)
    fc.guards_intact()
    _same_env(ec, ea)


def test_graph_replay_writes_the_same_bits():
    """The launch captured in a graph (one kernel node) and replayed once == the eager launch."""
    B, (E, rej) = 11, SHAPES[193]
    ea, eb, fa, fb, frag, m = _run_pair(B, E, rej, STEPS, masks=True)
    _compare(fa, fb)
    ec = _env(B, E, rej, L3)
    snap = ec.state.clone()
    fc = Bufs(ec, STEPS, fa.cap)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _fused256(ec, frag, fc, m, stream=torch.cuda.current_stream().cuda_stream)
    ec.state.copy_(snap)
    fc.restore()
    g.replay()
    torch.cuda.synchronize()
    _compare(fc, fa)
    fc.guards_intact()
    _same_env(ec, ea)


@pytest.mark.parametrize("E,fn", ((64, "lb_eval_steps64"), (8, "lb_eval_steps")))
def test_older_shape_is_handed_on(E, fn):
    """At R = 65 lb_eval_steps256 equals lb_eval_steps64, at R = 9 lb_eval_steps: the same kernels,
    the same bits."""
    B, rej = 8, True
    ea, eb = _env(B, E, rej, L3), _env(B, E, rej, L3)
    R = ea.cfg.obs_rows
    assert R == E + 1 and ea.eval_steps256_supported(R) and ea.eval_steps64_supported(R)
    assert ea.eval_steps_supported(R) == (fn == "lb_eval_steps")
    frag, m = _frag("dqn"), _masks(B, R)
    fa, fb = Bufs(ea, STEPS, 4 * B), Bufs(eb, STEPS, 4 * B)
    _fused256(ea, frag, fa, m)
    _fused256(eb, frag, fb, m, fn=fn)
    torch.cuda.synchronize()
    _compare(fa, fb)
    fa.guards_intact()
    fa.written()
    _same_env(ea, eb)


def test_vec_env_eval_steps256_matches_the_abi_and_checks_its_arguments():
    """LBVecEnv.eval_steps256 writes the env's own buffers and the caller's trace as the C call does."""
    B, (E, rej) = 9, SHAPES[130]
    ea, eb, fa, fb, frag, m = _run_pair(B, E, rej, STEPS, masks=True, with_log=False)
    env = _env(B, E, rej, L3)
    R = env.cfg.obs_rows
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda")
    good = dict(frag=frag, obs=env.obs, steps=STEPS, masks=m.bool(), actions_all=z(STEPS, B, dt=torch.int32),
                rewards_all=z(STEPS, B), dones_all=z(STEPS, B, dt=torch.uint8), ep_sum=z(B, dt=torch.float64),
                ep_cnt=z(B, dt=torch.float64))
    for kw in (dict(actions_all=z(STEPS, B, dt=torch.int64)), dict(masks=m), dict(ep_sum=None), dict(obs=z(B, R, 4)),
               dict(steps=0)):
        with pytest.raises(ValueError, match="eval_steps256:"):
            env.eval_steps256(**dict(good, **kw))
    with pytest.raises(RuntimeError, match="eval_steps64: .*eval_steps64_supported"):
        env.eval_steps64(**good)  # (the older entry point keeps refusing the shape)
    assert torch.equal(env.state, _env(B, E, rej, L3).state)  # a refused call launched nothing
    assert env.eval_steps256(**good) is env.obs
    torch.cuda.synchronize()
    assert _same(env.obs.reshape(-1), fa.obs[:B * R * 8])
    assert torch.equal(good["actions_all"].reshape(-1), fa.actions_all[:STEPS * B])
    assert _same(good["rewards_all"].reshape(-1), fa.rewards_all[:STEPS * B])
    assert torch.equal(good["dones_all"].reshape(-1), fa.dones_all[:STEPS * B])
    assert torch.equal(env.actions, fa.actions_out[:B]) and _same(env.rewards, fa.reward_out[:B])
    assert torch.equal(env.dones, fa.done_out[:B])
    _same_env(env, ea)
