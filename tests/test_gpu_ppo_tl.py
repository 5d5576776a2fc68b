"""PPO's value targets that bootstrap from the terminal state at a time limit, on the GPU
(include/lbk8s_abi_ppo_tl.h):

* lb_gae_tl against the segment-wise float32 reference (tests/ppo_tl_ref.py) and, with zero
  term_values, against lb_gae;
* lb_ds_value_where against lb_ds_forward's value on the same batch with finite rows, the unflagged
  sets' rows NaN: every forward variant (the in-register tile counts, the 33..80 VALU image, the
  chunked kernel), and batches at which a wave takes two and four sets;
* lb_ppo_steps_tl against the per-step launch sequence it is defined by -- lb_ds_sample, lb_step
  with terminal_obs, lb_ppo_record, lb_ds_value_where -- and, in everything but term_values and
  terminal_obs, against lb_ppo_steps on a twin env;
* PPO_DeepSets(bootstrap_timeouts=True): the one-launch path against the per-step path.

Every output buffer starts as NaN with guard elements past its end, as tests/test_gpu_ppo_steps.py,
whose helpers these are.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import ppo_tl_ref as tl
from test_gpu_ppo_steps import PAD, Bufs, _bits, _compare, _frag, _fused, _log_args, _nan, _ptr, _row, _same, _same_env, \
    _uniforms

pytestmark = pytest.mark.gpu


# ---- lb_gae_tl ------------------------------------------------------------------------------------
def _gae_gpu(fn_name):
    from lbk8s import ppo

    def run(rewards, values, dones, next_value, next_done, term_values, gamma, lam):
        T, B = rewards.shape
        cu = lambda x: torch.from_numpy(x.copy()).cuda()
        adv, ret = _nan(T * B), _nan(T * B)
        out = (adv[:T * B].view(T, B), ret[:T * B].view(T, B))
        if fn_name == "lb_gae_tl":
            ppo.gae_tl_device(cu(rewards), cu(values), cu(dones), cu(next_value).view(1, B), cu(next_done),
                              cu(term_values), gamma, lam, out=out)
        else:
            ppo.gae_device(cu(rewards), cu(values), cu(dones), cu(next_value).view(1, B), cu(next_done), gamma, lam,
                           out=out)
        torch.cuda.synchronize()
        assert torch.isnan(adv[T * B:]).all() and torch.isnan(ret[T * B:]).all()  # the guards
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    return run


@pytest.mark.parametrize("T,B", ((1, 1), (5, 67), (12, 130)))
def test_gae_tl_equals_the_segment_reference(T, B):
    case = tl.make_case(T, B, seed=100 * T + B)
    tl.check_gae_tl(_gae_gpu("lb_gae_tl"), case)
    zero = dict(case, term_values=np.zeros((T, B), np.float32))
    args = [zero[k] for k in tl.ORDER] + [tl.GAMMA, tl.LAMBDA]
    new, old = _gae_gpu("lb_gae_tl")(*args), _gae_gpu("lb_gae")(*args)
    for a, b in zip(new, old):
        assert np.array_equal(tl.bits(a), tl.bits(b))
    quiet = tl.make_case(T, B, seed=9, no_done=True)  # no done anywhere: term_values has no effect
    args = [quiet[k] for k in tl.ORDER] + [tl.GAMMA, tl.LAMBDA]
    new, old = _gae_gpu("lb_gae_tl")(*args), _gae_gpu("lb_gae")(*args)
    for a, b in zip(new, old):
        assert np.array_equal(tl.bits(a), tl.bits(b))


def test_gae_tl_device_refuses_misshaped_tensors():
    """gae_tl_device's own list of checked tensors, term_values and out among them (on the CPU the
    device refusal comes first: tests/test_ppo_tl_host.py)."""
    from lbk8s.ppo import gae_tl_device
    T, B = 4, 6
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda")
    good = dict(rewards=z(T, B), values=z(T, B), dones=z(T, B), next_value=z(1, B), next_done=z(B), term_values=z(T, B),
                gamma=0.95, gae_lambda=0.97, out=(z(T, B), z(T, B)))
    adv, ret = gae_tl_device(**good)
    assert adv is good["out"][0] and ret is good["out"][1]
    for name, bad in (("term_values", z(T, B + 1)), ("term_values", z(T - 1, B)), ("term_values", z(B, T).t()),
                      ("term_values", z(T, B, dt=torch.float64)), ("term_values", z(T, B).cpu()), ("term_values", None),
                      ("values", z(T, B + 1)), ("dones", z(T * B)), ("next_value", z(B + 1)), ("next_done", z(1, B + 1)),
                      ("out", (z(T, B + 1), z(T, B))), ("out", (z(T, B), z(T, B, dt=torch.float64))),
                      ("out", (z(T, B), z(B, T).t()))):
        with pytest.raises(ValueError, match="gae_tl_device: " + ("out" if name == "out" else name)):
            gae_tl_device(**dict(good, **{name: bad}))
    torch.cuda.synchronize()


# ---- lb_ds_value_where ----------------------------------------------------------------------------
_agent = {}


def _critic():
    """One seeded DeepSetAgent (its weights do not depend on the set's size) and its weight image."""
    from lbk8s import LBVecEnv, fused
    from lbk8s.deepsets import DeepSetAgent
    if not _agent:
        torch.manual_seed(5)
        agent = DeepSetAgent(LBVecEnv(1, as_tensors=True)).cuda()
        _agent["a"] = (agent, fused.packed(agent, agent.actor.net, agent.critic).clone())
    return _agent["a"]


def _value_where_case(B, R):
    from lbk8s import _native
    L = _native.lib()
    agent, frag = _critic()
    g = torch.Generator().manual_seed(1000 * R + B)
    x = torch.randn((B, R, 8), generator=g).cuda()
    want = _nan(B)
    _native.check(L.lb_ds_forward(frag.data_ptr(), x.data_ptr(), B, R, None, want.data_ptr(), None))
    env = torch.arange(B, device="cuda")
    patterns = {"none": env < 0, "all": env >= 0, "every_third": env % 3 == 0}
    if R <= 16:  # one env of each pair: a group of two sets is half flagged
        patterns.update(even_of_pair=env % 2 == 0, odd_of_pair=env % 2 == 1)
    for name, flag in patterns.items():
        xn = torch.where(flag.view(B, 1, 1), x, torch.full_like(x, float("nan")))
        out = _nan(B)
        flags = flag.to(torch.uint8).contiguous()
        _native.check(L.lb_ds_value_where(frag.data_ptr(), xn.data_ptr(), flags.data_ptr(), B, R, out.data_ptr(), None))
        torch.cuda.synchronize()
        assert torch.isnan(out[B:]).all(), name
        got, ref = _bits(out[:B]), _bits(want[:B])
        assert torch.equal(got[flag], ref[flag]), (name, B, R)
        assert (got[~flag] == 0).all(), (name, B, R)  # exactly +0.0
        assert not torch.isnan(out[:B]).any()


@pytest.mark.parametrize("B", (1, 67, 300))
@pytest.mark.parametrize("R", (7, 9, 16, 17, 33, 65, 80, 81, 257))
def test_value_where_equals_forward_on_flagged_sets(R, B):
    _value_where_case(B, R)


@pytest.mark.parametrize("R,P", ((9, 2), (9, 4), (17, 2)))
def test_value_where_with_several_sets_per_wave(R, P):
    """The batches at which lb_ds_forward takes P sets per wave iteration on this device (so a wave's
    group can be partly flagged in lb_ds_value_where itself), ragged by one set."""
    from lbk8s import fused
    simds = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    B = P * simds + 1
    ts = (R + 15) // 16
    assert fused.forward_kernel(fused.FWD, B, R)[:2] == (ts, P)
    _value_where_case(B, R)


def test_value_where_wrapper():
    from lbk8s import fused
    agent, _ = _critic()
    B, R = 10, 9
    x = torch.randn((B, R, 8), generator=torch.Generator().manual_seed(1)).cuda()
    _, value = fused.deepsets_forward(agent, x, require=True)
    flag = torch.arange(B, device="cuda") % 2 == 0
    out = torch.full((B,), float("nan"), device="cuda")
    x[~flag] = float("nan")
    assert fused.deepsets_value_where(agent, x, flag, out) is out
    assert torch.equal(_bits(out), _bits(torch.where(flag, value, torch.zeros_like(value))))
    for kw in (dict(flags=flag.float()), dict(flags=flag[:-1]), dict(out=out.double()), dict(out=out[:-1]),
               dict(flags=flag.cpu())):
        with pytest.raises(ValueError, match="deepsets_value_where"):
            fused.deepsets_value_where(**dict(dict(agent=agent, x=x, flags=flag, out=out), **kw))


# ---- lb_ppo_steps_tl ------------------------------------------------------------------------------
B_TL, L_TL, STEPS_TL = 37, 5, 12


def _env_tl(E, rej, reward, **scenario):
    """A reset env whose envs are out of phase inside every group of two: two plain steps, then the
    odd envs start over."""
    from lbk8s import LBVecEnv
    env = LBVecEnv(B_TL, seed=11, as_tensors=True, num_endpoints=E, rejection_allowed=rej, episode_length=L_TL,
                   reward_function=reward, **scenario)
    env.reset()
    env.step_device(None)
    env.step_device(None)
    env.reset_masked((torch.arange(B_TL, device="cuda") % 2).to(torch.uint8))
    return env


class TLBufs(Bufs):
    def __init__(self, B, R, steps, S, cap):
        super().__init__(B, R, steps, S, cap)
        self.term_values = _nan(steps * B)
        self.terminal_obs = _nan(B * R * 8)


def _tl_fused(env, frag, b, u, with_log):
    from lbk8s import _native
    B, R = b.B, b.R
    _native.check(_native.lib().lb_ppo_steps_tl(
        frag.data_ptr(), env.obs.data_ptr(), env.state.data_ptr(), C.byref(env._c), B, R, b.steps, b.S, u.data_ptr(),
        b.actions_f32.data_ptr(), b.logprobs.data_ptr(), b.values.data_ptr(), b.rewards.data_ptr(),
        b.obs_next.data_ptr(), b.dones_next.data_ptr(), _ptr(b.last_obs), _ptr(b.last_done),
        b.actions_out.data_ptr(), b.done_out.data_ptr(), b.ep_stats.data_ptr(), b.ep_sum.data_ptr(),
        b.ep_cnt.data_ptr(), *_log_args(b, with_log, 0), b.terminal_obs.data_ptr(), b.term_values.data_ptr(), None))


def _tl_sequence(env, frag, b, u, with_log):
    """The definition: steps x (lb_ds_sample, lb_step with terminal_obs, lb_ppo_record,
    lb_ds_value_where)."""
    from lbk8s import _native
    L = _native.lib()
    B, R = b.B, b.R
    cfg, state = C.byref(env._c), env.state.data_ptr()
    obs = env.obs.data_ptr()
    for i in range(b.steps):
        stored = i < b.S
        nobs = _row(b.obs_next, i, B * R * 8) if stored else b.last_obs.data_ptr()
        ndone = _row(b.dones_next, i, B) if stored else b.last_done.data_ptr()
        _native.check(L.lb_ds_sample(frag.data_ptr(), obs, B, R, None, _row(u, i, B), None, b.actions_out.data_ptr(),
                                     _row(b.actions_f32, i, B), _row(b.logprobs, i, B), _row(b.values, i, B), None))
        _native.check(L.lb_step(state, cfg, B, b.actions_out.data_ptr(), nobs, _row(b.rewards, i, B),
                                b.done_out.data_ptr(), b.terminal_obs.data_ptr(), b.ep_stats.data_ptr(), None, None))
        lg = _log_args(b, with_log, i)
        _native.check(L.lb_ppo_record(B, b.done_out.data_ptr(), b.ep_stats.data_ptr(), ndone, b.ep_sum.data_ptr(),
                                      b.ep_cnt.data_ptr(), _row(b.rewards, i, B) if with_log else None,
                                      env._rew64 if with_log else None, b.actions_out.data_ptr() if with_log else None,
                                      lg[0], lg[1], lg[2], lg[3], lg[4], lg[5], None))
        _native.check(L.lb_ds_value_where(frag.data_ptr(), b.terminal_obs.data_ptr(), b.done_out.data_ptr(), B, R,
                                          _row(b.term_values, i, B), None))
        obs = nobs


# e6: config 1's shape (N = 48, Z = 12, R = 7: the 12-zone state layout)
TL_CASES = {"e6": (6, True, "naive", dict(num_nodes=48, num_zones=12)), "e8_multi": (8, True, "multi", {}),
            "e16_no_reject": (16, False, "multi", {})}


@pytest.mark.parametrize("S", (STEPS_TL, STEPS_TL - 1))
@pytest.mark.parametrize("name", sorted(TL_CASES))
def test_ppo_steps_tl_equals_its_launch_sequence(name, S):
    E, rej, reward, scenario = TL_CASES[name]
    with_log = name == "e8_multi"  # (one env's cases run with the episode log on)
    B, steps = B_TL, STEPS_TL
    ea, eb, ec = (_env_tl(E, rej, reward, **scenario) for _ in range(3))
    assert all((e.cfg.num_nodes, e.cfg.num_zones) == (scenario.get("num_nodes", 24), scenario.get("num_zones", 4))
               for e in (ea, eb, ec))
    assert torch.equal(ea.state, eb.state) and torch.equal(ea.obs, eb.obs)
    R = ea.cfg.obs_rows
    assert R == E + int(rej) and ea.ppo_steps_tl_supported(R) and ea.ppo_steps_supported(R)
    frag = _frag(ea)
    u = _uniforms(steps, B)
    cap = 4 * B
    fa, fb, fc = TLBufs(B, R, steps, S, cap), TLBufs(B, R, steps, S, cap), Bufs(B, R, steps, S, cap)
    _tl_fused(ea, frag, fa, u, with_log)
    _tl_sequence(eb, frag, fb, u, with_log)
    _fused(ec, frag, ec.obs.data_ptr(), u, fc, with_log=with_log)  # lb_ppo_steps on the twin
    torch.cuda.synchronize()
    for other in (fb, fc):
        _compare(fa, other, cap_all=with_log)
    for k in ("term_values", "terminal_obs"):
        assert _same(getattr(fa, k), getattr(fb, k)), k
    fa.guards_intact()
    fa.written(with_log=with_log)
    n = steps * B
    assert torch.isnan(fa.term_values[n:]).all() and torch.isnan(fa.terminal_obs[B * R * 8:]).all()
    _same_env(ea, eb)
    _same_env(ea, ec)
    # every env finished at least twice, out of phase inside its group; the terminal values stand
    # where the done rows say, +0.0 elsewhere
    ended = fa.ep_cnt[:B] - fa.init["ep_cnt"][:B]
    assert ended.min().item() >= 2
    done_after = torch.cat([fa.dones_next[:S * B], fa.last_done[:B]] if S < steps else [fa.dones_next[:S * B]])
    tv = fa.term_values[:n]
    assert not torch.isnan(tv).any() and not torch.isnan(fa.terminal_obs[:B * R * 8]).any()
    assert torch.equal(tv != 0, done_after != 0) and (_bits(tv)[done_after == 0] == 0).all()
    d = (done_after != 0).view(steps, B)
    assert (d[:, 0::2][:, :B // 2] != d[:, 1::2][:, :B // 2]).any()  # a group with one env finishing alone


# ---- the learner ----------------------------------------------------------------------------------
def _learner(flags, env_kw, B, T, updates=2):
    from lbk8s import LBVecEnv, ppo
    env = LBVecEnv(B, seed=3, as_tensors=True, **env_kw)
    algo = ppo.PPO_DeepSets(env, num_steps=T, n_minibatches=4, update_epochs=1, seed=2, use_graphs=False,
                            bootstrap_timeouts=True, **flags)
    next_obs = env.reset()
    next_done = torch.zeros(B, device="cuda")
    out = []
    for _ in range(updates):
        next_obs, next_done = algo.rollout(next_obs, next_done)
        algo.update(next_obs, next_done)
        torch.cuda.synchronize()
        snap = {k: getattr(algo, k).detach().cpu().numpy().copy()
                for k in ("obs", "actions", "logprobs", "rewards", "dones", "values", "term_values", "advantages",
                          "returns")}
        snap["next_done"] = next_done.cpu().numpy().copy()
        snap["terminal_obs"] = env.terminal_obs.cpu().numpy().copy()
        out.append(snap)
    params = [p.detach().cpu().numpy().copy() for p in algo.agent.parameters()]
    env.close()
    return algo, out, params


def _term_values_stand_where_done(snap):
    after = np.concatenate([snap["dones"][1:], snap["next_done"][None]])
    assert np.array_equal(snap["term_values"] != 0, after == 1) and after.sum() > 0
    assert (snap["term_values"][after == 0].view(np.uint32) == 0).all()


def test_learner_one_launch_path_equals_per_step_path():
    env_kw = dict(num_endpoints=6, rejection_allowed=True, episode_length=5, reward_function="multi")
    a, runs_a, pa = _learner(dict(fused_rollout=True), env_kw, 8, 12)
    b, runs_b, pb = _learner(dict(fused_act=True, fused_bookkeeping=True), env_kw, 8, 12)
    assert a.bootstrap_timeouts and a.fused_rollout is True and a.fused_bookkeeping
    assert b.bootstrap_timeouts and b.fused_rollout is False and b.fused_act and b.fused_bookkeeping
    for ra, rb in zip(runs_a, runs_b):
        for k in ra:
            assert np.array_equal(ra[k].view(np.uint32), rb[k].view(np.uint32)), k
        _term_values_stand_where_done(ra)
        assert np.isfinite(ra["advantages"]).all()
    assert len(pa) == len(pb) and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(pa, pb))
    # the advantages are GAE-TL's of the storage (the reference needs next_value: the last step's
    # return minus its advantage is values[-1], so only the rows before the last are checked)
    s = runs_a[-1]
    T = s["rewards"].shape[0]
    want, _ = tl.gae_tl_ref(s["rewards"][:T - 1], s["values"][:T - 1], s["dones"][:T - 1], s["values"][T - 1],
                            s["dones"][T - 1], s["term_values"][:T - 1], a.gamma, a.gae_lambda)
    open_rows = np.cumsum(s["dones"][1:][::-1], axis=0)[::-1] > 0  # rows whose segment closes before the last step
    got = s["advantages"][:T - 1]
    assert open_rows.any() and np.array_equal(tl.bits(got)[open_rows], tl.bits(want)[open_rows])


def test_learner_torch_route_of_the_terminal_values(monkeypatch):
    """Where the fused forward does not cover the agent the per-step path takes torch:
    where(done, get_value(terminal_obs), 0), the unfinished envs' rows (NaN here) without effect."""
    from lbk8s import LBVecEnv, fused, ppo
    B = 8
    env = LBVecEnv(B, seed=3, as_tensors=True, num_endpoints=6, rejection_allowed=True, episode_length=5)
    on = ppo.PPO_DeepSets(env, num_steps=4, seed=2, use_graphs=False, bootstrap_timeouts=True)
    assert on._tv_fused is True
    monkeypatch.setattr(fused, "ENABLED", False)
    algo = ppo.PPO_DeepSets(env, num_steps=4, seed=2, use_graphs=False, bootstrap_timeouts=True, fused_rollout=True)
    assert algo._tv_fused is False and algo.fused_rollout is False and algo.bootstrap_timeouts
    monkeypatch.setattr(fused, "deepsets_value_where", lambda *a, **k: pytest.fail("the fused route was taken"))
    x = torch.randn((B, 7, 8), generator=torch.Generator().manual_seed(4)).cuda()
    done = torch.arange(B, device="cuda") % 3 == 0
    with torch.no_grad():
        want = torch.where(done, algo.agent.get_value(x).reshape(-1), torch.zeros(B, device="cuda"))
    env.terminal_obs.copy_(torch.where(done.view(B, 1, 1), x, torch.full_like(x, float("nan"))))
    algo._done_u8.copy_(done.to(torch.uint8))
    out = torch.full((B,), float("nan"), device="cuda")
    algo._terminal_values(out)
    assert torch.equal(_bits(out), _bits(want)) and (_bits(out)[~done] == 0).all() and (out[done] != 0).all()
    # and through a rollout: term_values stands where the done rows say
    next_obs, next_done = algo.rollout(env.reset(), torch.zeros(B, device="cuda"))
    algo.update(next_obs, next_done)
    torch.cuda.synchronize()
    assert torch.isfinite(algo.term_values).all() and torch.isfinite(algo.advantages).all()
    env.close()


def test_learner_e64_takes_the_per_step_path():
    """lb_ppo_steps64 has no terminal values: with the option on, fused_rollout_e64 reads False and
    the per-step path fills term_values (here through the torch policy step)."""
    env_kw = dict(num_endpoints=64, rejection_allowed=True, episode_length=2, reward_function="multi",
                  latency_weight=1.0, cpu_weight=0.0, gini_weight=0.0)
    algo, runs, _ = _learner(dict(fused_rollout_e64=True), env_kw, 16, 4, updates=1)
    assert algo.fused_rollout_e64 is False and algo.fused_rollout is False and algo.fused_rollout_e256 is False
    _term_values_stand_where_done(runs[0])
    assert np.isfinite(runs[0]["advantages"]).all() and np.isfinite(runs[0]["term_values"]).all()
    assert (runs[0]["next_done"] == 1).all()  # (episode_length 2, 4 steps: every env finished in the last step)
