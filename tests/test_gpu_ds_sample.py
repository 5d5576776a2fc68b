"""lb_ds_sample (k_deepsets_fwd<TS, P, 5>, k_deepsets_fwd_big<5>: the categorical sample fused into
the deep-sets forward) on the GPU, through tests/ds_sample_ref.py's cases and checker, and its
wiring up to PPO_DeepSets(fused_act=True).

Every output buffer carries padding and starts as NaN (actions: -7); the logits and the value
must equal the plain forward's bit for bit; every set's action must lie in its inverse-CDF
interval under the float64 softmax of the kernel's own logits (tests/ds_sample_ref.py has the
tolerances and their derivation).
"""
import copy

import numpy as np
import pytest
import torch

import ds_sample_ref as sr
from ds_sample_ref import MASK_KINDS, SAMPLE_CASES, case_id

pytestmark = pytest.mark.gpu


def on_device(s):
    from lbk8s import fused
    c = s.case
    assert fused.forward_kernel(fused.FWD_SAMPLE, s.B, c.R) == c.variant, case_id(c)
    assert fused.forward_kernel(fused.FWD, s.B, c.R) == c.variant, case_id(c)
    return copy.deepcopy(s.net).cuda(), s.x.cuda()


def image_of(net, heads):
    from lbk8s import fused
    return fused.packed(net, net.actor.net, net.critic) if heads == "ac" else fused.packed(net, net.q_network.net, None)


def launch(frag, x, masks, u, bufs):
    """lb_ds_sample through the C ABI into the padded buffers `bufs` (value None: actor only)."""
    from lbk8s import _native
    B, R, _ = x.shape

    def ptr(t):
        return None if t is None else t.data_ptr()
    _native.check(_native.lib().lb_ds_sample(frag.data_ptr(), x.data_ptr(), B, R, ptr(masks), u.data_ptr(),
                                             ptr(bufs["logits"]), bufs["actions"].data_ptr(), ptr(bufs["actions_f32"]),
                                             bufs["logprob"].data_ptr(), ptr(bufs["value"]),
                                             torch.cuda.current_stream().cuda_stream))


def plain_forward(net, x, heads):
    from lbk8s import fused
    if heads == "ac":
        logits, value = fused.deepsets_forward(net, x, require=True)
        return {"logits": logits.cpu().numpy(), "value": value.cpu().numpy()}
    return {"logits": fused.q_forward(net, x, require=True).cpu().numpy(), "value": None}


@pytest.mark.parametrize("c", SAMPLE_CASES, ids=case_id)
def test_sample(c):
    """Every case, without masks and with each mask kind; the last run twice (bit-equal) and
    once more without the optional outputs (the same actions and log-probabilities)."""
    s = sr.setup(c)
    net, x = on_device(s)
    B, R = s.B, c.R
    frag, u = image_of(net, c.heads), s.u.cuda()
    fwd = plain_forward(net, x, c.heads)
    out = {}
    for kind in MASK_KINDS:
        masks = sr.sample_masks(c, kind)
        md = None if masks is None else torch.from_numpy(masks).cuda()
        bufs = sr.alloc_outputs(B, R, c.heads, "cuda")
        launch(frag, x, md, u, bufs)
        got = sr.as_numpy(bufs)
        out[kind] = sr.check_sample(s, masks, s.u.numpy(), got, fwd=fwd)
        a = got["actions"][:B]
        if masks is not None and R > 1:
            assert a[9] == R - 1, a[9]  # (set 9: only row R - 1 valid)
        if masks is None and R % 2 == 0:
            assert a[3] in (R // 2 - 1, R // 2), a[3]  # (the uniform set, u = 0.5 on a boundary)
    print("ds-sample-margin", case_id(c), out)
    again = sr.alloc_outputs(B, R, c.heads, "cuda")
    launch(frag, x, md, u, again)
    for k, v in sr.as_numpy(again).items():
        assert v is None or np.array_equal(v, got[k], equal_nan=True), f"{case_id(c)}: {k} differs between two runs"
    lean = sr.alloc_outputs(B, R, c.heads, "cuda")
    launch(frag, x, md, u, dict(lean, logits=None, actions_f32=None))
    lean = sr.as_numpy(lean)
    assert np.array_equal(lean["actions"], got["actions"]) and np.array_equal(lean["logprob"], got["logprob"],
                                                                               equal_nan=True)
    assert np.isnan(lean["logits"]).all() and np.isnan(lean["actions_f32"]).all()


def _agent_case(R, bname):
    return next(c for c in SAMPLE_CASES if c.R == R and c.bname == bname and c.heads == "ac")


@pytest.mark.parametrize("R,bname", [(9, "B4"), (65, "B1")])
def test_storage_rows(R, bname):
    """fused.deepsets_sample writes rows [2] of (4, B) storage tensors; rows 1 and 3 stay NaN."""
    from lbk8s import fused
    s = sr.setup(_agent_case(R, bname))
    net, x = on_device(s)
    B, u = s.B, s.u.cuda()
    st = {k: torch.full((4, B), float("nan"), device="cuda") for k in ("actions_f32", "logprob", "value")}
    act = torch.full((4, B), -7, dtype=torch.int32, device="cuda")
    logits = torch.full((4, B, R), float("nan"), device="cuda")
    ret = fused.deepsets_sample(net, x, u, None, actions_out=act[2], logprob_out=st["logprob"][2],
                                value_out=st["value"][2], actions_f32_out=st["actions_f32"][2], logits_out=logits[2])
    assert ret[0].data_ptr() == act[2].data_ptr() and ret[1].data_ptr() == st["logprob"][2].data_ptr()
    for t in list(st.values()) + [logits]:
        assert torch.isnan(t[[0, 1, 3]]).all() and not torch.isnan(t[2]).any()
    assert (act[[0, 1, 3]] == -7).all()
    bufs = sr.alloc_outputs(B, R, "ac", "cuda")
    launch(image_of(net, "ac"), x, None, u, bufs)
    assert torch.equal(act[2], bufs["actions"][:B]) and torch.equal(st["logprob"][2], bufs["logprob"][:B])
    assert torch.equal(st["value"][2], bufs["value"][:B]) and torch.equal(logits[2].reshape(-1), bufs["logits"][:B * R])
    assert torch.equal(st["actions_f32"][2], act[2].float())
    # wrong dtype, shape or contiguity raises
    ok = dict(actions_out=act[2], logprob_out=st["logprob"][2], value_out=st["value"][2])
    for bad in (dict(actions_out=act[2].long()), dict(logprob_out=st["logprob"][2].double()),
                dict(value_out=st["value"][:, 0]), dict(logprob_out=st["logprob"][2, :B - 1]),
                dict(actions_f32_out=act[2]), dict(logits_out=logits[2, :, 0]), dict(value_out=None),
                dict(logprob_out=torch.empty((B, 2), device="cuda")[:, 0])):
        with pytest.raises(ValueError):
            fused.deepsets_sample(net, x, u, None, **dict(ok, **bad))
    with pytest.raises(ValueError):
        fused.deepsets_sample(net, x, u.double(), None, **ok)
    with pytest.raises(ValueError):
        fused.deepsets_sample(net, x, u, torch.ones((B, R), dtype=torch.uint8, device="cuda"), **ok)


def test_graph_replay():
    """One deepsets_sample call captured in a HIP graph; the uniforms buffer is rewritten and the
    graph replayed: the eager call's result on those uniforms."""
    from lbk8s import fused
    s = sr.setup(_agent_case(9, "B4"))
    net, x = on_device(s)
    B = s.B
    u = s.u.cuda().clone()
    masks = torch.from_numpy(sr.sample_masks(s.case, "equal")).cuda()

    def outs():
        return dict(actions_out=torch.full((B,), -7, dtype=torch.int32, device="cuda"),
                    logprob_out=torch.full((B,), float("nan"), device="cuda"),
                    value_out=torch.full((B,), float("nan"), device="cuda"))
    o = outs()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fused.deepsets_sample(net, x, u, masks, **o)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fused.deepsets_sample(net, x, u, masks, **o)
    first = o["actions_out"].clone()
    u2 = sr.sample_uniforms(B, 4242).cuda()
    u.copy_(u2)
    for t in o.values():
        t.fill_(-7 if t.dtype == torch.int32 else float("nan"))
    g.replay()
    e = outs()
    fused.deepsets_sample(net, x, u2, masks, **e)
    torch.cuda.synchronize()
    for k in o:
        assert torch.equal(o[k], e[k]), k
    assert not torch.equal(first, o["actions_out"])  # (other uniforms: other actions)


def _ppo(B, T, fused_act, **env_kw):
    from lbk8s import LBVecEnv
    from lbk8s.ppo import PPO_DeepSets
    env = LBVecEnv(B, seed=11, as_tensors=True, episode_length=10, **env_kw)
    algo = PPO_DeepSets(env, num_steps=T, n_minibatches=4, update_epochs=1, seed=5, fused_act=fused_act)
    next_obs = env.reset()
    if not isinstance(next_obs, torch.Tensor):
        next_obs = env.obs
    algo.rollout(next_obs, torch.zeros(B, device=algo.device))
    torch.cuda.synchronize()
    return algo


@pytest.mark.parametrize("B,T,R,env_kw", [(256, 8, 9, {}), (512, 4, 65, {"num_endpoints": 64})])
def test_ppo_fused_act(B, T, R, env_kw):
    """PPO_DeepSets(fused_act=True): one rollout's storage against the plain forward of the stored
    observations."""
    from lbk8s import fused
    algo = _ppo(B, T, True, **env_kw)
    assert algo.fused_act and algo.obs.shape == (T, B, R, 8)
    for t in range(T):
        logits, value = fused.deepsets_forward(algo.agent, algo.obs[t], require=True)
        a = algo.actions[t].cpu().numpy()
        assert np.array_equal(a, np.round(a)) and ((a >= 0) & (a < R)).all(), t
        assert torch.equal(algo.values[t], value), t
        lg = logits.cpu().numpy()
        m = sr.check_logprob(lg, None, a, algo.logprobs[t].cpu().numpy(), f"ppo R{R} step {t}")
        assert m <= 1.0
        if t == 0:
            sr.check_interval(lg, None, algo._u[0].cpu().numpy(), a, f"ppo R{R} step 0")
        if t == T - 1:  # (the env's action buffer holds the last step's actions)
            assert torch.equal(algo._act, algo.actions[t].to(torch.int32))


@pytest.mark.parametrize("B,T,env_kw", [(256, 8, {}), (512, 4, {"num_endpoints": 64})])
def test_ppo_default_path_is_agent_act(B, T, env_kw):
    """fused_act=False (the default) is the rollout as it was: every step's storage rows are
    agent.act's results on the stored observation and uniforms, bit for bit."""
    algo = _ppo(B, T, False, **env_kw)
    assert not algo.fused_act
    from lbk8s.ppo import PPO_DeepSets
    import inspect
    assert inspect.signature(PPO_DeepSets.__init__).parameters["fused_act"].default is False
    for t in range(T):
        action, logprob, value = algo.agent.act(algo.obs[t], uniforms=algo._u[t])
        assert action.dtype == torch.int64
        assert torch.equal(algo.actions[t], action.float()), t
        assert torch.equal(algo.logprobs[t], logprob) and torch.equal(algo.values[t], value), t
