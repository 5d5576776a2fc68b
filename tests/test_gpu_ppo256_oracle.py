"""k_ppo_steps256 (csrc/lbk8s_ppo256.h: lb_ppo_steps256, a PPO rollout's vector steps in one launch
for envs of 65 to 256 endpoints) pinned to the C oracle and the float64 definition of the draw,
independently of the three launches tests/test_gpu_ppo_steps256.py compares it with.

One launch of 6 steps on 8 envs with 2-step episodes (every env ends inside the launch and goes on
from its restart), at the first row count of each kernel instance and the largest: R = 66
(<2, false>), 81 (<2, true>), 129 and 257 (<4, true>: E = 129 .. 256 have four endpoints per lane;
129 rows with the reject row on E = 128 is <2, true>'s last).  Then:

  * the env: oracle.OracleBatch follows the launch's own actions; every step's reward, done flag
    and next observations equal the oracle's bit for bit;
  * the draw: for every stored row, lb_ds_forward's logits and value of that row's input
    observation (the plain forward, another kernel), with the row's uniform, action,
    log-probability and value, go through tests/ds_sample_ref.check_sample -- the logits and the
    value near the float64 network (ds_ref.near), the row's value equal to the plain forward's bit
    for bit, the action inside its inverse-CDF interval under the float64 softmax, the
    log-probability within the checker's bound.  Tolerances are the checker's, unchanged; no row is
    exempt.
"""
import copy

import numpy as np
import pytest
import torch

import ds_sample_ref as sr
from ds_sample_ref import Case, Setup
from eval_ref import bits

pytestmark = pytest.mark.gpu

B, STEPS, L = 8, 6, 2
# R: (E, reject, weight seed)
CASES = {66: (65, True, 3), 81: (80, True, 5), 129: (128, True, 7), 257: (256, True, 11)}


@pytest.mark.parametrize("R", sorted(CASES))
def test_ppo_steps256_equals_oracle_and_float64_draw(oracle_mod, R):
    from lbk8s import LBVecEnv, fused
    from lbk8s.deepsets import DeepSetAgent
    E, rej, wseed = CASES[R]
    kw = dict(num_endpoints=E, rejection_allowed=rej, reward_function="multi", episode_length=L)
    env = LBVecEnv(B, seed=5, as_tensors=True, **kw)
    env.reset()
    assert env.cfg.obs_rows == R and env.ppo_steps256_supported(R) and not env.ppo_steps64_supported(R)
    orc = oracle_mod.OracleBatch(kw, B, trace=False, auto_reset=True, seed=5)
    orc.init()
    obs0 = orc.reset()
    eq = np.testing.assert_array_equal
    eq(bits(env.obs.cpu().numpy()), bits(obs0), err_msg="reset obs")
    torch.manual_seed(wseed)
    agent = DeepSetAgent(env).cuda()
    n64 = copy.deepcopy(agent).double().cpu()
    frag = fused.packed(agent, agent.actor.net, agent.critic)
    u = torch.rand((STEPS, B), generator=torch.Generator().manual_seed(R)).cuda()
    u[0, 0], u[0, 1] = 0.0, sr.U_ONE
    z = lambda *s, dt=torch.float32: torch.full(s, float("nan") if dt.is_floating_point else 0, dtype=dt, device="cuda")
    actions, logprobs, values, rewards = z(STEPS, B), z(STEPS, B), z(STEPS, B), z(STEPS, B)
    obs_next, dones_next = z(STEPS, B, R, 8), z(STEPS, B)
    first = env.obs.clone()
    env.ppo_steps256(frag, first, u, actions, logprobs, values, rewards, obs_next, dones_next, None, None,
                     z(B, dt=torch.int32), z(B, dt=torch.uint8), torch.zeros(B, dtype=torch.float64, device="cuda"),
                     torch.zeros(B, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    a_all = actions.cpu().numpy()
    ended = np.zeros(B, np.int64)
    for i in range(STEPS):
        what = f"R{R} step {i}"
        a = a_all[i].astype(np.int32)
        assert np.array_equal(a_all[i], a.astype(np.float32)) and ((a >= 0) & (a < R)).all(), what
        # the draw of row i, on its input observation
        x = first if i == 0 else obs_next[i - 1]
        logits, value = fused.deepsets_forward(agent, x, require=True)
        with torch.no_grad():
            x64 = x.double().cpu()
            ref = {"logits": n64.actor(x64).numpy(), "value": n64.critic(x64).numpy()}
        s = Setup(Case("sample", "ac", R, f"B{B}", (0, 1, 0), False), B, None, None, None, ref)
        got = sr.as_numpy(sr.alloc_outputs(B, R, "ac"))
        got["actions"][:B], got["actions_f32"][:B] = a, a_all[i]
        got["logprob"][:B], got["value"][:B] = logprobs[i].cpu().numpy(), values[i].cpu().numpy()
        got["logits"][:B * R] = logits.cpu().numpy().reshape(-1)
        fwd = {"logits": logits.cpu().numpy(), "value": value.cpu().numpy()}
        margins = sr.check_sample(s, None, u[i].cpu().numpy(), got, fwd=fwd)
        print(what, margins)
        assert all(v <= 1.0 for v in margins.values()), what
        # the env, following the launch's actions
        o2, r2, d2, _, _ = orc.step(a)
        eq(bits(rewards[i].cpu().numpy()), bits(r2), err_msg=f"{what}: rewards")
        eq(dones_next[i].cpu().numpy(), d2.astype(np.float32), err_msg=f"{what}: dones_next")
        eq(bits(obs_next[i].cpu().numpy()), bits(o2), err_msg=f"{what}: obs_next")
        ended += d2.astype(np.int64)
    assert a_all[0, 0] == 0.0  # u = 0: the first row
    assert ended.min() >= STEPS // L - 1 and ended.max() >= 2  # every env went on from a restart
