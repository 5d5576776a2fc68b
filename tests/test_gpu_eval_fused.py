"""run_test(fused=True) (lbk8s/evaluate.py: the whole evaluation in one launch, LBVecEnv.eval_steps)
== the per-step loop written here -- fused.q_argmax_graphable on the same actor-only image, then
env.step -- on every array of the result dict and the per-step trace, bit for bit, for a PPO and
a DQN agent; the monitor file of both; the refusal and the fall-back at a shape with no one-launch
evaluation; the CLI flag.

Equality with run_test(fused=False) is deliberately not asserted: that loop takes torch's argmax
of a MODE 0 forward's scores, the launch takes the argmax inside the MODE 2 forward, and a float32
near-tie may resolve differently.  test_fused_against_the_torch_argmax_loop reports how many
episodes differ (measured on an MI355X with the seeds below: 0 of 50 for either agent).
"""
import csv
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import REPO

pytestmark = pytest.mark.gpu

N, E, L = 50, 6, 7
KW = dict(num_endpoints=E, episode_length=L)


def _agent(alg):
    from lbk8s.deepsets import DeepSetAgent, DQNDeepSetAgent
    torch.manual_seed(7 if alg == "ppo" else 8)
    return (DeepSetAgent if alg == "ppo" else DQNDeepSetAgent)(8).cuda().eval()


@torch.no_grad()
def _loop(agent, n, seed, **env_kwargs):
    """run_test's evaluation step by step: the greedy forward of the actor-only image, env.step."""
    from lbk8s import LBVecEnv, fused
    from lbk8s.deepsets import DeepSetAgent
    from lbk8s.evaluate import TEST_ENV
    from lbk8s.info import INFO_KEYS, ST_LENGTH, ST_RETURN, info_matrix
    kw = dict(TEST_ENV)
    kw.update(env_kwargs)
    env = LBVecEnv(n, device="cuda", seed=seed, env_id_offset=0, auto_reset=False, as_tensors=True, **kw)
    # (q_argmax_graphable packs a DQN agent's q_network: the PPO actor is the same module)
    qnet = types.SimpleNamespace(q_network=agent.actor) if isinstance(agent, DeepSetAgent) else agent
    frag = fused.frag_buffer(env.device)
    acts = torch.zeros(n, dtype=torch.int32, device=env.device)
    obs, masks = env.reset(), env.action_masks()
    tr = {k: [] for k in ("actions", "rewards", "dones")}
    for _ in range(env.cfg.episode_length):
        fused.q_argmax_graphable(qnet, obs, masks, acts, frag)
        obs, rew, dones, _ = env.step(acts)
        tr["actions"].append(env.actions.cpu().numpy().copy())
        tr["rewards"].append(rew.cpu().numpy().copy())
        tr["dones"].append(dones.cpu().numpy().copy())
    st = env.stats().cpu().numpy()
    info = info_matrix(st, env.rewards.cpu().numpy(), env.actions.cpu().numpy())
    out = {"r": st[:, ST_RETURN].copy(), "l": st[:, ST_LENGTH].astype(np.int64), "wall_s": 0.0}
    for j, k in enumerate(INFO_KEYS[:12]):
        out[k] = info[:, j]
    out.update({k: np.stack(v) for k, v in tr.items()})
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same_result(a, b, keys=None):
    keys = (set(a) | set(b)) - {"wall_s"} if keys is None else keys
    for k in sorted(keys):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, k
        np.testing.assert_array_equal(_bits(x), _bits(y), err_msg=k)


def _csv_rows(path):
    """The monitor file without its header line and its t column."""
    with open(path, newline="") as f:
        assert f.readline().startswith("#")
        rows = list(csv.reader(f))
    t = rows[0].index("t")
    return [r[:t] + r[t + 1:] for r in rows]


@pytest.mark.parametrize("alg", ("ppo", "dqn"))
def test_fused_run_test_equals_step_loop(tmp_path, alg):
    from lbk8s import evaluate
    from lbk8s.info import INFO_KEYS
    agent = _agent(alg)
    got = evaluate.run_test(agent, n_episodes=N, seed=42, fused=True, return_trace=True,
                            monitor_path=str(tmp_path / "fused.monitor.csv"), **KW)
    want = _loop(agent, N, 42, **KW)
    _same_result(got, want)
    assert got["actions"].shape == (L, N) and got["actions"].dtype == np.int32
    assert got["rewards"].dtype == np.float32 and got["dones"].dtype == np.bool_
    assert not got["dones"][:-1].any() and got["dones"][-1].all() and (got["l"] == L).all()
    assert len(np.unique(got["actions"])) > 1 and got["wall_s"] > 0
    # the float64 returns are the sums of the trace's rewards up to float32 rounding of each
    np.testing.assert_allclose(got["rewards"].astype(np.float64).sum(0), got["r"], rtol=1e-5, atol=1e-4)
    evaluate.write_monitor_csv(str(tmp_path / "loop.monitor.csv"), want, INFO_KEYS[:12])
    a, b = _csv_rows(tmp_path / "fused.monitor.csv"), _csv_rows(tmp_path / "loop.monitor.csv")
    assert a == b and len(a) == 1 + N
    # without the trace: the same dict, no trace keys
    plain = evaluate.run_test(agent, n_episodes=N, seed=42, fused=True, **KW)
    assert not {"actions", "rewards", "dones"} & set(plain)
    _same_result(plain, want, set(plain) - {"wall_s"})
    # fused=None takes the launch here
    _same_result(evaluate.run_test(agent, n_episodes=N, seed=42, fused=None, return_trace=True, **KW), want)


@pytest.mark.parametrize("alg", ("ppo", "dqn"))
def test_fused_against_the_torch_argmax_loop(alg):
    """Not an equality (a float32 near-tie may resolve differently): the loop path's trace has the
    launch's layout, and the number of episodes that differ is reported."""
    from lbk8s import evaluate
    agent = _agent(alg)
    a = evaluate.run_test(agent, n_episodes=N, seed=42, fused=True, return_trace=True, **KW)
    b = evaluate.run_test(agent, n_episodes=N, seed=42, return_trace=True, **KW)
    assert set(a) == set(b)
    for k in ("actions", "rewards", "dones"):
        assert a[k].shape == b[k].shape == (L, N) and a[k].dtype == b[k].dtype, k
    differ = int((a["actions"] != b["actions"]).any(0).sum())
    print(f"\n{alg}: {differ} of {N} episodes differ between run_test(fused=True) and run_test(fused=False)")
    same = ~(a["actions"] != b["actions"]).any(0)
    np.testing.assert_array_equal(_bits(a["r"][same]), _bits(b["r"][same]))


def test_fused_chunks_an_episode_longer_than_one_launch(monkeypatch):
    """episode_length > LB_EVAL_STEPS_MAX: launches of LB_EVAL_STEPS_MAX steps, the same result."""
    from lbk8s import _native, evaluate
    agent = _agent("dqn")
    whole = evaluate.run_test(agent, n_episodes=9, seed=3, fused=True, return_trace=True, **KW)
    monkeypatch.setattr(_native, "LB_EVAL_STEPS_MAX", 3)  # 7 steps: launches of 3, 3 and 1
    _same_result(evaluate.run_test(agent, n_episodes=9, seed=3, fused=True, return_trace=True, **KW), whole)


def test_fused_refused_and_fallback_at_e64():
    from lbk8s import evaluate
    agent = _agent("dqn")
    kw = dict(num_endpoints=64, episode_length=3)
    with pytest.raises(ValueError, match="eval_steps_supported"):
        evaluate.run_test(agent, n_episodes=8, seed=1, fused=True, **kw)
    loop = evaluate.run_test(agent, n_episodes=8, seed=1, fused=False, return_trace=True, **kw)
    _same_result(evaluate.run_test(agent, n_episodes=8, seed=1, fused=None, return_trace=True, **kw), loop)
    assert loop["actions"].shape == (3, 8)


def test_cli_test_fused(tmp_path):
    """python -m lbk8s.cli --testing --test-fused on a checkpoint saved here."""
    agent = _agent("dqn")
    path = tmp_path / "dqn.pt"
    torch.save(agent.state_dict(), path)
    env = dict(os.environ, PYTHONPATH=os.path.join(REPO, "gym-loadbalancing_amd"))
    r = subprocess.run([sys.executable, "-m", "lbk8s.cli", "--alg", "dqn_deepsets", "--no_training", "--testing",
                        "--test-fused", "--rejection", "--test_path", str(path), "--test_episodes", "5"],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    res = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    assert len(res["test_returns"]) == 5 and all(np.isfinite(res["test_returns"]))
    # the same episodes as the call the flag stands for
    from lbk8s import cli, evaluate
    want = evaluate.run_test(evaluate.load_agent(str(path), "dqn"), n_episodes=5, seed=0, fused=True,
                             **cli.env_kwargs(True, 6, 4, 24, "multi"))
    assert res["test_returns"] == [float(x) for x in want["r"]]
