"""run_test(fused=True, e256=True) (lbk8s/evaluate.py: the whole evaluation in one launch through
LBVecEnv.eval_steps256) at E = 80 and E = 180 == the per-step loop of tests/test_gpu_eval_fused.py --
fused.q_argmax_graphable on the same actor-only image, then env.step -- on every array of the
result dict and the per-step trace, bit for bit; the refusal at 32,768 episodes; e256=False left as
it was; run_sweep == its run_test calls, with its monitor files; the CLI's two flags.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from test_gpu_eval_fused import _agent, _csv_rows, _loop, _same_result

pytestmark = pytest.mark.gpu

N, L = 64, 10


@pytest.mark.parametrize("alg,E", (("dqn", 80), ("ppo", 180)))
def test_e256_run_test_equals_step_loop(alg, E):
    from lbk8s import evaluate
    agent = _agent(alg)
    kw = dict(num_endpoints=E, episode_length=L)
    got = evaluate.run_test(agent, n_episodes=N, seed=1, fused=True, e256=True, return_trace=True, **kw)
    want = _loop(agent, N, 1, **kw)
    _same_result(got, want)
    assert got["actions"].shape == (L, N) and got["actions"].dtype == np.int32
    assert not got["dones"][:-1].any() and got["dones"][-1].all() and (got["l"] == L).all()
    assert got["wall_s"] > 0
    # fused=None takes the launch here
    _same_result(evaluate.run_test(agent, n_episodes=N, seed=1, fused=None, e256=True, return_trace=True, **kw), want)
    # e256=False keeps today's answers: no one-launch evaluation under the older names
    with pytest.raises(ValueError, match="eval_steps64_supported"):
        evaluate.run_test(agent, n_episodes=N, seed=1, fused=True, e64=True, **kw)
    with pytest.raises(ValueError, match="eval_steps_supported"):
        evaluate.run_test(agent, n_episodes=N, seed=1, fused=True, **kw)


def test_e256_refused_at_32768_episodes():
    from lbk8s import evaluate
    with pytest.raises(ValueError, match="eval_steps256_supported"):
        evaluate.run_test(_agent("dqn"), n_episodes=32768, seed=1, fused=True, e256=True, num_endpoints=80,
                          episode_length=2)


def test_run_sweep_equals_its_run_test_calls(tmp_path):
    from lbk8s import evaluate
    agent = _agent("dqn")
    ends = (6, 80, 180)
    got = evaluate.run_sweep(agent, num_endpoints=ends, n_episodes=32, out_dir=str(tmp_path), fused=True, e256=True,
                             episode_length=L)
    assert tuple(got) == ends
    for i, e in enumerate(ends):
        ref = tmp_path / f"ref{e}.monitor.csv"
        want = evaluate.run_test(agent, n_episodes=32, seed=42, fused=True, e256=True, monitor_path=str(ref),
                                 num_endpoints=e, episode_length=L)
        _same_result(got[e], want)
        name = f"{i}_loadbalancer_gym_results_num_endpoints_{e}.monitor.csv"
        assert name == evaluate.sweep_monitor_name(i, e)
        assert _csv_rows(tmp_path / name) == _csv_rows(ref) and len(_csv_rows(ref)) == 1 + 32
    assert sorted(f for f in os.listdir(tmp_path) if f[0].isdigit()) == [evaluate.sweep_monitor_name(i, e)
                                                                          for i, e in enumerate(ends)]
    # the defaults (the per-step loop) give run_test's defaults; no out_dir, no file
    plain = evaluate.run_sweep(agent, num_endpoints=(80,), n_episodes=8, episode_length=3)
    _same_result(plain[80], evaluate.run_test(agent, n_episodes=8, seed=42, num_endpoints=80, episode_length=3))


def test_cli_test_sweep_fused_e256(tmp_path):
    """python -m lbk8s.cli --testing --test-sweep 6,80 --test-fused-e256 on a checkpoint saved here:
    one line and one monitor file per entry, the episodes of the run_sweep call the flags stand for."""
    agent = _agent("dqn")
    path = tmp_path / "dqn.pt"
    torch.save(agent.state_dict(), path)
    env = dict(os.environ, PYTHONPATH=os.path.join(REPO, "gym-loadbalancing_amd"))
    r = subprocess.run([sys.executable, "-m", "lbk8s.cli", "--alg", "dqn_deepsets", "--no_training", "--testing",
                        "--test-sweep", "6,80", "--test-fused-e256", "--rejection", "--test_path", str(path),
                        "--test_episodes", "5"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("num_endpoints ")]
    assert [ln.split()[1].rstrip(":") for ln in lines] == ["6", "80"] and all("wall" in ln for ln in lines)
    res = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    from lbk8s import cli, evaluate
    kw = cli.env_kwargs(True, 6, 4, 24, "multi")
    kw.pop("num_endpoints")
    want = evaluate.run_sweep(evaluate.load_agent(str(path), "dqn"), num_endpoints=(6, 80), n_episodes=5, seed=0,
                              fused=True, e256=True, **kw)
    for i, e in enumerate((6, 80)):
        assert res["test_sweep"][str(e)]["mean_return"] == float(want[e]["r"].mean())
        assert len(_csv_rows(tmp_path / evaluate.sweep_monitor_name(i, e))) == 1 + 5
