"""run_test(fused=True, e64=True) (lbk8s/evaluate.py: the whole evaluation in one launch through
LBVecEnv.eval_steps64) at E = 64 == the per-step loop of tests/test_gpu_eval_fused.py --
fused.q_argmax_graphable on the same actor-only image, then env.step -- on every array of the
result dict and the per-step trace, bit for bit; the refusal and the fall-back past 64 endpoints;
e64=False left as it was; the CLI flag.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from test_gpu_eval_fused import _agent, _loop, _same_result

pytestmark = pytest.mark.gpu

KW = dict(num_endpoints=64, episode_length=3)


@pytest.mark.parametrize("alg", ("dqn", "ppo"))
def test_e64_run_test_equals_step_loop(alg):
    from lbk8s import evaluate
    agent = _agent(alg)
    got = evaluate.run_test(agent, n_episodes=8, seed=1, fused=True, e64=True, return_trace=True, **KW)
    want = _loop(agent, 8, 1, **KW)
    _same_result(got, want)
    assert got["actions"].shape == (3, 8) and got["actions"].dtype == np.int32
    assert not got["dones"][:-1].any() and got["dones"][-1].all() and (got["l"] == 3).all()
    assert got["wall_s"] > 0
    # fused=None takes the launch here; at a 16-lane shape e64=True is the same evaluation
    _same_result(evaluate.run_test(agent, n_episodes=8, seed=1, fused=None, e64=True, return_trace=True, **KW), want)
    small = dict(num_endpoints=6, episode_length=7)
    _same_result(evaluate.run_test(agent, n_episodes=9, seed=3, fused=True, e64=True, return_trace=True, **small),
                 evaluate.run_test(agent, n_episodes=9, seed=3, fused=True, return_trace=True, **small))


def test_e64_refused_and_fallback_at_e100():
    from lbk8s import evaluate
    agent = _agent("dqn")
    kw = dict(num_endpoints=100, episode_length=3)
    with pytest.raises(ValueError, match="eval_steps64_supported"):
        evaluate.run_test(agent, n_episodes=8, seed=1, fused=True, e64=True, **kw)
    loop = evaluate.run_test(agent, n_episodes=8, seed=1, fused=False, return_trace=True, **kw)
    _same_result(evaluate.run_test(agent, n_episodes=8, seed=1, fused=None, e64=True, return_trace=True, **kw), loop)
    assert loop["actions"].shape == (3, 8)
    # e64=False keeps today's answers at E = 64
    with pytest.raises(ValueError, match="eval_steps_supported"):
        evaluate.run_test(agent, n_episodes=8, seed=1, fused=True, **KW)


def test_cli_test_fused_e64(tmp_path):
    """python -m lbk8s.cli --testing --test-fused-e64 at 64 endpoints on a checkpoint saved here."""
    agent = _agent("dqn")
    path = tmp_path / "dqn.pt"
    torch.save(agent.state_dict(), path)
    env = dict(os.environ, PYTHONPATH=os.path.join(REPO, "gym-loadbalancing_amd"))
    r = subprocess.run([sys.executable, "-m", "lbk8s.cli", "--alg", "dqn_deepsets", "--no_training", "--testing",
                        "--test-fused-e64", "--rejection", "--num_endpoints", "64", "--test_path", str(path),
                        "--test_episodes", "5"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    res = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    assert len(res["test_returns"]) == 5 and all(np.isfinite(res["test_returns"]))
    # the same episodes as the call the flag stands for
    from lbk8s import cli, evaluate
    want = evaluate.run_test(evaluate.load_agent(str(path), "dqn"), n_episodes=5, seed=0, fused=True, e64=True,
                             **cli.env_kwargs(True, 64, 4, 24, "multi"))
    assert res["test_returns"] == [float(x) for x in want["r"]]
