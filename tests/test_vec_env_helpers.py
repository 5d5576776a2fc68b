"""LBVecEnv's private helpers behind record_ppo / ppo_steps / eval_steps, on the host alone: the
launch splitter (every launch ends where a monitor flush is due) and the tensor-spec checker."""
import pytest
import torch

from lbk8s.vec_env import LBVecEnv


def _bare(monitor, log_every=64, logged=0):
    """An LBVecEnv with the helpers' fields only (no library, no device)."""
    env = LBVecEnv.__new__(LBVecEnv)
    env.torch = torch
    env.ep_stats = torch.zeros(4, 1, dtype=torch.float64)
    env.monitor = monitor
    env._log_every = log_every
    env._log_times = [0.0] * logged
    env.flushes = []
    env.flush_monitor = lambda: (env.flushes.append(len(env._log_times)), env._log_times.clear())
    return env


def _split(env, T, most):
    out = []
    for i, n in env._launches(T, most):
        out.append((i, n))
        env._logged(n)
    return out


def test_launches_unmonitored_split_by_the_maximum_only():
    env = _bare(False)
    assert _split(env, 10, 4096) == [(0, 10)]
    assert _split(env, 10, 4) == [(0, 4), (4, 4), (8, 2)]
    assert env._log_times == [] and env.flushes == []


def test_launches_end_where_a_flush_is_due():
    env = _bare(True, log_every=64, logged=60)  # 60 steps logged since the last flush
    assert _split(env, 100, 4096) == [(0, 4), (4, 64), (68, 32)]
    assert env.flushes == [64, 64] and len(env._log_times) == 32
    env = _bare(True, log_every=8)
    assert _split(env, 20, 5) == [(0, 5), (5, 3), (8, 5), (13, 3), (16, 4)]  # the maximum and the cadence
    assert env.flushes == [8, 8] and len(env._log_times) == 4


def test_check_tensors():
    env = _bare(False)
    ok = torch.zeros(3, 2)
    env._check_tensors("f", [("a", ok, (3, 2), torch.float32, False), ("b", None, (3,), torch.int32, True)])
    for bad in (None, ok.double(), ok.t(), torch.zeros(2, 3), ok.numpy()):
        with pytest.raises(ValueError, match=r"f: a must be a contiguous \(3, 2\) torch.float32 tensor on cpu"):
            env._check_tensors("f", [("a", bad, (3, 2), torch.float32, False)])
