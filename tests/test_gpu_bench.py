"""bench.py's plain run, --full and --dump-outputs, in process at a small size (4,104 envs:
no multiple of the block; 7 timed steps after a 3-step warm-up: a window inside one ring cycle)."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARGS = ["--gpus", "1", "--envs", "4104", "--steps", "7", "--warmup", "3"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(capsys, extra):
    import bench
    capsys.readouterr()
    bench.main(ARGS + extra)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_dumps_its_last_step(capsys, tmp_path):
    """A plain run measures the headline only; two runs with the same arguments write the same
    arrays (float32 / float64, under 64 MB), and those are the last timed step's outputs."""
    import bench
    lines, dumps = [], []
    for name in ("a", "b"):
        d = tmp_path / name
        lines.append(_bench(capsys, ["--dump-outputs", str(d)]))
        dumps.append({f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))})
    line = lines[0]
    for k in HEADLINE:
        assert k in line
    assert "lb_step" not in line and "cpu_baseline" not in line
    assert line["steps"] == 7 and line["warmup"] == 3
    assert line["value"] == pytest.approx(4104 * 7 / (line["ms_per_step"] * 7e-3))
    a, b = dumps
    assert sorted(a) == ["done", "env_ids", "ep_stats", "obs", "obs_env_ids", "reward", "terminal_obs"]
    assert sum(x.nbytes for x in a.values()) <= 64e6
    for k in a:
        assert a[k].dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(a[k], b[k])
    assert a["obs"].shape == (4104, 9, 8) and a["reward"].shape == (4104,)
    np.testing.assert_array_equal(a["env_ids"], np.arange(4104))
    # the same trajectory stepped by hand: bench.py's stagger, then warm-up + timed steps
    from lbk8s import LBVecEnv
    import torch
    env = LBVecEnv(4104, device="cuda:0", seed=0, as_tensors=True)
    L = env.cfg.episode_length
    env.reset()
    gid = torch.arange(4104, device="cuda:0")
    for r in range(1, L):
        env.step_device(None)
        env.reset_masked((gid % L) == r)
    for _ in range(1 + 3 + 7):  # (one step on a side stream precedes the graph capture)
        env.step_device(None)
    np.testing.assert_array_equal(a["obs"], env.obs.cpu().numpy())
    np.testing.assert_array_equal(a["reward"], env.rewards.cpu().numpy())
    np.testing.assert_array_equal(a["done"], env.dones.cpu().numpy().astype(np.float32))
    np.testing.assert_array_equal(a["terminal_obs"], env.terminal_obs.cpu().numpy())
    np.testing.assert_array_equal(a["ep_stats"], env.ep_stats.cpu().numpy())
    # a wide output is cut to a fixed sample of env rows
    ids = bench._dump_ids(1 << 20, 1000)
    assert ids.shape == (1000,) and np.all(np.diff(ids) > 0) and ids.max() < 1 << 20
    np.testing.assert_array_equal(ids, bench._dump_ids(1 << 20, 1000))


def test_full_run_keeps_the_other_measurements(capsys):
    """--full: the lb_step launch shape next to the same headline (and the CPU baselines,
    switched off here: they start a process per core)."""
    line = _bench(capsys, ["--full", "--no-cpu-baseline"])
    for k in HEADLINE:
        assert k in line
    assert line["lb_step"]["ms_per_step"] > 0 and line["lb_step"]["resets_in_window"] > 0
    assert "cpu_baseline" not in line
