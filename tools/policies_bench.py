#!/usr/bin/env python3
"""Measurements of the policies LB_POLICY_ROUND_ROBIN .. LB_POLICY_REWARD_GREEDY (recorded, no
threshold): profiles/policies_rollout.json.

    python tools/policies_bench.py [--out profiles/policies_rollout.json]

* per vector step, the one-launch lb_rollout against K x (lb_policy + lb_step), for each new kind,
  at 4,096 default envs and at 2,000 envs of config 1 (run_baselines' env): K = 100 steps per
  launch, device events around `reps` launches after a warm-up, the median of 5 windows;
* the reward-greedy lb_policy launch at E = 64 and E = 256, 4,096 envs (the same timing);
* the mean episode return of the seven deterministic policies and of uniform random at config 1
  (naive reward) and at the evaluation env (lbk8s.evaluate.TEST_ENV: multi reward, latency weight
  1), 2,000 episodes each (run_baselines; random through the same rollout);
* VGPRs / scratch / LDS of the new kernels, read from the library's code objects
  (tools/kernel_meta.py).
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gym-loadbalancing_amd"), os.path.join(REPO, "tools")]

K8S = ("round_robin", "least_loaded", "least_latency", "reward_greedy")


def timed(torch, fn, reps, windows=5):
    """Median over `windows` of the device time of `reps` calls of fn, per call, in us."""
    for _ in range(max(3, reps // 5)):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return statistics.median(out), min(out), max(out)


def rollout_vs_steps(torch, LBVecEnv, B, kw, K=100):
    rows = []
    for kind in K8S:
        env = LBVecEnv(B, seed=3, as_tensors=True, **kw)
        env.reset()
        R = env.cfg.obs_rows
        obs = torch.empty((K, B, R, 8), device="cuda")
        rew = torch.empty((K, B), device="cuda")
        dn = torch.empty((K, B), dtype=torch.uint8, device="cuda")
        act = torch.empty((K, B), dtype=torch.int32, device="cuda")

        def one_launch():
            env.rollout(kind, K, obs_out=obs, reward_out=rew, done_out=dn, actions_out=act)

        def per_step():
            for k in range(K):
                env.policy(kind, out=act[k])
                env.step_device(act[k], obs_out=obs[k], reward_out=rew[k], done_out=dn[k])

        r = timed(torch, one_launch, 20)
        s = timed(torch, per_step, 5)
        rows.append(dict(kind=kind, envs=B, steps_per_launch=K, kernel=env.rollout_kernel(K, kind=kind),
                         rollout_us_per_vector_step=dict(median=r[0] / K, min=r[1] / K, max=r[2] / K),
                         policy_plus_step_us_per_vector_step=dict(median=s[0] / K, min=s[1] / K, max=s[2] / K)))
        assert env.status() == 0
    return rows


def greedy_policy_launch(torch, LBVecEnv, E, B=4096):
    env = LBVecEnv(B, seed=3, as_tensors=True, num_endpoints=E, reward_function="multi")
    env.reset()
    for _ in range(10):  # some history: counters and loads that differ
        env.step_device(None)
    out = torch.empty(B, dtype=torch.int32, device="cuda")
    t = timed(torch, lambda: env.policy("reward_greedy", out=out), 200)
    return dict(num_endpoints=E, envs=B, reward_function="multi", us_per_launch=dict(median=t[0], min=t[1], max=t[2]))


def mean_returns(torch, n=2000):
    import numpy as np

    from lbk8s import LBVecEnv
    from lbk8s.evaluate import TEST_ENV
    from lbk8s.info import ST_RETURN
    from lbk8s.run_baselines import CFG1, DEVICE_POLICIES, run_baselines
    out = {}
    for name, kw in (("config1_naive", CFG1), ("evaluation_env_multi_latency1", TEST_ENV)):
        row = {p: float(np.mean(run_baselines(policy=p, n_episodes=n, **kw)["returns"]))
               for p in DEVICE_POLICIES}
        env = LBVecEnv(n, seed=42, auto_reset=False, as_tensors=True, geometry="slice", **kw)
        env.reset()
        env.rollout("random", env.cfg.episode_length)
        row["random"] = float(env.stats()[:, ST_RETURN].mean().item())
        out[name] = dict(episodes=n, seed=42, mean_return=row)
    return out


def new_kernels():
    import kernel_meta

    from lbk8s import _native
    rows = []
    for k in kernel_meta.kernels(_native.LIB_PATH):
        n = k.get("name", "")
        tpe = "k_rollout_tpe" in n and any(f"ELi{kind}ELb" in n for kind in (4, 5, 6, 7))
        if tpe or "k_rollout_slice_k8s" in n or "k_policy_rg" in n:
            rows.append({f: k.get(f) for f in ("name", "vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count",
                                               "sgpr_spill_count", "private_segment_fixed_size",
                                               "group_segment_fixed_size")})
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "policies_rollout.json"))
    args = ap.parse_args()
    import torch

    from lbk8s import LBVecEnv
    from lbk8s.run_baselines import CFG1
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    res = dict(device=torch.cuda.get_device_name(0),
               rollout_vs_policy_plus_step=rollout_vs_steps(torch, LBVecEnv, 4096, {}) +
               rollout_vs_steps(torch, LBVecEnv, 2000, dict(CFG1)),
               reward_greedy_policy_launch=[greedy_policy_launch(torch, LBVecEnv, E) for E in (64, 256)],
               mean_returns=mean_returns(torch),
               new_kernels=new_kernels())
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({k: res[k] for k in ("rollout_vs_policy_plus_step", "reward_greedy_policy_launch", "mean_returns")}))


if __name__ == "__main__":
    main()
