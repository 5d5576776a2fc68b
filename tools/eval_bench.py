#!/usr/bin/env python3
"""A/B of the greedy evaluation: lbk8s.evaluate.run_test step by step (one fused forward, three
torch ops and one lb_step per time step, issued from Python) against run_test(fused=True) (the
whole episode in one launch: lb_eval_steps).

    python tools/eval_bench.py [--rounds 20] [--warmup 3] [--alg dqn] [--out profiles/eval_fused_ab.json]

Shapes: the evaluation's own (run_test_deepset.py: 2,000 episodes side by side, E = 6 with the
reject row, L = 100) and PPO's training batch (4,096 envs, E = 8, L = 100).  Both paths run in this
one process, alternating call by call after the warm-up calls of each.  Per call two times are
taken: run_test's own play window ("wall_s": a host clock from the first step's issue to the
device-to-host copy of the statistics, which waits for the device; divided by L it is the time per
vector step) and device events around the whole call (env construction, reset, the play window, the
result's copies).  The medians over the rounds go to the JSON file with the device and the host the
run was on.  No speed is asserted here.

With --fused-rollout-e64 the one launch is lb_eval_steps64 (run_test(e64=True)) and the shapes are
its own: 2,000 envs of E = 64 and of E = 32 with the reject row, L = 100.  With --fused-e256 it is
lb_eval_steps256 (run_test(e256=True)) at 2,000 envs of E = 80, 128, 180 and 256 with the reject
row, L = 100: the evaluation sweep's sizes past 64 endpoints and the env's largest.
"""
import argparse
import json
import os
import platform
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gym-loadbalancing_amd")]

SHAPES = {"run_test_2000_envs_E6": dict(n=2000, E=6, L=100), "ppo_batch_4096_envs_E8": dict(n=4096, E=8, L=100)}
SHAPES_E64 = {"run_test_2000_envs_E64": dict(n=2000, E=64, L=100), "run_test_2000_envs_E32": dict(n=2000, E=32, L=100)}
SHAPES_E256 = {f"run_test_2000_envs_E{E}": dict(n=2000, E=E, L=100) for E in (80, 128, 180, 256)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--alg", choices=("dqn", "ppo"), default="dqn")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "eval_fused_ab.json"))
    ap.add_argument("--fused-rollout-e64", action="store_true",
                    help="the one launch through lb_eval_steps64 (run_test(e64=True)) at E = 64 and E = 32")
    ap.add_argument("--fused-e256", action="store_true",
                    help="the one launch through lb_eval_steps256 (run_test(e256=True)) at E = 80, 128, 180 and 256")
    args = ap.parse_args()
    e64, e256 = args.fused_rollout_e64, args.fused_e256
    import numpy as np
    import torch

    from lbk8s import _native, evaluate
    from lbk8s.deepsets import DeepSetAgent, DQNDeepSetAgent
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench.py measures on a HIP device: none found")
    torch.manual_seed(1)
    agent = (DQNDeepSetAgent if args.alg == "dqn" else DeepSetAgent)(8).cuda().eval()
    prop = torch.cuda.get_device_properties(0)
    out = dict(what="A/B of run_test's play window: the per-step loop (fused=False) against one lb_eval_steps launch "
                    "(fused=True); one process, the two paths alternating call by call after warm-up",
               box=dict(host=platform.node(), device=prop.name, compute_units=prop.multi_processor_count,
                        torch=torch.__version__, hip=torch.version.hip),
               lib_source_hash=_native.lib().lb_source_hash().decode(), agent=args.alg, rounds=args.rounds,
               warmup_calls_per_path=args.warmup, e64=e64, e256=e256, shapes={})
    for name, sh in (SHAPES_E256 if e256 else SHAPES_E64 if e64 else SHAPES).items():
        kw = dict(num_endpoints=sh["E"], episode_length=sh["L"])

        def call(fused, **more):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            res = evaluate.run_test(agent, n_episodes=sh["n"], seed=42, fused=fused, e64=e64, e256=e256, **kw, **more)
            b.record()
            b.synchronize()
            return res, a.elapsed_time(b)

        for fused in (False, True):
            for _ in range(args.warmup):
                call(fused)
        step_us, call_ms = {False: [], True: []}, {False: [], True: []}
        for _ in range(args.rounds):
            for fused in (False, True):
                res, ms = call(fused)
                step_us[fused].append(res["wall_s"] / sh["L"] * 1e6)
                call_ms[fused].append(ms)
        a = call(True, return_trace=True)[0]
        b = call(False, return_trace=True)[0]
        differ = int((a["actions"] != b["actions"]).any(0).sum())

        def summary(fused):
            return dict(us_per_vector_step_median=round(statistics.median(step_us[fused]), 2),
                        us_per_vector_step_min=round(min(step_us[fused]), 2),
                        us_per_vector_step_max=round(max(step_us[fused]), 2),
                        us_per_vector_step_spread=round(max(step_us[fused]) - min(step_us[fused]), 2),
                        whole_call_ms_median=round(statistics.median(call_ms[fused]), 3))

        row = dict(envs=sh["n"], num_endpoints=sh["E"], obs_rows=sh["E"] + 1, episode_length=sh["L"],
                   loop=summary(False), one_launch=summary(True),
                   episodes_that_differ=differ, mean_return_loop=float(np.mean(b["r"])),
                   mean_return_one_launch=float(np.mean(a["r"])))
        row["loop_over_one_launch"] = round(row["loop"]["us_per_vector_step_median"]
                                            / row["one_launch"]["us_per_vector_step_median"], 2)
        out["shapes"][name] = row
        print(json.dumps({name: row}), flush=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
