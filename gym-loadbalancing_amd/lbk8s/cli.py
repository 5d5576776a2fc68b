"""run.py equivalent: the reference's CLI on the MI355X framework.

    python -m lbk8s.cli --alg ppo_deepsets --num_endpoints 64 --num_envs 4096 --total_steps 409600

Same flags and defaults as /root/reference/run.py:23-45, the same env construction
(get_env, :95-127: arrival rate 100, call duration 1, episode length 100, latency weight
1, cpu 0, gini 0; rejection only with --rejection), the same trainer arguments
(get_model, :54-72) and the same model name (:189-191).  By design:
  * the reference's SubprocVecEnv of 8 workers becomes one LBVecEnv of --num_envs envs
    (default 8) on the GPU, trained by the GPU-resident lbk8s.ppo / lbk8s.dqn;
  * only the deep-sets algorithms exist here: "ppo", "a2c", "recurrent_ppo" and
    "mask_ppo" (:56-63) are stable-baselines3 models, which this framework does not
    include (LBVecEnv can serve them as a VecEnv);
  * --testing runs the greedy evaluation of lbk8s.evaluate on the saved / given
    checkpoint (the reference's test_model, :130-161, plots one episode's reward);
  * loading returns the agent (the reference's get_load_model returns load()'s None);
  * the training envs write VecMonitor's file, vec_loadbalancer_k8s_gym_results.monitor.csv
    (run.py:122; one file per rank, suffixed, with --nproc > 1);
  * --nproc N trains on N GPUs of the node: N ranks (one process per GPU, launched here
    through torch.distributed.run), each with --num_envs envs of its own global env-id
    range, gradients and episode statistics all-reduced over RCCL; rank 0 saves.
"""
import argparse
import json
import logging
import os
import sys

SB3_ALGS = ("ppo", "recurrent_ppo", "a2c", "mask_ppo")


def build_parser():
    p = argparse.ArgumentParser(description="Run RL Agent!")
    p.add_argument("--alg", default="dqn_deepsets",
                   help='The algorithm: ["mask_ppo", "recurrent_ppo", "ppo", "mask_ppo", "ppo_deepsets", "dqn_deepsets"]')
    p.add_argument("--env_name", default="loadbalancer", help='Env: ["loadbalancer"]')
    p.add_argument("--num_endpoints", default=6, help="num_endpoints: 4, 8, etc")
    p.add_argument("--rejection", default=False, action="store_true", help="Testing mode")
    p.add_argument("--num_zones", default=4, help="num_zones: 4, 8, etc")
    p.add_argument("--num_nodes", default=24, help="num_nodes: 4, 8, etc")
    p.add_argument("--reward", default="multi", help='reward: ["naive", "latency", "fairness", "multi"]')
    p.add_argument("--training", default=True, action="store_true", help="Training mode")
    p.add_argument("--testing", default=False, action="store_true", help="Testing mode")
    p.add_argument("--loading", default=False, action="store_true", help="Loading mode")
    p.add_argument("--load_path",
                   default="results/a2c/multi/"
                           "ppo_env_loadbalancer_num_endpoints_6_num_zones_4_reward_multi_totalSteps_200000_run_1/"
                           "ppo_env_loadbalancer_num_endpoints_6_num_zones_4_reward_multi_totalSteps_200000",
                   help="Loading path, ex: logs/model/test.zip")
    p.add_argument("--test_path",
                   default="results/loadbalancer/multi/"
                           "a2c_env_loadbalancer_num_endpoints_6_num_zones_4_reward_multi_totalSteps_200000_run_1/"
                           "a2c_env_loadbalancer_num_endpoints_6_num_zones_4_reward_multi_totalSteps_200000",
                   help="Testing path, ex: logs/model/test.zip")
    p.add_argument("--steps", default=200000, help="Save model after X steps")
    p.add_argument("--total_steps", default=200000, help="The total number of steps.")
    # framework additions
    p.add_argument("--num_envs", default=8, type=int, help="parallel envs on the GPU (reference: 8 workers)")
    p.add_argument("--no_training", action="store_true", help="skip training (--training is always on)")
    p.add_argument("--test_episodes", default=1, type=int, help="episodes played side by side by --testing")
    p.add_argument("--test_sequential", action="store_true",
                   help="--testing plays the episodes one after another on one env, as run_test_deepset.py")
    p.add_argument("--test-fused", action="store_true",
                   help="--testing plays its episodes in one launch (run_test(fused=True)) where the env's shape "
                        "has it (E <= 16, R <= 16, fewer than 32,768 episodes; with --test-fused-e64 E <= 64, "
                        "R <= 65); ignored with --test_sequential")
    p.add_argument("--test-fused-e64", action="store_true",
                   help="--testing plays its episodes in one launch through lb_eval_steps64 "
                        "(run_test(fused=True, e64=True)): E <= 64, R <= 65, fewer than 32,768 episodes; ignored "
                        "with --test_sequential")
    p.add_argument("--test-fused-e256", action="store_true",
                   help="--testing plays its episodes in one launch through lb_eval_steps256 "
                        "(run_test(fused=True, e256=True)): E <= 256, R <= 257, fewer than 32,768 episodes; ignored "
                        "with --test_sequential")
    p.add_argument("--test-sweep", nargs="?", const=True, default=None, type=sweep_list, metavar="E,E,...",
                   help="--testing plays --test_episodes episodes at each of these numbers of endpoints "
                        "(run_sweep; default 6,12,16,24,32,48,64,80,128,150,180, as run_test_deepset.py), writes "
                        "one VecMonitor file per entry to the working directory and prints one line per entry; "
                        "ignored with --test_sequential")
    p.add_argument("--device", default="cuda")
    p.add_argument("--seed", default=0, type=int, help="Philox seed of the envs")
    p.add_argument("--nproc", default=1, type=int, help="GPUs (ranks) to train on, one process each")
    p.add_argument("--monitor_file", default="vec_loadbalancer_k8s_gym_results",
                   help="VecMonitor file of the training envs (run.py:122); '' disables it")
    p.add_argument("--fused-act", action="store_true",
                   help="ppo_deepsets: the rollout's policy step as one launch (PPO_DeepSets(fused_act=True))")
    p.add_argument("--fused-bookkeeping", action="store_true",
                   help="ppo_deepsets: the rollout step's bookkeeping and GAE as one launch each")
    p.add_argument("--fused-rollout", action="store_true",
                   help="ppo_deepsets: a rollout's vector steps as one launch where the env's shape has it "
                        "(E <= 16, R <= 16, fewer than 32,768 envs; with --fused-rollout-e64 E <= 64, R <= 65)")
    p.add_argument("--fused-rollout-e64", action="store_true",
                   help="ppo_deepsets: a rollout's vector steps as one launch through lb_ppo_steps64 "
                        "(PPO_DeepSets(fused_rollout_e64=True)): E <= 64, R <= 65, fewer than 32,768 envs")
    p.add_argument("--fused-rollout-e256", action="store_true",
                   help="ppo_deepsets: a rollout's vector steps as one launch through lb_ppo_steps256 "
                        "(PPO_DeepSets(fused_rollout_e256=True)): E <= 256, R <= 257, fewer than 32,768 envs")
    p.add_argument("--bootstrap-timeouts", action="store_true",
                   help="ppo_deepsets: at an episode's end (always the time limit) bootstrap the value target "
                        "from the critic's value of the terminal observation "
                        "(PPO_DeepSets(bootstrap_timeouts=True)); an error for dqn_deepsets")
    p.add_argument("--dqn-steps-e64", action="store_true",
                   help="dqn_deepsets: a train period's vector steps as one launch through lb_dqn_steps64 "
                        "(DQN_DeepSets(multi_step_e64=True)): E <= 64, R <= 65, fewer than 32,768 envs")
    p.add_argument("--dqn-steps-e256", action="store_true",
                   help="dqn_deepsets: a train period's vector steps as one launch through lb_dqn_steps256 "
                        "(DQN_DeepSets(multi_step_e256=True)): E <= 256, R <= 257, fewer than 32,768 envs")
    return p


def sweep_list(text):
    """--test-sweep's value: a comma list of endpoint counts -> a tuple of ints."""
    try:
        out = tuple(int(x) for x in str(text).split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a comma list of endpoint counts: {text!r}")
    if not out or min(out) < 1:
        raise argparse.ArgumentTypeError(f"endpoint counts must be >= 1: {text!r}")
    return out


def sweep_endpoints(args):
    """The endpoint counts --test-sweep asks for: None without the flag (or with --test_sequential,
    which wins), evaluate.SWEEP_ENDPOINTS for the bare flag, else its list."""
    if args.test_sweep is None or args.test_sequential:
        return None
    if args.test_sweep is True:
        from .evaluate import SWEEP_ENDPOINTS
        return SWEEP_ENDPOINTS
    return args.test_sweep


def eval_launch_flags(args):
    """run_test's fused / e64 / e256 from --test-fused / --test-fused-e64 / --test-fused-e256
    (all off with --test_sequential, which wins)."""
    if args.test_sequential:
        return dict(fused=False, e64=False, e256=False)
    return dict(fused=args.test_fused or args.test_fused_e64 or args.test_fused_e256, e64=args.test_fused_e64,
                e256=args.test_fused_e256)


def env_kwargs(rejection, num_endpoints, num_zones, num_nodes, reward_function):
    """get_env's LoadBalancerK8sEnv arguments (run.py:97-107)."""
    return dict(num_nodes=num_nodes, num_zones=num_zones, num_endpoints=num_endpoints,
                rejection_allowed=rejection, arrival_rate_r=100, call_duration_r=1, episode_length=100,
                reward_function=reward_function, latency_weight=1.0, cpu_weight=0.0, gini_weight=0.0)


def get_env(env_name, rejection, num_endpoints, num_zones, num_nodes, reward_function, num_envs=8,
            device="cuda", seed=0, env_id_offset=0, monitor_file=None):
    if env_name != "loadbalancer":
        raise SystemExit("Invalid environment!")
    from .info import INFO_KEYS
    from .vec_env import LBVecEnv
    return LBVecEnv(num_envs, device=device, seed=seed, env_id_offset=env_id_offset, as_tensors=True, monitor=True,
                    info_keywords=INFO_KEYS, monitor_file=monitor_file or None,
                    **env_kwargs(rejection, num_endpoints, num_zones, num_nodes, reward_function))


def get_model(alg, env, rank=0, dqn_steps_e64=False, dqn_steps_e256=False, **ppo_flags):
    """get_model (run.py:54-72) for the deep-sets algorithms.  With several ranks each rank's
    learner seed is offset by its rank, so rollout uniforms, minibatch permutations, replay
    samples and exploration coins differ across GPUs (the parameters are broadcast from rank
    0, so the replicas still start identical).  ppo_flags: PPO_DeepSets' fused_act /
    fused_bookkeeping / fused_rollout / fused_rollout_e64 / fused_rollout_e256 / bootstrap_timeouts (all off by
    default); dqn_steps_e64 /
    dqn_steps_e256: DQN_DeepSets' multi_step_e64 / multi_step_e256 (off by default)."""
    if alg == "ppo_deepsets":
        from .ppo import PPO_DeepSets
        return PPO_DeepSets(env, num_steps=100, n_minibatches=8, ent_coef=0.001, seed=2 + rank, **ppo_flags)
    if alg == "dqn_deepsets":
        from .dqn import DQN_DeepSets
        return DQN_DeepSets(env, num_steps=100, n_minibatches=8, seed=1 + rank, multi_step_e64=dqn_steps_e64,
                            multi_step_e256=dqn_steps_e256)
    if alg in SB3_ALGS:
        raise SystemExit(f"{alg!r} is a stable-baselines3 model; this framework provides the deep-sets "
                         "algorithms (ppo_deepsets, dqn_deepsets) and LBVecEnv as a VecEnv")
    raise SystemExit("Invalid algorithm!")


def model_name(alg, env_name, num_endpoints, num_zones, reward, total_steps):
    """run.py:189-191."""
    return (alg + "_env_" + env_name + "_num_endpoints_" + str(num_endpoints) + "_num_zones_" + str(num_zones)
            + "_reward_" + reward + "_totalSteps_" + str(total_steps))


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    args = build_parser().parse_args(argv)
    if args.bootstrap_timeouts and args.alg != "ppo_deepsets":  # (before any rank is spawned)
        raise SystemExit(f"--bootstrap-timeouts is a ppo_deepsets option: {args.alg!r} has no value target that "
                         "bootstraps from the terminal observation (DQN's replay stores the post-reset observation "
                         "at a done)")
    if args.nproc > 1 and int(os.environ.get("WORLD_SIZE", "1")) == 1:
        # spawn the ranks before anything touches the GPU, then wait for them
        from .dist import launch
        child = [a for i, a in enumerate(argv)  # the ranks get the torchrun environment instead
                 if not a.startswith("--nproc") and not (i > 0 and argv[i - 1] == "--nproc")]
        raise SystemExit(launch(args.nproc, "lbk8s.cli", child, module=True))
    logging.info(args)
    alg, reward = args.alg, args.reward
    num_nodes, num_zones, num_endpoints = int(args.num_nodes), int(args.num_zones), int(args.num_endpoints)
    total_steps = int(args.total_steps)
    name = model_name(alg, args.env_name, num_endpoints, num_zones, reward, total_steps)
    result = {"name": name}
    if args.training and not args.no_training:
        from .dist import init_from_env
        rank, world, dev = init_from_env("cuda" if str(args.device).startswith("cuda") else "cpu")
        mon = args.monitor_file + (f"_rank{rank}" if world > 1 and args.monitor_file else "")
        env = get_env(args.env_name, args.rejection, num_endpoints, num_zones, num_nodes, reward,
                      num_envs=args.num_envs, device=dev if world > 1 else args.device, seed=args.seed,
                      env_id_offset=rank * args.num_envs, monitor_file=mon)
        flags = dict(fused_act=args.fused_act, fused_bookkeeping=args.fused_bookkeeping,
                     fused_rollout=args.fused_rollout,
                     fused_rollout_e64=args.fused_rollout_e64,
                     fused_rollout_e256=args.fused_rollout_e256) if alg == "ppo_deepsets" else {}
        if alg == "ppo_deepsets" and args.bootstrap_timeouts:
            flags["bootstrap_timeouts"] = True
        if alg == "dqn_deepsets" and args.dqn_steps_e64:
            flags["dqn_steps_e64"] = True
        if alg == "dqn_deepsets" and args.dqn_steps_e256:
            flags["dqn_steps_e256"] = True
        model = get_model(alg, env, rank, **flags)
        if args.loading:  # resume training
            model.load(args.load_path)
        model.learn(total_timesteps=total_steps)
        env.close()
        result.update(world_size=world, episode_returns=[float(r) for r in model.episode_returns[-3:]])
        if rank == 0:
            model.save(name)
            result["saved"] = name
        if world > 1:
            import torch.distributed as dist
            dist.destroy_process_group()
            if rank != 0:
                return result
    if args.testing:
        from .evaluate import load_agent, run_sequential, run_sweep, run_test
        agent = load_agent(args.test_path, "ppo" if alg == "ppo_deepsets" else "dqn", device=args.device)
        kw = env_kwargs(args.rejection, num_endpoints, num_zones, num_nodes, reward)
        if args.test_sequential:
            from .vec_env import LBVecEnv
            env = LBVecEnv(1, device=args.device, seed=args.seed, as_tensors=True, **kw)
            res = run_sequential(agent, args.test_episodes, env)
        elif sweep_endpoints(args) is not None:
            kw.pop("num_endpoints")  # (the sweep's own)
            sweep = run_sweep(agent, num_endpoints=sweep_endpoints(args), n_episodes=args.test_episodes,
                              seed=args.seed, out_dir=".", device=args.device, **eval_launch_flags(args), **kw)
            res = None
            result["test_sweep"] = {}
            for e, r in sweep.items():
                print(f"num_endpoints {e}: mean return {float(r['r'].mean()):.6f}, wall {r['wall_s']:.3f} s")
                result["test_sweep"][str(e)] = {"mean_return": float(r["r"].mean()), "wall_s": float(r["wall_s"])}
        else:
            res = run_test(agent, n_episodes=args.test_episodes, seed=args.seed, device=args.device,
                           **eval_launch_flags(args), **kw)
        if res is not None:
            result["test_returns"] = [float(r) for r in res["r"]]
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
