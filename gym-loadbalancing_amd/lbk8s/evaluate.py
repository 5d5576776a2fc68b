"""Evaluation of trained deep-sets agents: run_test_deepset.py.

The reference (/root/reference/run_test_deepset.py:44-98) loads a PPO or DQN checkpoint
(`agent.load(path)`: a torch state_dict, ppo_deepset.py:296-300, dqn_deepset.py:227-231)
and plays `n_episodes` episodes on ONE env, one after the other, with deterministic
masked argmax actions (`agent.predict(obs, action_mask)`), while VecMonitor writes the
per-episode return and the info keywords.

Two forms:
* run_test: the episodes run side by side: `n_episodes` envs on the device, one vector
  step per time step: logits (PPO actor) or Q values (DQN) from the fused forward kernel,
  masked argmax, the fused env step.  Auto-reset is off, so every env plays exactly one
  episode (episode_length steps).  Episode i is the scenario of global env id
  `env_id_offset + i` (Philox), so any single episode can be replayed alone.
  With fused=True (the CLI's --test-fused) the whole episode is one launch (lb_eval_steps: the
  argmax inside the forward kernel, the env in registers) where the env's shape has it: at most
  16 observation rows, or with e64=True (--test-fused-e64, lb_eval_steps64) at most 65 (E <= 64),
  or with e256=True (--test-fused-e256, lb_eval_steps256) at most 257 (E <= 256), fewer than
  32,768 envs in every case.
* run_sweep: run_test_deepset.py:35-36's loop over the number of endpoints (a policy trained at 6
  endpoints played at SWEEP_ENDPOINTS), one run_test per entry, as one call.
* run_sequential: the reference loop as written — ONE env, episodes one after another,
  DummyVecEnv's auto-reset on done followed by the loop's own reset() (so the auto-reset's
  scenario is drawn and discarded), VecMonitor's float32 episode return.  Pinned by
  fixtures recorded from the reference env + the reference networks
  (tests/golden/gen_golden_eval.py) replayed in trace mode.
"""
import csv
import os
import time

import numpy as np
import torch

from . import fused
from .deepsets import HUGE_NEG, DeepSetAgent, DQNDeepSetAgent
from .info import INFO_KEYS, ST_LENGTH, ST_RETURN, info_matrix
from .vec_env import LBVecEnv

# run_test_deepset.py:19-57 (its env_kwargs' n_nodes is unused: NUM_NODES / NUM_ZONES win)
TEST_ENV = dict(num_nodes=48, num_zones=12, num_endpoints=6, rejection_allowed=True, arrival_rate_r=100,
                call_duration_r=1, episode_length=100, reward_function="multi", latency_weight=1.0,
                cpu_weight=0.0, gini_weight=0.0)


def load_agent(path, alg, in_channels=8, device="cuda"):
    """A reference checkpoint (torch state_dict) -> DeepSetAgent ("ppo") or DQNDeepSetAgent ("dqn")."""
    agent = (DeepSetAgent if alg == "ppo" else DQNDeepSetAgent)(in_channels).to(device)
    agent.load_state_dict(torch.load(path, map_location=device, weights_only=True))
    agent.eval()
    return agent


@torch.no_grad()
def greedy_actions(agent, obs, masks):
    """agent.predict(obs, masks) of ppo_deepset.py:289-294 / dqn_deepset.py: argmax of the
    masked logits (Categorical(logits).mode) or Q values; first index on ties."""
    if isinstance(agent, DeepSetAgent):
        scores, _ = fused.deepsets_forward(agent, obs)
    else:
        scores = fused.q_forward(agent, obs)
    scores = torch.where(masks, scores, torch.full((), HUGE_NEG, device=scores.device))
    return torch.argmax(scores, dim=1).to(torch.int32)


def eval_image(agent, device):
    """The actor-only weight image of a DeepSetAgent's actor or a DQNDeepSetAgent's Q network (the
    same module) in a fixed buffer, as fused.q_argmax_graphable packs it: what lb_eval_steps reads.
    Returns (the module, the image)."""
    net = agent.actor if isinstance(agent, DeepSetAgent) else agent.q_network
    frag = fused.pack_net_into(net.net, fused.frag_buffer(device))
    return net, frag


@torch.no_grad()
def run_test(agent, n_episodes=2000, seed=42, env_id_offset=0, device="cuda", monitor_path=None, fused=False,
             return_trace=False, e64=False, e256=False, **env_kwargs):
    """Play n_episodes greedy episodes in parallel -> dict of per-episode numpy arrays:
    "r" return, "l" length, the 12 numeric info keys of the final step, and "wall_s".

    fused: False, one forward, masked argmax and env step per time step, issued from Python; True,
    the whole episode in one launch (LBVecEnv.eval_steps; ValueError where the shape has none);
    None, the launch where it is supported, else the loop.  The launch takes the argmax inside
    the forward kernel, the loop torch's argmax of the forward's scores: a float32 near-tie may
    resolve differently.  return_trace: also "actions" / "rewards" / "dones" (L, n), every step's.
    e64: the one launch is LBVecEnv.eval_steps64 (up to 64 endpoints: eval_steps64_supported) in
    place of eval_steps; fused=True / None then ask that query.  False: eval_steps in every case.
    e256: the one launch is LBVecEnv.eval_steps256 (up to 256 endpoints: eval_steps256_supported), in
    place of either; fused=True / None then ask that query.  False: as above in every case."""
    kw = dict(TEST_ENV)
    kw.update(env_kwargs)
    env = LBVecEnv(n_episodes, device=device, seed=seed, env_id_offset=env_id_offset, auto_reset=False,
                   as_tensors=True, **kw)
    L = env.cfg.episode_length
    if fused or fused is None:
        why = _no_one_launch(agent, env, e64, e256)
        if why and fused:
            raise ValueError(f"run_test(fused=True): {why}")
        fused = not why
    obs = env.reset()
    masks = env.action_masks()
    trace = None
    if return_trace:
        trace = (torch.empty((L, n_episodes), dtype=torch.int32, device=env.device),
                 torch.empty((L, n_episodes), dtype=torch.float32, device=env.device),
                 torch.empty((L, n_episodes), dtype=torch.uint8, device=env.device))
    if fused:
        t0 = time.time()
        _, frag = eval_image(agent, env.device)
        # (every action is always valid: action_masks() is all True, so no mask is passed; eval_steps
        # plays an episode longer than LB_EVAL_STEPS_MAX in launches of that many steps)
        launch = env.eval_steps256 if e256 else (env.eval_steps64 if e64 else env.eval_steps)
        launch(frag, obs, L, None, *(trace or ()))
    else:
        t0 = time.time()
        for i in range(L):
            obs, _, _, _ = env.step(greedy_actions(agent, obs, masks))
            if trace is not None:
                trace[0][i].copy_(env.actions)
                trace[1][i].copy_(env.rewards)
                trace[2][i].copy_(env.dones)
    st = env.stats().cpu().numpy()
    wall = time.time() - t0
    info = info_matrix(st, env.rewards.cpu().numpy(), env.actions.cpu().numpy())
    out = {"r": st[:, ST_RETURN].copy(), "l": st[:, ST_LENGTH].astype(np.int64), "wall_s": wall}
    for j, k in enumerate(INFO_KEYS[:12]):
        out[k] = info[:, j]
    if monitor_path is not None:
        write_monitor_csv(monitor_path, out, INFO_KEYS[:12])
    if trace is not None:
        out["actions"], out["rewards"] = trace[0].cpu().numpy(), trace[1].cpu().numpy()
        out["dones"] = trace[2].cpu().numpy().astype(bool)
    return out


def _no_one_launch(agent, env, e64=False, e256=False):
    """Why run_test cannot play `env` with `agent` in one launch (None: it can); e64: the launch
    is eval_steps64; e256: it is eval_steps256."""
    net = (agent.actor if isinstance(agent, DeepSetAgent) else agent.q_network).net
    if not fused._geometry_ok(net, env.obs):
        return f"the fused forward does not cover this agent on {tuple(env.obs.shape)} observations"
    if e256:
        if not env.eval_steps256_supported(env.obs.shape[1]):
            return (f"no one-launch evaluation for {env.num_envs} envs of {env.cfg.num_endpoints} endpoints "
                    "(eval_steps256_supported: at most 257 observation rows, fewer than 32,768 envs)")
        return None
    if e64:
        if not env.eval_steps64_supported(env.obs.shape[1]):
            return (f"no one-launch evaluation for {env.num_envs} envs of {env.cfg.num_endpoints} endpoints "
                    "(eval_steps64_supported: at most 65 observation rows, fewer than 32,768 envs)")
        return None
    if not env.eval_steps_supported(env.obs.shape[1]):
        return (f"no one-launch evaluation for {env.num_envs} envs of {env.cfg.num_endpoints} endpoints "
                "(eval_steps_supported: at most 16 observation rows, fewer than 32,768 envs)")
    return None


# run_test_deepset.py:35-36: the numbers of endpoints a policy trained at 6 is evaluated at
SWEEP_ENDPOINTS = (6, 12, 16, 24, 32, 48, 64, 80, 128, 150, 180)


def sweep_monitor_name(i, e):
    """The i-th sweep entry's VecMonitor file (run_test_deepset.py:57's name)."""
    return f"{i}_loadbalancer_gym_results_num_endpoints_{e}.monitor.csv"


def run_sweep(agent, num_endpoints=SWEEP_ENDPOINTS, n_episodes=2000, seed=42, out_dir=None, fused=False, e64=False,
              e256=False, **env_kwargs):
    """The reference's evaluation sweep: for the i-th entry e of num_endpoints, run_test with
    num_endpoints=e, the same seed and the same fused / e64 / e256 / env_kwargs -> {e: run_test's
    dict}.  An entry equals that run_test call exactly.  out_dir: where entry i's VecMonitor file
    (sweep_monitor_name(i, e), through write_monitor_csv) goes; None writes none."""
    out = {}
    for i, e in enumerate(num_endpoints):
        path = os.path.join(out_dir, sweep_monitor_name(i, e)) if out_dir is not None else None
        out[e] = run_test(agent, n_episodes=n_episodes, seed=seed, monitor_path=path, fused=fused, e64=e64,
                          e256=e256, **dict(env_kwargs, num_endpoints=e))
    return out


@torch.no_grad()
def run_sequential(agent, n_episodes, env, draws=None, monitor_path=None, info_keywords=INFO_KEYS):
    """run_test_deepset.py:83-98 on a one-env LBVecEnv (auto_reset on, as DummyVecEnv):

        for episode: obs = envs.reset(); mask = env_method("action_masks")
                     while not done: obs, r, dones, info = envs.step(agent.predict(obs, mask))

    draws: None (Philox) or, for an env in trace mode, an object whose next_reset() /
    next_step() return the reference's draws for the next reset() / step() in call order
    (the step that ends an episode also consumes the auto-reset's).  Returns per-step
    "actions" / "rewards" / "dones" and per-episode "r" (VecMonitor's float32 return), "l",
    "total_reward" (float64) and the final info's keys."""
    if env.num_envs != 1 or not env.auto_reset:
        raise ValueError("run_sequential plays one env with auto-reset (DummyVecEnv of one env)")
    L = env.cfg.episode_length
    out = {k: [] for k in ("actions", "rewards", "dones", "r", "l", "total_reward")}
    for k in info_keywords:
        out[k] = []
    for _ in range(n_episodes):
        obs = env.reset(trace=draws.next_reset() if draws is not None else None)
        obs = torch.as_tensor(obs, device=env.device)
        masks = env.action_masks()
        done, ret32, length = False, np.float32(0.0), 0
        while not done:
            a = greedy_actions(agent, obs, masks)
            st = draws.next_step() if draws is not None else None
            rt = draws.next_reset() if (draws is not None and length + 1 == L) else None
            obs, rew, dones, infos = env.step(a, trace=st, reset_trace=rt)
            obs = torch.as_tensor(obs, device=env.device)
            r = float(np.asarray(rew.cpu() if isinstance(rew, torch.Tensor) else rew)[0])
            done = bool(np.asarray(dones.cpu() if isinstance(dones, torch.Tensor) else dones)[0])
            ret32 = np.float32(ret32 + np.float32(r))
            length += 1
            out["actions"].append(int(a[0]))
            out["rewards"].append(r)
            out["dones"].append(done)
            if done:
                info = infos[0]
                out["r"].append(float(ret32))
                out["l"].append(length)
                out["total_reward"].append(float(env._host_ep_stats()[0, ST_RETURN]))
                for k in info_keywords:
                    out[k].append(info[k])
    res = {k: np.asarray(v) for k, v in out.items()}
    if monitor_path is not None:
        res["wall_s"] = 0.0
        write_monitor_csv(monitor_path, res, info_keywords)
    return res


def write_monitor_csv(path, res, info_keywords):
    """VecMonitor's file layout: a '#' JSON header line, then r, l, t and the info keywords."""
    with open(path, "w", newline="") as f:
        f.write('#{"t_start": %.6f}\n' % time.time())
        w = csv.writer(f)
        w.writerow(["r", "l", "t"] + list(info_keywords))
        for i in range(len(res["r"])):
            w.writerow([round(float(res["r"][i]), 6), int(res["l"][i]), round(res["wall_s"], 6)]
                       + [res[k][i] for k in info_keywords])
