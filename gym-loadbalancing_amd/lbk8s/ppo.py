"""GPU-resident PPO for the deep-sets agent.

Restates envs/ppo_deepset.py (CleanRL PPO, :53-300) on device tensors end to end:
rollout storage (T, B, ...) filled by LBVecEnv.step_device (obs written straight into
the storage slot, no host copies), GAE (:192-205), flattened minibatches, clipped policy
and value losses, entropy bonus, advantage normalisation per minibatch, clip_grad_norm,
Adam(eps=1e-5) (:216-267).  Hyper-parameter names and defaults are the reference's.
Reference quirk kept: actions are sampled WITHOUT masks during the rollout (:169; the
masks are all True anyway, :808-821) and the stored masks are used in the update.

Multi-GPU: one process per GPU, each with its own envs (LBVecEnv env_id_offset); the
gradients are averaged with one all_reduce per optimizer step (RCCL over xGMI) and the
logged episode return is the mean over every rank's finished episodes.

The minibatch step (loss, fused forward/backward, clip_grad_norm, Adam) is captured once
as HIP graphs and replayed per minibatch: ~200 launches per minibatch otherwise leave the
GPU waiting on the host between the fused kernels.  With several ranks the step is two
graphs — loss/backward ending in the gradients packed into one flat bucket, then
unpack/average + clip + Adam — with the bucket's all_reduce issued between them on the
same stream (the collective stays outside the captures, so any backend works).  The
capture's warm-up steps are undone (parameters and Adam state restored), so the graph path
computes the same update as the eager one.  The step, its bucket and its capture are
train_step.TrainStep, which DQN shares.

With fused_act and fused_bookkeeping a rollout's vector step is three launches (lb_ds_sample,
lb_step, lb_ppo_record) and GAE is one (lb_gae, gae_device); with fused_rollout the whole
rollout's vector steps are ONE launch (lb_ppo_steps, LBVecEnv.ppo_steps) where the env's shape has
it (E <= 16 below 32,768 envs, R <= 16), and with fused_rollout_e64 where lb_ppo_steps64 has it
(E <= 64 below 32,768 envs, R <= 65, Philox mode: config 4), and with fused_rollout_e256 where
lb_ppo_steps256 has it (E <= 256, R <= 257: the evaluation sweep's sizes).  All five flags are off by
default.

bootstrap_timeouts (off by default: the reference's behaviour) is partial-episode bootstrapping.
Every episode of this env ends at its time limit, a truncation, and the observation holds no step
index, so the reference's GAE trains the critic toward "return until a deadline it cannot see".
With the option, at a `done` the TD error bootstraps from the critic's value of the episode's
terminal observation (storage `term_values`, compute_gae_tl / gae_tl_device) and the lambda-chain
is still cut there.
"""
import os
import time
from typing import Optional

import torch
from torch import nn, optim

from . import _native
from . import dist as lbdist
from . import fused
from .deepsets import DeepSetAgent
from .train_step import TrainStep


def ppo_loss(agent, obs, actions, logprobs_old, masks, advantages, returns, values_old,
             clip_coef=0.2, ent_coef=0.01, vf_coef=0.5, norm_adv=True, clip_vloss=True):
    """One minibatch of ppo_deepset.py:227-263 -> (loss, pg_loss, v_loss, entropy, approx_kl, clipfrac).

    On a HIP device the deep-sets forward/backward are the fused training kernels and the
    loss head (log-softmax, ratio, clipped losses, entropy and their gradients) is one
    launch (fused_train.ppo_head); elsewhere, the same ops as the reference in torch."""
    from . import fused_train
    if (obs.is_cuda and torch.is_grad_enabled() and fused_train.supported(agent.actor.net, obs)
            and (masks is None or masks.shape[-1] == obs.shape[1])):
        logits, newvalue = agent.actor_critic(obs)
        adv = advantages
        if norm_adv:
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        loss, st = fused_train.ppo_head(logits, newvalue.view(-1), masks, actions, logprobs_old, adv, returns,
                                        values_old, clip_coef, ent_coef, vf_coef, clip_vloss)
        return loss, st[0], 0.5 * st[1], st[2], st[3], st[4]
    # the same Categorical ops as the reference: the actor's last Gamma term shifts every
    # logit of a set equally, so its true gradient is 0 and what autograd returns is
    # rounding noise that only an identical op sequence reproduces
    _, newlogprob, entropy, newvalue = agent.get_action_and_value(obs, actions.long(), masks)
    newvalue = newvalue.view(-1)
    logratio = newlogprob - logprobs_old
    ratio = logratio.exp()
    adv = advantages
    if norm_adv:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    pg_loss = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - clip_coef, 1 + clip_coef)).mean()
    if clip_vloss:
        v_unclipped = (newvalue - returns) ** 2
        v_clipped = values_old + torch.clamp(newvalue - values_old, -clip_coef, clip_coef)
        v_loss = 0.5 * torch.max(v_unclipped, (v_clipped - returns) ** 2).mean()
    else:
        v_loss = 0.5 * ((newvalue - returns) ** 2).mean()
    entropy_loss = entropy.mean()
    loss = pg_loss - ent_coef * entropy_loss + v_loss * vf_coef
    with torch.no_grad():
        approx_kl = ((ratio - 1) - logratio).mean()
        clipfrac = ((ratio - 1.0).abs() > clip_coef).float().mean()
    return loss, pg_loss, v_loss, entropy_loss, approx_kl, clipfrac


def compute_gae(rewards, values, dones, next_value, next_done, gamma, gae_lambda):
    """ppo_deepset.py:192-205 on (T, B) device tensors."""
    T = rewards.shape[0]
    advantages = torch.zeros_like(rewards)
    lastgaelam = torch.zeros_like(rewards[0])
    for t in reversed(range(T)):
        if t == T - 1:
            nextnonterminal = 1.0 - next_done
            nextvalues = next_value
        else:
            nextnonterminal = 1.0 - dones[t + 1]
            nextvalues = values[t + 1]
        delta = rewards[t] + gamma * nextvalues * nextnonterminal - values[t]
        lastgaelam = delta + gamma * gae_lambda * nextnonterminal * lastgaelam
        advantages[t] = lastgaelam
    return advantages, advantages + values


def compute_gae_tl(rewards, values, dones, next_value, next_done, term_values, gamma, gae_lambda):
    """compute_gae with the bootstrap at a time limit, on (T, B) device tensors: where step t ended
    the episode (dones[t + 1], or next_done at t = T - 1) the TD error takes term_values[t], the
    critic's value of the episode's terminal observation, in place of values[t + 1] (the next
    episode's first value); the lambda-chain is cut there as in compute_gae.  lb_gae_tl's
    expression order (include/lbk8s_abi_ppo_tl.h): compute_gae's bits with term_values zero, and
    with no done anywhere."""
    T = rewards.shape[0]
    advantages = torch.zeros_like(rewards)
    lastgaelam = torch.zeros_like(rewards[0])
    for t in reversed(range(T)):
        if t == T - 1:
            nextdone = next_done.reshape(-1)
            nextvalues = next_value.reshape(-1)
        else:
            nextdone = dones[t + 1]
            nextvalues = values[t + 1]
        nextnonterminal = 1.0 - nextdone
        bootstrap = torch.where(nextdone != 0, term_values[t], nextvalues)
        delta = rewards[t] + gamma * bootstrap - values[t]
        lastgaelam = delta + gamma * gae_lambda * nextnonterminal * lastgaelam
        advantages[t] = lastgaelam
    return advantages, advantages + values


def _gae_arg(name, t, shape, device, who="gae_device"):
    if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != shape
            or not t.is_contiguous() or t.device != device):
        raise ValueError(f"{who}: {name} must be a contiguous {shape} torch.float32 tensor on {device}")
    return t


@torch.no_grad()
def gae_device(rewards, values, dones, next_value, next_done, gamma, gae_lambda, out=None):
    """compute_gae in one launch (lb_gae): the same recurrence in float32, op for op, one thread
    per env -> (advantages, returns), (T, B) each.

    rewards, values, dones (T, B) and next_value, next_done with B elements (next_value may be
    (1, B), as update() shapes it): contiguous float32 tensors on one HIP device, else
    ValueError.  out = (advantages, returns) preallocated (T, B) tensors, distinct from each
    other and from the inputs (default: allocated here).  No host synchronisation; with `out`
    no allocation either, so the call can be captured in a HIP graph."""
    if not isinstance(rewards, torch.Tensor) or rewards.dim() != 2:
        raise ValueError("gae_device: rewards must be a (T, B) tensor")
    if rewards.device.type != "cuda":
        raise ValueError(f"gae_device: the tensors must be on a HIP device, not {rewards.device}")
    T, B = rewards.shape
    dev = rewards.device
    for name, t in (("rewards", rewards), ("values", values), ("dones", dones)):
        _gae_arg(name, t, (T, B), dev)
    for name, t in (("next_value", next_value), ("next_done", next_done)):
        if isinstance(t, torch.Tensor) and tuple(t.shape) == (1, B):
            t = t.view(B)
        _gae_arg(name, t, (B,), dev)
    if out is None:
        out = (torch.empty_like(rewards), torch.empty_like(rewards))
    adv, ret = out
    _gae_arg("out[0]", adv, (T, B), dev)
    _gae_arg("out[1]", ret, (T, B), dev)
    _native.check(_native.lib().lb_gae(
        rewards.data_ptr(), values.data_ptr(), dones.data_ptr(), next_value.data_ptr(), next_done.data_ptr(),
        T, B, float(gamma), float(gae_lambda), adv.data_ptr(), ret.data_ptr(),
        torch.cuda.current_stream(dev).cuda_stream))
    return adv, ret


@torch.no_grad()
def gae_tl_device(rewards, values, dones, next_value, next_done, term_values, gamma, gae_lambda, out=None):
    """compute_gae_tl in one launch (lb_gae_tl): gae_device's arguments, checks and conventions,
    plus term_values (T, B), a contiguous float32 tensor on the same device and distinct from the
    outputs."""
    who = "gae_tl_device"
    if not isinstance(rewards, torch.Tensor) or rewards.dim() != 2:
        raise ValueError(f"{who}: rewards must be a (T, B) tensor")
    if rewards.device.type != "cuda":
        raise ValueError(f"{who}: the tensors must be on a HIP device, not {rewards.device}")
    T, B = rewards.shape
    dev = rewards.device
    for name, t in (("rewards", rewards), ("values", values), ("dones", dones), ("term_values", term_values)):
        _gae_arg(name, t, (T, B), dev, who)
    for name, t in (("next_value", next_value), ("next_done", next_done)):
        if isinstance(t, torch.Tensor) and tuple(t.shape) == (1, B):
            t = t.view(B)
        _gae_arg(name, t, (B,), dev, who)
    if out is None:
        out = (torch.empty_like(rewards), torch.empty_like(rewards))
    adv, ret = out
    _gae_arg("out[0]", adv, (T, B), dev, who)
    _gae_arg("out[1]", ret, (T, B), dev, who)
    _native.check(_native.lib().lb_gae_tl(
        rewards.data_ptr(), values.data_ptr(), dones.data_ptr(), next_value.data_ptr(), next_done.data_ptr(),
        term_values.data_ptr(), T, B, float(gamma), float(gae_lambda), adv.data_ptr(), ret.data_ptr(),
        torch.cuda.current_stream(dev).cuda_stream))
    return adv, ret


class PPO_DeepSets:
    def __init__(self, env, learning_rate: float = 2.5e-4, anneal_lr: bool = False, num_steps: int = 128,
                 gae: bool = True, gae_lambda: float = 0.97, gamma: float = 0.95, n_minibatches: int = 4,
                 update_epochs: int = 4, norm_adv: bool = True, clip_coef: float = 0.2,
                 clip_vloss: bool = True, ent_coef: float = 0.01, vf_coef: float = 0.5,
                 max_grad_norm: float = 0.5, target_kl: Optional[float] = None, seed: int = 1,
                 device=None, log_fn=None, num_envs=None, tensorboard_log=None, use_graphs=None,
                 fused_act: bool = False, fused_bookkeeping: bool = False, fused_rollout: bool = False,
                 fused_rollout_e64: bool = False, fused_rollout_e256: bool = False,
                 bootstrap_timeouts: bool = False):
        # fused_act: the rollout's policy step as ONE launch (fused.deepsets_sample) that writes the
        # env's action buffer and the step's storage rows (actions, logprobs, values) directly.  Off
        # by default: a draw on a CDF boundary can pick the neighbouring row (and u = 0 never picks
        # an invalid one), which changes learner trajectories.
        # fused_bookkeeping: the rest of the rollout step (the done row of the storage, the finished
        # episodes' sums, the VecMonitor log) as ONE launch (LBVecEnv.record_ppo) and GAE as one
        # launch (gae_device) instead of eager torch arithmetic.  Same storage, advantages and
        # monitor file, bit for bit; the logged mean return sums per-env float64 accumulators, so
        # it can differ from the default's in the last bits.  Off by default, as fused_act.
        # fused_rollout: the T vector steps of a rollout as ONE launch (LBVecEnv.ppo_steps): each
        # wave takes its envs through every step, the observations in LDS and the env in registers.
        # The same storage, advantages and monitor file as fused_act + fused_bookkeeping, bit for
        # bit, whose buffers it implies.  Effective where the sampling forward covers the agent,
        # the env has the one-launch shape (ppo_steps_supported) and the device is HIP; elsewhere
        # the attribute reads False and the other two flags decide.  Off by default.
        # fused_rollout_e64: fused_rollout through LBVecEnv.ppo_steps64, whose shapes reach 64
        # endpoints (ppo_steps64_supported: R <= 65 below 32,768 envs, Philox mode); where it holds,
        # fused_rollout reads True.  fused_rollout alone keeps its 16-lane meaning.  Off by default.
        # fused_rollout_e256: the same through LBVecEnv.ppo_steps256, whose shapes reach 256 endpoints
        # (ppo_steps256_supported: R <= 257; a superset: it serves E <= 64 too and takes precedence
        # where both are on).  Off by default.
        # bootstrap_timeouts: at a `done` (always a time limit here) the value target bootstraps from
        # the critic's value of the terminal observation (storage term_values (T, B), filled during
        # the rollout; compute_gae_tl / gae_tl_device in update()).  The one-launch rollout is then
        # LBVecEnv.ppo_steps_tl, which has lb_ppo_steps' shapes: with any fused_rollout* flag on and
        # ppo_steps_supported, fused_rollout reads True and the other two False; on every other
        # shape the per-step path runs (one more launch per step, fused.deepsets_value_where, or its
        # torch equivalent where the fused forward does not cover the agent).  Off by default: the
        # reference treats every done as a true terminal.
        # num_envs / tensorboard_log: accepted for signature compatibility with
        # ppo_deepset.py:53-75 (the env's num_envs is used; there is no tensorboard writer)
        self.env = env
        self.device = torch.device(device) if device is not None else env.device
        self.num_envs = env.num_envs
        self.learning_rate, self.anneal_lr, self.num_steps = learning_rate, anneal_lr, num_steps
        self.gae, self.gae_lambda, self.gamma = gae, gae_lambda, gamma
        self.n_minibatches, self.update_epochs, self.norm_adv = n_minibatches, update_epochs, norm_adv
        self.clip_coef, self.clip_vloss, self.ent_coef, self.vf_coef = clip_coef, clip_vloss, ent_coef, vf_coef
        self.max_grad_norm, self.target_kl, self.seed = max_grad_norm, target_kl, seed
        self.batch_size = int(self.num_envs * num_steps)
        self.minibatch_size = int(self.batch_size // n_minibatches)
        self.log_fn = log_fn or (lambda d: None)
        torch.manual_seed(seed)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(seed)
        self.agent = DeepSetAgent(env).to(self.device)
        self._multi = lbdist.is_multi()
        if self._multi:
            lbdist.broadcast_parameters(self.agent)  # replicas start from rank 0's weights
        if use_graphs is None:
            use_graphs = self.device.type == "cuda"
        # a captured step needs equal minibatches and a device-side Adam step / lr
        self.use_graphs = bool(use_graphs) and self.batch_size % self.minibatch_size == 0
        if self.use_graphs:
            self._lr = torch.tensor(float(learning_rate), device=self.device)
            # torch's fused (single multi-tensor kernel) Adam: fewer launches per captured step
            self.optimizer = optim.Adam(self.agent.parameters(), lr=self._lr, eps=1e-5, capturable=True,
                                        fused=os.environ.get("LBK8S_FUSED_ADAM", "1") == "1")
        else:
            self.optimizer = optim.Adam(self.agent.parameters(), lr=learning_rate, eps=1e-5)
        # backward -> [gradient all_reduce] -> clip_grad_norm -> Adam, eager or captured
        self._ts = TrainStep(self.agent, self.optimizer, self.device, hook=self._clip)
        self._mb_graphs = None
        T, B = num_steps, self.num_envs
        R, A = env.observation_space.shape[0], env.action_space.n
        dev = self.device
        self.obs = torch.zeros((T, B, R, 8), device=dev)
        self.actions = torch.zeros((T, B), device=dev)
        self.masks = torch.ones((T, B, A), dtype=torch.bool, device=dev)
        self.logprobs = torch.zeros((T, B), device=dev)
        self.rewards = torch.zeros((T, B), device=dev)
        self.dones = torch.zeros((T, B), device=dev)
        self.values = torch.zeros((T, B), device=dev)
        self._last_obs = torch.zeros((B, R, 8), device=dev)  # obs after the last rollout step
        self._act = torch.zeros(B, dtype=torch.int32, device=dev)
        self._done_u8 = torch.zeros(B, dtype=torch.uint8, device=dev)
        self.episode_returns = []
        self._ep_sum = torch.zeros((), dtype=torch.float64, device=dev)
        self._ep_cnt = torch.zeros((), dtype=torch.float64, device=dev)
        # the rollout's categorical draws: T x B uniforms drawn in one call per rollout, the
        # samples by inverse CDF (no multinomial launch chain or host-synchronising check per
        # step).  Capturing the T steps as one HIP graph was measured (config 4: 19.5 ms per
        # rollout either way): the rollout is GPU-bound, so it runs eagerly.
        self._u = torch.zeros((T, B), device=dev)
        self.fused_act = bool(fused_act) and fused.sample_supported(self.agent, self.obs[0])
        self.fused_bookkeeping = bool(fused_bookkeeping) and dev.type == "cuda" and hasattr(env, "record_ppo")
        self.fused_rollout = (bool(fused_rollout) and dev.type == "cuda" and hasattr(env, "ppo_steps")
                              and fused.sample_supported(self.agent, self.obs[0]) and env.ppo_steps_supported(R))
        self.fused_rollout_e64 = (bool(fused_rollout_e64) and dev.type == "cuda" and hasattr(env, "ppo_steps64")
                                  and fused.sample_supported(self.agent, self.obs[0])
                                  and env.ppo_steps64_supported(R))
        self.fused_rollout_e256 = (bool(fused_rollout_e256) and dev.type == "cuda" and hasattr(env, "ppo_steps256")
                                   and fused.sample_supported(self.agent, self.obs[0])
                                   and env.ppo_steps256_supported(R))
        self.bootstrap_timeouts = bool(bootstrap_timeouts)
        if self.bootstrap_timeouts:  # the one-launch rollout with terminal values has lb_ppo_steps' shapes only
            self.fused_rollout = ((bool(fused_rollout) or bool(fused_rollout_e64) or bool(fused_rollout_e256))
                                  and dev.type == "cuda" and hasattr(env, "ppo_steps_tl")
                                  and fused.sample_supported(self.agent, self.obs[0]) and env.ppo_steps_supported(R))
            self.fused_rollout_e64 = self.fused_rollout_e256 = False
            self.term_values = torch.zeros((T, B), device=dev)
            # the per-step path's route, decided once: one launch where the fused forward covers the agent
            self._tv_fused = hasattr(env, "terminal_obs") and fused.sample_supported(self.agent, env.terminal_obs)
        self.fused_rollout = self.fused_rollout or self.fused_rollout_e64 or self.fused_rollout_e256
        if self.fused_rollout:  # (its buffers are fused_bookkeeping's; GAE in one launch too)
            self.fused_bookkeeping = True
        self.advantages = self.returns = None  # the last update()'s
        if self.fused_bookkeeping:
            self._ep_sum = torch.zeros(B, dtype=torch.float64, device=dev)  # per env (lb_ppo_record)
            self._ep_cnt = torch.zeros(B, dtype=torch.float64, device=dev)
            self._next_done = torch.zeros(B, device=dev)  # the done flags after the last step
            self._gae_out = (torch.zeros((T, B), device=dev), torch.zeros((T, B), device=dev))

    def _rollout_body(self, next_done):
        """The T vector steps on the storage buffers (no host sync, no RNG call: the uniforms
        are drawn before).  Returns the done flags after the last step."""
        env = self.env
        T = self.num_steps
        if self.fused_rollout:  # one launch (per monitor flush): every storage row, the sums, the log
            self.dones[0] = next_done
            agent = self.agent
            steps = (env.ppo_steps256 if self.fused_rollout_e256
                     else env.ppo_steps64 if self.fused_rollout_e64 else env.ppo_steps)
            tl = {}
            if self.bootstrap_timeouts:
                steps, tl = env.ppo_steps_tl, dict(term_values=self.term_values)
            steps(fused.packed(agent, agent.actor.net, agent.critic), self.obs[0], self._u, self.actions,
                  self.logprobs, self.values, self.rewards, self.obs[1:], self.dones[1:], self._last_obs,
                  self._next_done, self._act, self._done_u8, self._ep_sum, self._ep_cnt, **tl)
            return self._next_done
        next_obs = self.obs[0]
        fb = self.fused_bookkeeping
        if fb:  # record_ppo writes every later row
            self.dones[0] = next_done
        for step in range(T):
            if not fb:
                self.dones[step] = next_done
            if self.fused_act:  # one launch: the sample and its storage rows (no masks, :169)
                self.agent.act(next_obs, uniforms=self._u[step],
                               out=dict(actions_out=self._act, actions_f32_out=self.actions[step],
                                        logprob_out=self.logprobs[step], value_out=self.values[step]))
            else:
                action, logprob, value = self.agent.act(next_obs, uniforms=self._u[step])  # no masks (:169)
                self.values[step] = value
                self.actions[step] = action.float()
                self.logprobs[step] = logprob
                self._act.copy_(action)
            # the env writes the next observation straight into the next storage slot
            next_obs = self.obs[step + 1] if step + 1 < T else self._last_obs
            env.step_device(self._act, obs_out=next_obs, reward_out=self.rewards[step], done_out=self._done_u8)
            if self.bootstrap_timeouts:  # V(terminal observation) of the envs that finished, 0 elsewhere
                self._terminal_values(self.term_values[step])
            if fb:  # one launch: the next done row, the episode sums, the VecMonitor log
                next_done = self.dones[step + 1] if step + 1 < T else self._next_done
                env.record_ppo(self._done_u8, self.rewards[step], self._act, next_done, self._ep_sum, self._ep_cnt)
                continue
            env.record_episodes(self._done_u8, self.rewards[step], self._act)  # VecMonitor file, if any
            next_done = self._done_u8.float()
            # finished-episode returns accumulate on the device (no per-step host sync)
            self._ep_sum += (env.ep_stats[:, 0] * next_done).sum()
            self._ep_cnt += next_done.sum()
        return next_done

    def _terminal_values(self, out):
        """out (B,) = the critic's value of env.terminal_obs where the last step_device finished the
        env (self._done_u8), else 0: one launch where the fused forward covers the agent."""
        env = self.env
        if self._tv_fused:
            fused.deepsets_value_where(self.agent, env.terminal_obs, self._done_u8, out=out)
            return
        done = self._done_u8 != 0
        # (an unfinished env's terminal_obs row is stale or unwritten: it must not reach the output)
        x = torch.where(done.view(-1, 1, 1), env.terminal_obs, torch.zeros_like(env.terminal_obs))
        with torch.no_grad():
            v = self.agent.get_value(x).reshape(-1)
        out.copy_(torch.where(done, v, torch.zeros_like(v)))

    def rollout(self, next_obs, next_done):
        """Fill the (T, B) storage; returns the obs/done that follow the last step."""
        env = self.env
        if next_obs.data_ptr() != self.obs[0].data_ptr():
            self.obs[0].copy_(next_obs)
        torch.rand(self._u.shape, generator=self.gen, device=self.device, out=self._u)
        next_done = self._rollout_body(next_done)
        next_obs = self._last_obs
        env.flush_monitor()
        mean, _ = lbdist.mean_episode_return(self._ep_sum, self._ep_cnt)  # over every rank
        if mean is not None:
            self.episode_returns.append(mean)
        self._ep_sum.zero_()
        self._ep_cnt.zero_()
        return next_obs, next_done

    def _clip(self):
        nn.utils.clip_grad_norm_(self.agent.parameters(), self.max_grad_norm)

    def _mb_backward(self, *mb):
        """Loss and gradients of one minibatch (obs, actions, logprobs, masks, adv, ret, val)."""
        out = ppo_loss(self.agent, *mb, self.clip_coef, self.ent_coef, self.vf_coef, self.norm_adv, self.clip_vloss)
        self._ts.backward(out[0])
        return out

    def _minibatch_step(self, *mb):
        out = self._mb_backward(*mb)
        self._ts.allreduce()
        self._ts.apply()
        return out

    def _capture(self, src, mb):
        """Capture one minibatch step on static buffers (filled from minibatch `mb`)."""
        self._static = [torch.empty((self.minibatch_size,) + t.shape[1:], dtype=t.dtype, device=t.device)
                        for t in src]
        for d, t in zip(self._static, src):
            torch.index_select(t, 0, mb, out=d)
        self._mb_graphs, self._static_out = self._ts.capture(lambda: self._mb_backward(*self._static))

    def _replay(self):
        self._ts.replay(self._mb_graphs)

    def update(self, next_obs, next_done):
        with torch.no_grad():
            next_value = self.agent.get_value(next_obs).reshape(1, -1)
            if self.bootstrap_timeouts and self.fused_bookkeeping:
                advantages, returns = gae_tl_device(self.rewards, self.values, self.dones, next_value, next_done,
                                                    self.term_values, self.gamma, self.gae_lambda, out=self._gae_out)
            elif self.bootstrap_timeouts:
                advantages, returns = compute_gae_tl(self.rewards, self.values, self.dones, next_value, next_done,
                                                     self.term_values, self.gamma, self.gae_lambda)
            elif self.fused_bookkeeping:  # one launch into the preallocated buffers
                advantages, returns = gae_device(self.rewards, self.values, self.dones, next_value, next_done,
                                                 self.gamma, self.gae_lambda, out=self._gae_out)
            else:
                advantages, returns = compute_gae(self.rewards, self.values, self.dones, next_value, next_done,
                                                  self.gamma, self.gae_lambda)
        self.advantages, self.returns = advantages, returns
        R = self.obs.shape[2]
        b_obs = self.obs.reshape(-1, R, 8)
        b_logprobs = self.logprobs.reshape(-1)
        b_actions = self.actions.reshape(-1)
        b_masks = self.masks.reshape(-1, self.masks.shape[-1])
        b_adv, b_ret, b_val = advantages.reshape(-1), returns.reshape(-1), self.values.reshape(-1)
        src = (b_obs, b_actions, b_logprobs, b_masks, b_adv, b_ret, b_val)
        stats = {}
        for epoch in range(self.update_epochs):
            b_inds = torch.randperm(self.batch_size, device=self.device, generator=self.gen)
            for start in range(0, self.batch_size, self.minibatch_size):
                mb = b_inds[start:start + self.minibatch_size]
                if self.use_graphs:
                    if self._mb_graphs is None:
                        self._capture(src, mb)
                    for d, t in zip(self._static, src):
                        torch.index_select(t, 0, mb, out=d)
                    self._replay()
                    out = self._static_out
                else:
                    out = self._minibatch_step(*(t[mb] for t in src))
                loss, pg, vl, ent, kl, cf = out
            if self.target_kl is not None:
                # every rank takes the same decision (one rank leaving the epoch loop early
                # would skip collectives the others still issue): the mean kl over the ranks
                kl_all = kl.detach().clone()
                if self._multi:
                    lbdist.all_reduce_sum(kl_all)
                    kl_all /= torch.distributed.get_world_size()
                if kl_all > self.target_kl:
                    break
        if self.use_graphs:
            fused.invalidate(self.agent)  # replayed Adam steps do not move the version counters
        stats.update(loss=loss.item(), pg_loss=pg.item(), v_loss=vl.item(), entropy=ent.item(),
                     approx_kl=kl.item(), clipfrac=cf.item())
        return stats

    def learn(self, total_timesteps: int = 500000):
        env = self.env
        start = time.time()
        next_obs = env.reset()
        if not isinstance(next_obs, torch.Tensor):
            next_obs = env.obs
        next_done = torch.zeros(self.num_envs, device=self.device)
        num_updates = total_timesteps // self.batch_size
        global_step = 0
        for update in range(1, num_updates + 1):
            if self.anneal_lr:
                lr = (1.0 - (update - 1.0) / num_updates) * self.learning_rate
                if self.use_graphs:
                    self._lr.fill_(lr)  # the captured Adam step reads the lr tensor
                else:
                    self.optimizer.param_groups[0]["lr"] = lr
            next_obs, next_done = self.rollout(next_obs, next_done)
            global_step += self.batch_size
            stats = self.update(next_obs, next_done)
            stats.update(update=update, global_step=global_step,
                         sps=global_step / (time.time() - start),
                         ep_return=self.episode_returns[-1] if self.episode_returns else float("nan"))
            self.log_fn(stats)
        return self

    def predict(self, obs, masks=None):
        with torch.no_grad():
            x = torch.as_tensor(obs, dtype=torch.float32, device=self.device)
            m = None if masks is None else torch.as_tensor(masks, dtype=torch.bool, device=self.device)
            return self.agent.get_action(x, m, deterministic=True)

    def save(self, path):
        torch.save(self.agent.state_dict(), path)

    def load(self, path):
        self.agent.load_state_dict(torch.load(path, map_location=self.device, weights_only=True))
