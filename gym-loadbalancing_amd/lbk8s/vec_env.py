"""LBVecEnv — drop-in SB3-style VecEnv over the HIP kernels.

Replaces `SubprocVecEnv([lambda: LoadBalancerK8sEnv(...)] * 8)` + `VecMonitor` of
run.py:95-127 for the callers envs/ppo_deepset.py:145-189 and envs/dqn_deepset.py:116-156:

    reset() -> obs (B, R, 8) float32
    step(actions) -> (obs, rewards (B,) float32, dones (B,) bool, infos: sequence of dicts)
    step_async / step_wait, env_method("action_masks"), get_attr, num_envs,
    observation_space, action_space, close(), seed()

Semantics (SB3 VecEnv, documented there, not pinned by the reference's tests):
auto-reset on done; infos[i]["terminal_observation"] holds the pre-reset obs; with
monitor=True infos[i]["episode"] = {"r", "l", "t"} plus the info_keywords copied from
the final info, like VecMonitor, and with monitor_file=name every finished episode is
appended to name.monitor.csv in VecMonitor's layout (run.py:122 wraps the training envs
in VecMonitor(env, "vec_loadbalancer_k8s_gym_results", info_keywords)).  `infos` is
lazy: a dict is built only when indexed (per-env Python dicts for 10^6 envs would cost
more than the step itself).  seed(s) is applied at the next reset() (SB3's convention;
the reference's own env.seed raises TypeError, loadbalancer_k8s_env.py:128,569).

Every buffer is a torch tensor on the HIP device; calls are asynchronous on torch's
current stream.  With as_tensors=True the step returns those device tensors (zero
copy); otherwise numpy copies (the reference callers wrap them in torch.Tensor()).
"""
import ctypes as C
import csv
import json
import os
import time

import numpy as np

from . import _native
from .config import LBConfig
from .info import ST_ACC, ST_EPISODE, ST_LENGTH, ST_RETURN, csv_rows, step_info

# trace array name -> (dtype, per-env length key)
_TRACE_SPEC = {
    "t0": ("f8", None), "step_x1": ("f8", None), "step_x2": ("f8", None), "step_r": ("i4", None),
    "step_n": ("i4", None), "reset_lat0": ("f8", "E"), "reset_topo": ("i4", "ZZ"),
    "reset_ntype": ("i4", "N"), "reset_nzone": ("i4", "N"), "reset_ncpu": ("i4", "N"),
    "reset_enode": ("i4", "E"), "reset_x1": ("f8", None), "reset_x2": ("f8", None),
    "reset_r": ("i4", None), "reset_n": ("i4", None),
}


class LazyInfos:
    """Sequence of per-env info dicts, materialised on access."""

    def __init__(self, env, rewards, actions, dones, monitor_t):
        self._env, self._r, self._a, self._d = env, rewards, actions, dones
        self._t = monitor_t
        self._stats = None
        self._cache = {}

    def __len__(self):
        return self._env.num_envs

    def __iter__(self):
        for i in range(len(self)):
            yield self[i]

    def _host(self):
        if not isinstance(self._r, np.ndarray):
            self._r = self._r.cpu().numpy()
            self._a = self._a.cpu().numpy()
            self._d = self._d.cpu().numpy().astype(bool)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(len(self)))]
        i = int(i)
        if i < 0:
            i += len(self)
        if i in self._cache:
            return self._cache[i]
        self._host()
        env = self._env
        if self._d[i] and env.auto_reset:  # ep_stats rows are written by the auto-reset
            st = env._host_ep_stats()[i]
        else:
            if self._stats is None:
                self._stats = env.stats().cpu().numpy()
            st = self._stats[i]
        info = step_info(st, float(self._r[i]), int(self._a[i]))
        if self._d[i] and env.auto_reset:
            info["terminal_observation"] = env._host_terminal_obs()[i]
            if env.monitor:  # (VecMonitor: the float32 running return)
                ep = {"r": float(env._host_ep_r32()[i]), "l": int(st[ST_LENGTH]),
                      "t": round(time.time() - env._t_start, 6)}
                for k in env.info_keywords:
                    ep[k] = info[k]
                info["episode"] = ep
        self._cache[i] = info
        return info


class _MonitorWriter:
    """VecMonitor's results file (SB3 ResultsWriter): a '#' JSON header line, then one row
    per finished episode: r, l, t (seconds since t_start) and the info keywords."""

    def __init__(self, filename, t_start, info_keywords):
        if not filename.endswith("monitor.csv"):
            filename = os.path.join(filename, "monitor.csv") if os.path.isdir(filename) else filename + ".monitor.csv"
        self.path = filename
        self.t_start = t_start
        self.keys = tuple(info_keywords)
        self.f = open(filename, "w", newline="")
        self.f.write("#" + json.dumps({"t_start": t_start, "env_id": "None"}) + "\n")
        self.w = csv.writer(self.f)
        self.w.writerow(["r", "l", "t"] + list(self.keys))
        self.f.flush()

    def write(self, rows, t):
        """rows: episode-log rows (lb_episode_log layout); t: host time of each row's step.
        'r' is VecMonitor's float32 running return."""
        for row, tt in zip(rows, t):
            info = step_info(row[:_native.LB_ST_K], float(row[_native.LB_EPLOG_REWARD]),
                             int(row[_native.LB_EPLOG_ACTION]))
            # VecMonitor writes its float32 running return as it stands (str of the float32,
            # no rounding; only the time is rounded to 6 places)
            r32 = np.float32(row[_native.LB_EPLOG_RET32])
            self.w.writerow([r32, int(row[ST_LENGTH]), round(tt - self.t_start, 6)]
                            + [info[k] for k in self.keys])
        self.f.flush()

    def close(self):
        self.f.close()


class LBVecEnv:
    """B vectorized LoadBalancerK8sEnv instances resident on one HIP device."""

    def __init__(self, num_envs, device=None, seed=0, env_id_offset=0, trace=False, t0=None,
                 auto_reset=True, as_tensors=False, monitor=False, info_keywords=(),
                 save_csv=False, monitor_file=None, geometry="auto", **env_kwargs):
        import torch
        self.torch = torch
        self.cfg = LBConfig(**env_kwargs)
        self.num_envs = int(num_envs)
        if self.num_envs < 1:
            raise ValueError("num_envs must be >= 1")
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise RuntimeError("LBVecEnv runs on a HIP device (there is no CPU fallback)")
        self.trace_mode = bool(trace)
        self.auto_reset = bool(auto_reset)
        self.as_tensors = bool(as_tensors)
        self.monitor = bool(monitor) or monitor_file is not None
        self.info_keywords = tuple(info_keywords)
        self.geometry = geometry
        self.save_csv = bool(save_csv)
        self.env_id_offset = int(env_id_offset)
        self.observation_space = self.cfg.observation_space()
        self.action_space = self.cfg.action_space()
        self._c = self.cfg.to_c(seed, env_id_offset, auto_reset, trace, geometry)
        self._pending_seed = None
        self._L = _native.lib()
        nbytes = C.c_uint64()
        _native.check(self._L.lb_state_bytes(C.byref(self._c), self.num_envs, C.byref(nbytes)))
        B, R = self.num_envs, self.cfg.obs_rows
        dev = self.device
        self.state = torch.zeros(int(nbytes.value), dtype=torch.uint8, device=dev)
        self.obs = torch.zeros((B, R, 8), dtype=torch.float32, device=dev)
        self.terminal_obs = torch.zeros((B, R, 8), dtype=torch.float32, device=dev)
        self.rewards = torch.zeros(B, dtype=torch.float32, device=dev)
        self.dones = torch.zeros(B, dtype=torch.uint8, device=dev)
        self.ep_stats = torch.zeros((B, _native.LB_ST_K), dtype=torch.float64, device=dev)
        self.actions = torch.zeros(B, dtype=torch.int32, device=dev)
        self._flags = torch.zeros(1, dtype=torch.int32, device=dev)
        self._trace_bufs = {}
        self._trace = _native.LBTraceC()
        self._pending = None
        self._reset_called = False
        self._episode_count = 0
        self._t_start = time.time()
        self._host_cache = {}
        self._monitor = _MonitorWriter(monitor_file, self._t_start, self.info_keywords) if monitor_file else None
        # the float64 rewards of the last lb_step, inside the state blob (lb_reward64): VecMonitor
        # adds them to its float32 returns with one rounding (lb_episode_log)
        ptr = C.c_void_p()
        _native.check(self._L.lb_reward64(self._ptr(self.state), C.byref(self._c), B, C.byref(ptr)))
        self._rew64 = ptr
        if self.monitor:  # VecMonitor: float32 running returns and the device episode log
            self._ret32 = torch.zeros(B, dtype=torch.float32, device=dev)
            self._ep_r32 = torch.zeros(B, dtype=torch.float32, device=dev)
            # an env finishes at most once per episode_length steps, so flushing every
            # min(64, L) steps never holds more than B rows
            self._log = torch.empty((B, _native.LB_EPLOG_W), dtype=torch.float64, device=dev)
            self._log_count = torch.zeros(1, dtype=torch.int32, device=dev)
            self._log_every = max(1, min(64, self.cfg.episode_length))
            self._log_times = []
        if self.trace_mode:
            if t0 is None:
                raise ValueError("trace mode needs t0 (current_time after __init__) per env")
            self._set_trace({"t0": t0})
        _native.check(self._L.lb_init(self._ptr(self.state), C.byref(self._c), B,
                                      C.byref(self._trace) if self.trace_mode else None, self._stream()))

    # ---- plumbing ---------------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    @staticmethod
    def _ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    def _set_trace(self, arrays):
        """Validate and upload injected draws (trace mode); keeps device copies alive."""
        cfg, B = self.cfg, self.num_envs
        sizes = {None: 1, "E": cfg.num_endpoints, "N": cfg.num_nodes,
                 "ZZ": cfg.num_zones * (cfg.num_zones - 1)}
        for name, arr in arrays.items():
            dt, per = _TRACE_SPEC[name]
            a = np.ascontiguousarray(np.asarray(arr).reshape(B, -1), dtype=dt)
            if a.shape[1] != sizes[per]:
                raise ValueError(f"trace {name}: expected {sizes[per]} values per env, got {a.shape[1]}")
            self._validate_trace(name, a)
            t = self.torch.from_numpy(a.reshape(-1)).to(self.device)
            self._trace_bufs[name] = t
            setattr(self._trace, name, t.data_ptr())

    def _validate_trace(self, name, a):
        # the kernels index tables with these values: reject what the reference's numpy
        # generator could never have produced
        cfg = self.cfg
        lim = {"reset_nzone": (0, 3), "reset_ntype": (0, 4), "reset_ncpu": (0, 127),
               "reset_enode": (0, min(23, cfg.num_nodes - 1)), "reset_topo": (0, 511),
               "step_r": (0, 6), "reset_r": (0, 6), "step_n": (0, cfg.num_nodes - 1),
               "reset_n": (0, cfg.num_nodes - 1)}
        if name in lim:
            lo, hi = lim[name]
            if a.size and (a.min() < lo or a.max() > hi):
                raise ValueError(f"trace {name} outside [{lo}, {hi}]")
        if name == "reset_lat0" and a.size and (a.min() < 0 or a.max() >= 501):
            raise ValueError("trace reset_lat0 outside [0, 501)")

    def _host_ep_stats(self):
        if "ep_stats" not in self._host_cache:
            self._host_cache["ep_stats"] = self.ep_stats.cpu().numpy()
        return self._host_cache["ep_stats"]

    def _host_ep_r32(self):
        if "r32" not in self._host_cache:
            self._host_cache["r32"] = self._ep_r32.cpu().numpy()
        return self._host_cache["r32"]

    def _host_terminal_obs(self):
        if "term" not in self._host_cache:
            self._host_cache["term"] = self.terminal_obs.cpu().numpy()
        return self._host_cache["term"]

    def _out(self, t):
        return t if self.as_tensors else t.cpu().numpy()

    # ---- VecEnv API -----------------------------------------------------------------------------
    def reset(self, trace=None):
        """reset() of every env (loadbalancer_k8s_env.py:290-400) -> obs (B, R, 8) float32."""
        if self._pending_seed is not None:  # seed() takes effect here, for every env at once
            self._c.seed = self._pending_seed
            self._pending_seed = None
        if self.trace_mode:
            if trace is None:
                raise ValueError("trace mode: reset() needs the reset draws")
            self._set_trace({"reset_" + k: v for k, v in trace.items()})
        _native.check(self._L.lb_reset(self._ptr(self.state), C.byref(self._c), self.num_envs, None,
                                       self._ptr(self.obs),
                                       C.byref(self._trace) if self.trace_mode else None, self._stream()))
        self._reset_called = True
        return self._out(self.obs)

    def step_async(self, actions, trace=None, reset_trace=None):
        self._pending = (actions, trace, reset_trace)

    def step_wait(self):
        if self._pending is None:
            raise RuntimeError("step_wait() without step_async()")
        actions, trace, reset_trace = self._pending
        self._pending = None
        return self._step(actions, trace, reset_trace)

    def step(self, actions, trace=None, reset_trace=None):
        return self._step(actions, trace, reset_trace)

    def _step(self, actions, trace, reset_trace):
        torch = self.torch
        if not self._reset_called:
            # the reference raises TypeError here (node_type is a float array until reset)
            raise TypeError("step() called before reset()")
        if isinstance(actions, torch.Tensor):
            a = actions.reshape(-1).to(device=self.device, dtype=torch.int32)
        else:
            a = torch.from_numpy(np.ascontiguousarray(np.asarray(actions).reshape(-1), np.int32)).to(self.device)
        if a.numel() != self.num_envs:
            raise ValueError(f"expected {self.num_envs} actions, got {a.numel()}")
        self.actions.copy_(a)
        if self.trace_mode:
            if trace is None:
                raise ValueError("trace mode: step() needs the step draws")
            self._set_trace({"step_" + k: v for k, v in trace.items()})
            if reset_trace is not None:
                self._set_trace({"reset_" + k: v for k, v in reset_trace.items()})
        _native.check(self._L.lb_step(
            self._ptr(self.state), C.byref(self._c), self.num_envs, self._ptr(self.actions),
            self._ptr(self.obs), self._ptr(self.rewards), self._ptr(self.dones),
            self._ptr(self.terminal_obs), self._ptr(self.ep_stats),
            C.byref(self._trace) if self.trace_mode else None, self._stream()))
        self._host_cache = {}
        dones_b = self.dones.bool()
        infos = LazyInfos(self, self.rewards, self.actions, self.dones, self._t_start)
        if self.save_csv:
            self._write_csv()
        if self.monitor:
            self.record_episodes()
            self.flush_monitor()
        if self.as_tensors:
            return self.obs, self.rewards, dones_b, infos
        obs = self.obs.cpu().numpy()
        rew = self.rewards.cpu().numpy()
        dn = dones_b.cpu().numpy()
        infos._r, infos._a, infos._d = rew, self.actions.cpu().numpy(), dn
        return obs, rew, dn, infos

    def _write_csv(self):
        dn = self.dones.cpu().numpy().astype(bool)
        if not dn.any():
            return
        st = self._host_ep_stats()
        with open(self.cfg.file_results_name + ".csv", "a+", newline="") as f1, \
                open("no_cost_updated.csv", "a+", newline="") as f2:
            w1 = csv.DictWriter(f1, fieldnames=list(csv_rows(st[0], 0)[0].keys()))
            w2 = csv.DictWriter(f2, fieldnames=list(csv_rows(st[0], 0)[1].keys()))
            for i in np.flatnonzero(dn):
                self._episode_count += 1
                r1, r2 = csv_rows(st[i], int(st[i, ST_EPISODE]))
                w1.writerow(r1)
                w2.writerow(r2)

    def env_method(self, method_name, *args, indices=None, **kwargs):
        idx = self._indices(indices)
        if method_name == "action_masks":
            # loadbalancer_k8s_env.py:808-821: every action is always valid
            return [np.ones(self.cfg.num_actions, dtype=bool) for _ in idx]
        raise AttributeError(f"LBVecEnv has no env method {method_name!r}")

    def action_masks(self):
        """(B, A) bool device tensor, all True (the batched form of env_method('action_masks'))."""
        return self.torch.ones((self.num_envs, self.cfg.num_actions), dtype=self.torch.bool,
                               device=self.device)

    def get_attr(self, attr_name, indices=None):
        idx = self._indices(indices)
        if attr_name in _native.LB_FIELD:
            vals = self.field(attr_name).cpu().numpy()
            return [vals[i] for i in idx]
        v = getattr(self.cfg, attr_name)
        return [v for _ in idx]

    def set_attr(self, attr_name, value, indices=None):
        raise AttributeError("LBVecEnv attributes are device state; set them through reset()")

    def _indices(self, indices):
        if indices is None:
            return range(self.num_envs)
        if isinstance(indices, int):
            return [indices]
        return indices

    def seed(self, seed=None):
        """Re-key the Philox stream at the next reset() (SB3 VecEnv convention).

        Until then every env keeps its current key, auto-resets included: an episode never
        mixes two keys (the step may redraw the current episode's scenario from the key)."""
        self._pending_seed = int(seed or 0) & (2**64 - 1)
        return [seed] * self.num_envs

    def close(self):
        if self._monitor is not None:
            self.flush_monitor()
            self._monitor.close()
        self.state = None

    # ---- VecMonitor file ------------------------------------------------------------------------
    def _check_tensors(self, who, spec):
        """Each (name, tensor, shape, dtype, optional) of spec: a contiguous tensor of that shape and
        dtype on the env's device, or None where optional."""
        t, dev = self.torch, self.ep_stats.device
        for name, x, shape, dt, optional in spec:
            if x is None and optional:
                continue
            if (not isinstance(x, t.Tensor) or x.dtype != dt or tuple(x.shape) != shape or not x.is_contiguous()
                    or x.device != dev):
                raise ValueError(f"{who}: {name} must be a contiguous {shape} {dt} tensor on {dev}")

    def _log_args(self):
        """The episode-log arguments of a launch (ret32, ep_r32, its first step's tag, log, cap,
        count); all empty for an env that is not monitored."""
        if not self.monitor:
            return (None, None, 0, None, 0, None)
        return (self._ptr(self._ret32), self._ptr(self._ep_r32), len(self._log_times), self._ptr(self._log),
                self.num_envs, self._ptr(self._log_count))

    def _logged(self, n=1):
        """n vector steps were logged: their host times, and the flush when it is due."""
        if not self.monitor:
            return
        self._log_times.extend(time.time() for _ in range(n))
        if len(self._log_times) >= self._log_every:
            self.flush_monitor()

    def _launches(self, T, most):
        """(i, n) of the launches of a request of T steps, at most `most` each: launch i .. i + n - 1
        is the rest of the request, or ends where a flush is due (the caller reports each launch
        with _logged(n); within that many steps an env finishes at most once, so the log cannot
        overflow)."""
        i = 0
        while i < T:
            n = min(T - i, most)
            if self.monitor:
                n = min(n, self._log_every - len(self._log_times))
            yield i, n
            i += n

    def record_episodes(self, dones=None, rewards=None, actions=None):
        """VecMonitor bookkeeping of the last vector step, on the device: the float32 running
        returns and, for the finished envs only, their rows appended to the episode log
        (lb_episode_log; nothing per env crosses to the host).  The device learners call this
        after every step_device with the buffers they passed it; the drop-in step() does it
        itself.  The host reads the log at flush_monitor (every min(64, L) steps)."""
        if not self.monitor:
            return
        d = self.dones if dones is None else dones
        r = self.rewards if rewards is None else rewards
        a = self.actions if actions is None else actions
        _native.check(self._L.lb_episode_log(
            self.num_envs, self._ptr(d), self._ptr(self.ep_stats), self._ptr(r), self._rew64, self._ptr(a),
            *self._log_args(), self._stream()))
        self._logged()

    def record_ppo(self, dones, rewards, actions, next_done_out, ep_sum, ep_cnt):
        """PPO's bookkeeping of the last vector step in one launch (lb_ppo_record): the done
        flags as float32 into next_done_out (B,) (the next row of the learner's `dones`
        storage), the finished envs' returns added to the per-env float64 accumulators ep_sum /
        ep_cnt (B,), and everything record_episodes does (the episode-log append, its step time
        and the flush cadence) when the env is monitored; no log otherwise."""
        t = self.torch
        B = self.num_envs
        self._check_tensors("record_ppo", [
            (name, x, (B,), dt, False)
            for name, x, dt in (("dones", dones, t.uint8), ("rewards", rewards, t.float32),
                                ("actions", actions, t.int32), ("next_done_out", next_done_out, t.float32),
                                ("ep_sum", ep_sum, t.float64), ("ep_cnt", ep_cnt, t.float64))])
        step = (self._ptr(rewards), self._rew64, self._ptr(actions)) if self.monitor else (None, None, None)
        _native.check(self._L.lb_ppo_record(
            B, self._ptr(dones), self._ptr(self.ep_stats), self._ptr(next_done_out), self._ptr(ep_sum),
            self._ptr(ep_cnt), *step, *self._log_args(), self._stream()))
        self._logged()

    def ppo_steps_supported(self, R):
        """Whether lb_ppo_steps (a PPO rollout's vector steps in one launch) covers this env with
        R-row observations."""
        return bool(self._L.lb_ppo_steps_supported(C.byref(self._c), self.num_envs, R))

    def ppo_steps64_supported(self, R):
        """Whether lb_ppo_steps64 (ppo_steps for envs of up to 64 endpoints: R <= 65 below 32,768
        envs, Philox mode) covers this env with R-row observations; true wherever
        ppo_steps_supported is."""
        return bool(self._L.lb_ppo_steps64_supported(C.byref(self._c), self.num_envs, R))

    def ppo_steps64(self, frag, obs, uniforms, actions_f32, logprobs, values, rewards, obs_next, dones_next,
                    last_obs, last_done, actions, dones, ep_sum, ep_cnt):
        """lb_ppo_steps64: ppo_steps, argument for argument, on the shapes of ppo_steps64_supported
        (config 4's E = 64, R = 65 among them); on a shape ppo_steps covers, the same kernel."""
        return self._ppo_steps("ppo_steps64", self._L.lb_ppo_steps64, frag, obs, uniforms, actions_f32, logprobs,
                               values, rewards, obs_next, dones_next, last_obs, last_done, actions, dones, ep_sum,
                               ep_cnt)

    def ppo_steps256_supported(self, R):
        """Whether lb_ppo_steps256 (ppo_steps for envs of up to 256 endpoints: R <= 257 below 32,768
        envs, Philox mode) covers this env with R-row observations; true wherever
        ppo_steps64_supported is."""
        return bool(self._L.lb_ppo_steps256_supported(C.byref(self._c), self.num_envs, R))

    def ppo_steps256(self, frag, obs, uniforms, actions_f32, logprobs, values, rewards, obs_next, dones_next,
                     last_obs, last_done, actions, dones, ep_sum, ep_cnt):
        """lb_ppo_steps256: ppo_steps, argument for argument, on the shapes of ppo_steps256_supported
        (the evaluation sweep's 80, 128, 150 and 180 endpoints among them); on a shape ppo_steps64
        covers, that entry point's kernel."""
        return self._ppo_steps("ppo_steps256", self._L.lb_ppo_steps256, frag, obs, uniforms, actions_f32, logprobs,
                               values, rewards, obs_next, dones_next, last_obs, last_done, actions, dones, ep_sum,
                               ep_cnt)

    def ppo_steps(self, frag, obs, uniforms, actions_f32, logprobs, values, rewards, obs_next, dones_next,
                  last_obs, last_done, actions, dones, ep_sum, ep_cnt):
        """lb_ppo_steps: T = uniforms.shape[0] PPO vector steps -- each fused.deepsets_sample on the
        weight image `frag` (no masks), step_device and record_ppo -- in one launch, bit for bit
        those 3 T launches.  obs (B, R, 8) is the first step's input; uniforms, actions_f32,
        logprobs, values and rewards are (T, B) float32; step i's next observation / done row go to
        obs_next[i] / dones_next[i] (S, B, R, 8) / (S, B) for i < S, S = T or T - 1, else to
        last_obs (B, R, 8) / last_done (B,) (required when S = T - 1, else None).  actions (B,)
        int32 and dones (B,) uint8 end as the last step leaves them; ep_sum / ep_cnt (B,) float64
        as record_ppo's.  A monitored env logs every step with its own host time and flushes at
        record_ppo's cadence: the request is split into launches that end where a flush is due
        (within that many steps an env finishes at most once, so the log cannot overflow)."""
        return self._ppo_steps("ppo_steps", self._L.lb_ppo_steps, frag, obs, uniforms, actions_f32, logprobs, values,
                               rewards, obs_next, dones_next, last_obs, last_done, actions, dones, ep_sum, ep_cnt)

    def ppo_steps_tl_supported(self, R):
        """Whether lb_ppo_steps_tl (ppo_steps with the terminal values) covers this env with R-row
        observations: ppo_steps_supported's answer."""
        return bool(self._L.lb_ppo_steps_tl_supported(C.byref(self._c), self.num_envs, R))

    def ppo_steps_tl(self, frag, obs, uniforms, actions_f32, logprobs, values, rewards, obs_next, dones_next,
                     last_obs, last_done, actions, dones, ep_sum, ep_cnt, term_values):
        """lb_ppo_steps_tl: ppo_steps, argument for argument, and the rollout's terminal values.  Each
        step's lb_step also writes the finished envs' pre-reset observations to self.terminal_obs,
        and row i of term_values (T, B) float32 is fused.deepsets_value_where(frag's agent,
        terminal_obs, step i's dones): the critic's value of the terminal observation of the envs
        that finished in step i, +0.0 for the rest -- bit for bit that launch after every step.
        self.terminal_obs ends as every env's last terminal observation (untouched for an env that
        never finished).  The shapes of ppo_steps_supported; split at the monitor's flushes as
        ppo_steps."""
        return self._ppo_steps("ppo_steps_tl", self._L.lb_ppo_steps_tl, frag, obs, uniforms, actions_f32, logprobs,
                               values, rewards, obs_next, dones_next, last_obs, last_done, actions, dones, ep_sum,
                               ep_cnt, term_values=term_values)

    def _ppo_steps(self, who, entry, frag, obs, uniforms, actions_f32, logprobs, values, rewards, obs_next,
                   dones_next, last_obs, last_done, actions, dones, ep_sum, ep_cnt, term_values=None):
        """ppo_steps / ppo_steps64 / ppo_steps256 / ppo_steps_tl (who: the method's name, entry: its
        library function; term_values: ppo_steps_tl's, whose entry takes terminal_obs and its rows
        before the stream)."""
        t = self.torch
        if not self._reset_called and not t.cuda.is_current_stream_capturing():
            raise TypeError("step() called before reset()")
        B = self.num_envs
        if not isinstance(uniforms, t.Tensor) or uniforms.dim() != 2 or uniforms.shape[0] < 1:
            raise ValueError(f"{who}: uniforms must be a (T, B) tensor with T >= 1")
        if not isinstance(obs, t.Tensor) or obs.dim() != 3:
            raise ValueError(f"{who}: obs must be a (B, R, 8) tensor")
        T, R = uniforms.shape[0], obs.shape[1]
        S = obs_next.shape[0] if isinstance(obs_next, t.Tensor) and obs_next.dim() == 4 else -1
        if S not in (T, T - 1):
            raise ValueError(f"{who}: obs_next must be a ({T} or {T - 1}, {B}, {R}, 8) tensor")
        last = S == T and last_obs is None and last_done is None  # (last_* optional: every row is stored)
        self._check_tensors(who, [
            ("frag", frag, (_native.LB_DS_FRAG_FLOATS,), t.float32, False), ("obs", obs, (B, R, 8), t.float32, False),
            ("uniforms", uniforms, (T, B), t.float32, False), ("actions_f32", actions_f32, (T, B), t.float32, False),
            ("logprobs", logprobs, (T, B), t.float32, False), ("values", values, (T, B), t.float32, False),
            ("rewards", rewards, (T, B), t.float32, False), ("obs_next", obs_next, (S, B, R, 8), t.float32, False),
            ("dones_next", dones_next, (S, B), t.float32, False), ("actions", actions, (B,), t.int32, False),
            ("dones", dones, (B,), t.uint8, False), ("ep_sum", ep_sum, (B,), t.float64, False),
            ("ep_cnt", ep_cnt, (B,), t.float64, False), ("last_obs", last_obs, (B, R, 8), t.float32, last),
            ("last_done", last_done, (B,), t.float32, last)])
        tl = who == "ppo_steps_tl"
        if tl:
            self._check_tensors(who, [("term_values", term_values, (T, B), t.float32, False),
                                      ("terminal_obs", self.terminal_obs, (B, R, 8), t.float32, False)])
        if not getattr(self, who + "_supported")(R):
            raise RuntimeError(f"{who}: the env's shape has no one-launch rollout ({who}_supported)")
        for i, n in self._launches(T, _native.LB_PPO_STEPS_MAX):
            s = min(n, S - i)  # rows of obs_next / dones_next this launch fills (n, or n - 1 at the end)
            src = obs if i == 0 else obs_next[i - 1]
            _native.check(entry(
                self._ptr(frag), self._ptr(src), self._ptr(self.state), C.byref(self._c), B, R, n, s,
                self._ptr(uniforms[i]), self._ptr(actions_f32[i]), self._ptr(logprobs[i]), self._ptr(values[i]),
                self._ptr(rewards[i]), self._ptr(obs_next[i]) if s else None,
                self._ptr(dones_next[i]) if s else None, self._ptr(last_obs) if s < n else None,
                self._ptr(last_done) if s < n else None, self._ptr(actions), self._ptr(dones),
                self._ptr(self.ep_stats), self._ptr(ep_sum), self._ptr(ep_cnt), *self._log_args(),
                *((self._ptr(self.terminal_obs), self._ptr(term_values[i])) if tl else ()), self._stream()))
            self._logged(n)

    def eval_steps_supported(self, R):
        """Whether lb_eval_steps (a greedy evaluation's vector steps in one launch) covers this env
        with R-row observations."""
        return bool(self._L.lb_eval_steps_supported(C.byref(self._c), self.num_envs, R))

    def eval_steps64_supported(self, R):
        """Whether lb_eval_steps64 (eval_steps for envs of up to 64 endpoints: R <= 65 below 32,768
        envs, Philox mode) covers this env with R-row observations; true wherever
        eval_steps_supported is."""
        return bool(self._L.lb_eval_steps64_supported(C.byref(self._c), self.num_envs, R))

    def eval_steps64(self, frag, obs, steps, masks=None, actions_all=None, rewards_all=None, dones_all=None,
                     ep_sum=None, ep_cnt=None):
        """lb_eval_steps64: eval_steps, argument for argument, on the shapes of eval_steps64_supported
        (E = 64 with the reject row among them); on a shape eval_steps covers, the same kernel."""
        return self._eval_steps("eval_steps64", self._L.lb_eval_steps64, frag, obs, steps, masks, actions_all,
                                rewards_all, dones_all, ep_sum, ep_cnt)

    def eval_steps256_supported(self, R):
        """Whether lb_eval_steps256 (eval_steps for envs of up to 256 endpoints: R <= 257 below
        32,768 envs, Philox mode) covers this env with R-row observations; true wherever
        eval_steps64_supported is."""
        return bool(self._L.lb_eval_steps256_supported(C.byref(self._c), self.num_envs, R))

    def eval_steps256(self, frag, obs, steps, masks=None, actions_all=None, rewards_all=None, dones_all=None,
                      ep_sum=None, ep_cnt=None):
        """lb_eval_steps256: eval_steps, argument for argument, on the shapes of
        eval_steps256_supported (the evaluation sweep's 80, 128, 150 and 180 endpoints among them);
        on a shape eval_steps64 covers, that entry point's kernel."""
        return self._eval_steps("eval_steps256", self._L.lb_eval_steps256, frag, obs, steps, masks, actions_all,
                                rewards_all, dones_all, ep_sum, ep_cnt)

    def eval_steps(self, frag, obs, steps, masks=None, actions_all=None, rewards_all=None, dones_all=None,
                   ep_sum=None, ep_cnt=None):
        """lb_eval_steps: `steps` greedy vector steps -- each the masked argmax of the actor-only
        weight image `frag` on obs (fused.q_argmax_graphable's forward), step_device and, for a
        monitored env or with ep_sum / ep_cnt, record_ppo's bookkeeping -- in one launch, bit for
        bit those launches.  obs (B, R, 8) float32 is updated in place: it ends as the observations
        after the last step.  masks (B, R) bool or None (all valid), fixed over the steps.  Step
        i's actions / rewards / dones go to row i of actions_all (steps, B) int32 / rewards_all
        (steps, B) float32 / dones_all (steps, B) uint8, each optional.  The env's own actions /
        rewards / dones / ep_stats buffers end as the last step leaves them; ep_sum / ep_cnt (B,)
        float64, both or neither, as record_ppo's.  A monitored env logs every step with its own
        host time and flushes at record_ppo's cadence: the request is split into launches that end
        where a flush is due.  Returns obs."""
        return self._eval_steps("eval_steps", self._L.lb_eval_steps, frag, obs, steps, masks, actions_all,
                                rewards_all, dones_all, ep_sum, ep_cnt)

    def _eval_steps(self, who, entry, frag, obs, steps, masks, actions_all, rewards_all, dones_all, ep_sum, ep_cnt):
        """eval_steps / eval_steps64 / eval_steps256 (who: the method's name, entry: its library function)."""
        t = self.torch
        if not self._reset_called and not t.cuda.is_current_stream_capturing():
            raise TypeError("step() called before reset()")
        B = self.num_envs
        T = int(steps)
        if T < 1:
            raise ValueError(f"{who}: steps must be >= 1")
        if not isinstance(obs, t.Tensor) or obs.dim() != 3:
            raise ValueError(f"{who}: obs must be a (B, R, 8) tensor")
        if (ep_sum is None) != (ep_cnt is None):
            raise ValueError(f"{who}: ep_sum and ep_cnt go together")
        R = obs.shape[1]
        self._check_tensors(who, [
            ("frag", frag, (_native.LB_DS_FRAG_FLOATS,), t.float32, False), ("obs", obs, (B, R, 8), t.float32, False),
            ("masks", masks, (B, R), t.bool, True), ("actions_all", actions_all, (T, B), t.int32, True),
            ("rewards_all", rewards_all, (T, B), t.float32, True), ("dones_all", dones_all, (T, B), t.uint8, True),
            ("ep_sum", ep_sum, (B,), t.float64, True), ("ep_cnt", ep_cnt, (B,), t.float64, True)])
        if not getattr(self, who + "_supported")(R):
            raise RuntimeError(f"{who}: the env's shape has no one-launch evaluation ({who}_supported)")
        for i, n in self._launches(T, _native.LB_EVAL_STEPS_MAX):
            row = lambda x: self._ptr(x[i]) if x is not None else None
            _native.check(entry(
                self._ptr(frag), self._ptr(obs), self._ptr(self.state), C.byref(self._c), B, R, self._ptr(masks), n,
                row(actions_all), row(rewards_all), row(dones_all), self._ptr(self.actions), self._ptr(self.rewards),
                self._ptr(self.dones), self._ptr(self.ep_stats), self._ptr(ep_sum), self._ptr(ep_cnt),
                *self._log_args(), self._stream()))
            self._logged(n)
        self._host_cache = {}
        return obs

    def flush_monitor(self):
        """Write the logged episodes (one host sync): in step order, env order within a step."""
        if not self.monitor or not self._log_times:
            return
        n = int(self._log_count.item())
        if n > self.num_envs:
            raise RuntimeError(f"episode log overflow ({n} rows > {self.num_envs})")
        rows = self._log[:n].cpu().numpy() if n else np.zeros((0, _native.LB_EPLOG_W))
        order = np.lexsort((rows[:, _native.LB_EPLOG_ENV], rows[:, _native.LB_EPLOG_TAG]))
        rows = rows[order]
        if self._monitor is not None and n:
            t = [self._log_times[int(g)] for g in rows[:, _native.LB_EPLOG_TAG]]
            self._monitor.write(rows, t)
        self._log_count.zero_()
        self._log_times = []

    def reset_masked(self, mask):
        """reset() of the envs where mask (B,) is nonzero; the others keep their episode."""
        m = mask.to(device=self.device, dtype=self.torch.uint8).contiguous()
        _native.check(self._L.lb_reset(self._ptr(self.state), C.byref(self._c), self.num_envs, self._ptr(m),
                                       self._ptr(self.obs), None, self._stream()))

    # ---- framework extras (device-resident) -----------------------------------------------------
    def step_device(self, actions, obs_out=None, terminal_obs_out=None, reward_out=None,
                    done_out=None, ep_stats_out=None):
        """Launch one fused step on device tensors; no host sync, no infos.

        actions: (B,) int32 device tensor, or None: every env takes its uniform random action
        drawn inside the step kernel (the value policy("random") would return; Philox mode).
        obs_out / reward_out / done_out default to the env's own buffers; pass slices of a
        rollout ring to write there directly.
        """
        if not self._reset_called:
            raise TypeError("step() called before reset()")
        _native.check(self._L.lb_step(
            self._ptr(self.state), C.byref(self._c), self.num_envs, self._ptr(actions),
            self._ptr(obs_out if obs_out is not None else self.obs),
            self._ptr(reward_out if reward_out is not None else self.rewards),
            self._ptr(done_out if done_out is not None else self.dones),
            self._ptr(terminal_obs_out if terminal_obs_out is not None else self.terminal_obs),
            self._ptr(ep_stats_out if ep_stats_out is not None else self.ep_stats),
            C.byref(self._trace) if self.trace_mode else None, self._stream()))

    def rollout(self, kind, steps, obs_out=None, reward_out=None, done_out=None, actions_out=None,
                terminal_obs_out=None, ep_stats_out=None):
        """`steps` vector steps under an on-device policy (_native.LB_POLICY: "topo" / "zone_cpu" /
        "endpoint_cpu" / "random", or "round_robin" / "least_loaded" / "least_latency" /
        "reward_greedy") in one launch (lb_rollout): the same trajectory as
        `steps` x (policy(kind), step_device(actions)).  Step k's outputs go to slot k of
        obs_out (K, B, R, 8), reward_out (K, B), done_out (K, B) uint8, actions_out (K, B)
        int32 (each None = not written)."""
        if not self._reset_called:
            raise TypeError("step() called before reset()")
        if self.trace_mode:
            raise RuntimeError("rollout() draws from Philox; trace mode steps one call at a time")
        _native.check(self._L.lb_rollout(
            self._ptr(self.state), C.byref(self._c), self.num_envs, _native.LB_POLICY[kind], int(steps),
            self._ptr(obs_out), self._ptr(reward_out), self._ptr(done_out), self._ptr(actions_out),
            self._ptr(terminal_obs_out if terminal_obs_out is not None else self.terminal_obs),
            self._ptr(ep_stats_out if ep_stats_out is not None else self.ep_stats), self._stream()))

    def rollout_kernel(self, steps, outputs_all=True, kind=None):
        """The kernel lb_rollout launches for `steps` vector steps with every output given
        (outputs_all) or not (lb_rollout_kernel; host only).  lb_rollout_kernel answers for the
        policies 0..3; with kind one of _native.POLICIES_WITHOUT_LEAN_KERNELS those answers become
        k_rollout_tpe (lb_rollout's rule)."""
        k = C.c_int32(-1)
        _native.check(self._L.lb_rollout_kernel(C.byref(self._c), self.num_envs, int(steps), int(bool(outputs_all)),
                                                C.byref(k)))
        name = _native.LB_ROLLOUT[k.value]
        lean = ("k_rollout_lean", "k_rollout_lean_split", "k_rollout_img")
        if kind in _native.POLICIES_WITHOUT_LEAN_KERNELS and name in lean:
            return "k_rollout_tpe"
        return name

    def policy(self, kind, out=None):
        """Batched on-device policy (_native.LB_POLICY) -> (B,) int32 device tensor: an
        envs/baselines.py greedy policy ("topo", "zone_cpu", "endpoint_cpu"), uniform "random",
        "round_robin" (current_step mod E), "least_loaded" (argmin avg_load_served),
        "least_latency" (argmin endpoint_latency + endpoint_topology_latency) or "reward_greedy"
        (argmax over every action of the reward step() would return; always 0 under the naive
        reward).  The last four look at all E endpoints; lowest index on ties."""
        out = out if out is not None else self.torch.empty(self.num_envs, dtype=self.torch.int32,
                                                           device=self.device)
        _native.check(self._L.lb_policy(self._ptr(self.state), C.byref(self._c), self.num_envs,
                                        _native.LB_POLICY[kind], self._ptr(out), self._stream()))
        return out

    def dqn_act(self, frag, obs, masks, ex, out):
        """lb_dqn_act: the DQN's explore decision for this vector step drawn on the device (ex:
        _native.LBDQNExploreC) and the actions into out -- every env's random action when
        exploring, else the greedy action of the Q network packed in frag."""
        R = obs.shape[1]
        _native.check(self._L.lb_dqn_act(frag.data_ptr(), obs.data_ptr(), self.num_envs, R, self._ptr(masks),
                                         self._ptr(self.state), C.byref(self._c), C.byref(ex), self._ptr(out),
                                         self._stream()))
        return out

    def dqn_step(self, frag, obs, masks, ex, actions, next_obs, reward, done, rb, pos_in, pos_out, ep_sum, ep_cnt):
        """lb_dqn_step: one DQN vector step -- dqn_act, step_device(actions, next_obs, reward, done)
        and the replay write (lb_replay_add into rb at the device slot *pos_in, obs <- next_obs,
        finished-episode sums) -- in one launch where the shape allows it (config 5's 4096 envs),
        else as those three launches; bit for bit the same either way."""
        self._dqn_guard()
        _native.check(self._L.lb_dqn_step(
            *self._dqn_args(frag, obs, masks, ex, actions, next_obs, reward, done, rb, pos_in, pos_out, ep_sum, ep_cnt),
            self._stream()))
        return actions

    def _dqn_args(self, frag, obs, masks, ex, actions, next_obs, reward, done, rb, pos_in, pos_out, ep_sum, ep_cnt):
        """lb_dqn_step's arguments up to ep_cnt, which lb_dqn_steps, lb_dqn_steps64 and lb_dqn_steps256 begin with too."""
        return (frag.data_ptr(), obs.data_ptr(), self.num_envs, obs.shape[1], self._ptr(masks), self._ptr(self.state),
                C.byref(self._c), C.byref(ex), self._ptr(actions), self._ptr(next_obs), self._ptr(reward),
                self._ptr(done), self._ptr(self.terminal_obs), self._ptr(self.ep_stats), rb.size, pos_in, pos_out,
                rb.obs.data_ptr(), rb.next_obs.data_ptr(), rb.actions.data_ptr(), rb.rewards.data_ptr(),
                rb.dones.data_ptr(), self._ptr(ep_sum), self._ptr(ep_cnt))

    def _dqn_guard(self):
        """step_device's checks for the DQN step entry points (they step the env too).  A launch
        captured into a HIP graph does not run: the learner captures its period graphs before
        its reset(), and the replays follow the reset."""
        if not self._reset_called and not self.torch.cuda.is_current_stream_capturing():
            raise TypeError("step() called before reset()")
        if self.trace_mode:
            raise RuntimeError("the DQN step draws its exploration and actions from Philox; trace mode steps "
                               "one call at a time (dqn_act + step)")

    def dqn_steps_supported(self, R):
        """Whether lb_dqn_steps (several DQN vector steps in one launch) covers this env with
        R-row observations."""
        return bool(self._L.lb_dqn_steps_supported(C.byref(self._c), self.num_envs, R))

    def dqn_steps(self, n, frag, obs, masks, ex, actions, next_obs, reward, done, rb, pos_in, pos_out, ep_sum, ep_cnt,
                  sync):
        """lb_dqn_steps: n DQN vector steps (dqn_step n times, the explore draw, replay slot and
        step counter advancing per step) in one launch; pos_in / pos_out and the explore
        struct's step words may coincide.  sync: a device int32 tensor holding 0."""
        self._dqn_guard()
        _native.check(self._L.lb_dqn_steps(
            *self._dqn_args(frag, obs, masks, ex, actions, next_obs, reward, done, rb, pos_in, pos_out, ep_sum, ep_cnt),
            int(n), sync.data_ptr(), self._stream()))
        return actions

    def dqn_steps64_supported(self, R):
        """Whether lb_dqn_steps64 (dqn_steps for envs of up to 64 endpoints: R <= 65 below 32,768
        envs, Philox mode) covers this env with R-row observations; true wherever
        dqn_steps_supported is."""
        return bool(self._L.lb_dqn_steps64_supported(C.byref(self._c), self.num_envs, R))

    def dqn_steps64(self, n, frag, obs, masks, ex, actions, next_obs, reward, done, rb, pos_in, pos_out, ep_sum,
                    ep_cnt, sync):
        """lb_dqn_steps64: dqn_steps, argument for argument, on the shapes of dqn_steps64_supported
        (config 4's E = 64, R = 65 among them), 1 <= n <= 32; on a shape dqn_steps covers, the same
        kernel.  masks (B, R) bool or uint8, or None (all valid); rb: the replay ring (size, obs,
        next_obs, actions, rewards, dones); pos_in / pos_out: device addresses of the slot words."""
        return self._dqn_steps_wide("dqn_steps64", self._L.lb_dqn_steps64, self.dqn_steps64_supported, n, frag, obs, masks,
                                    ex, actions, next_obs, reward, done, rb, pos_in, pos_out, ep_sum, ep_cnt, sync)

    def dqn_steps256_supported(self, R):
        """Whether lb_dqn_steps256 (dqn_steps for envs of up to 256 endpoints: R <= 257 below 32,768
        envs, Philox mode) covers this env with R-row observations; true wherever
        dqn_steps64_supported is."""
        return bool(self._L.lb_dqn_steps256_supported(C.byref(self._c), self.num_envs, R))

    def dqn_steps256(self, n, frag, obs, masks, ex, actions, next_obs, reward, done, rb, pos_in, pos_out, ep_sum,
                     ep_cnt, sync):
        """lb_dqn_steps256: dqn_steps, argument for argument, on the shapes of dqn_steps256_supported
        (the evaluation sweep's 80, 128, 150 and 180 endpoints among them), 1 <= n <= 32; on a shape
        dqn_steps64 covers, the same kernel.  The arguments are dqn_steps64's."""
        return self._dqn_steps_wide("dqn_steps256", self._L.lb_dqn_steps256, self.dqn_steps256_supported, n, frag, obs,
                                    masks, ex, actions, next_obs, reward, done, rb, pos_in, pos_out, ep_sum, ep_cnt, sync)

    def _dqn_steps_wide(self, who, entry, supported, n, frag, obs, masks, ex, actions, next_obs, reward, done, rb,
                        pos_in, pos_out, ep_sum, ep_cnt, sync):
        """dqn_steps64 / dqn_steps256 (who: the method's name, entry: its library function, supported:
        its query): the arguments checked, then the launch."""
        self._dqn_guard()
        t = self.torch
        B = self.num_envs
        n = int(n)
        if not 1 <= n <= 32:
            raise ValueError(f"{who}: n must be in [1, 32]")
        if not isinstance(obs, t.Tensor) or obs.dim() != 3:
            raise ValueError(f"{who}: obs must be a (B, R, 8) tensor")
        if (ep_sum is None) != (ep_cnt is None):
            raise ValueError(f"{who}: ep_sum and ep_cnt go together")
        if not isinstance(ex, _native.LBDQNExploreC):
            raise ValueError(f"{who}: ex must be a _native.LBDQNExploreC")
        R, S = obs.shape[1], int(rb.size)
        mdt = masks.dtype if isinstance(masks, t.Tensor) and masks.dtype == t.uint8 else t.bool
        self._check_tensors(who, [
            ("frag", frag, (_native.LB_DS_FRAG_FLOATS,), t.float32, False), ("obs", obs, (B, R, 8), t.float32, False),
            ("masks", masks, (B, R), mdt, True), ("actions", actions, (B,), t.int32, False),
            ("next_obs", next_obs, (B, R, 8), t.float32, False), ("reward", reward, (B,), t.float32, False),
            ("done", done, (B,), t.uint8, False), ("rb.obs", rb.obs, (S, B, R, 8), t.float32, False),
            ("rb.next_obs", rb.next_obs, (S, B, R, 8), t.float32, False),
            ("rb.actions", rb.actions, (S, B), t.int64, False), ("rb.rewards", rb.rewards, (S, B), t.float32, False),
            ("rb.dones", rb.dones, (S, B), t.float32, False), ("ep_sum", ep_sum, (B,), t.float64, True),
            ("ep_cnt", ep_cnt, (B,), t.float64, True), ("sync", sync, (1,), t.int32, False)])
        if not supported(R):
            raise RuntimeError(f"{who}: the env's shape has no one-launch vector step ({who}_supported)")
        _native.check(entry(
            *self._dqn_args(frag, obs, masks, ex, actions, next_obs, reward, done, rb, pos_in, pos_out, ep_sum, ep_cnt),
            n, self._ptr(sync), self._stream()))
        return actions

    def field(self, name):
        """Env attribute as a float64 device tensor: (B, E) or (B,)."""
        shape = (self.num_envs,) if name in _native.PER_ENV_FIELDS else (self.num_envs, self.cfg.num_endpoints)
        out = self.torch.empty(shape, dtype=self.torch.float64, device=self.device)
        _native.check(self._L.lb_get_field(self._ptr(self.state), C.byref(self._c), self.num_envs,
                                           _native.LB_FIELD[name], self._ptr(out), self._stream()))
        return out

    def stats(self):
        """Current per-env accumulators (B, 16) float64 (info.py ST_* layout)."""
        out = self.torch.empty((self.num_envs, _native.LB_ST_K), dtype=self.torch.float64,
                               device=self.device)
        _native.check(self._L.lb_get_stats(self._ptr(self.state), C.byref(self._c), self.num_envs,
                                           self._ptr(out), self._stream()))
        return out

    def status(self):
        _native.check(self._L.lb_status(self._ptr(self.state), C.byref(self._c), self.num_envs,
                                        self._ptr(self._flags), self._stream()))
        return int(self._flags.item())

    def accepted_fraction(self):
        st = self.stats()
        return (st[:, ST_ACC] / st[:, ST_LENGTH].clamp(min=1)).mean().item()

    def __repr__(self):
        return f"LBVecEnv(num_envs={self.num_envs}, {self.cfg})"
