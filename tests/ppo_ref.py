"""The reference side of a PPO rollout's vector steps (envs/ppo_deepset.py:160-190), for the tests
that pin lb_ppo_steps, lb_ppo_steps64 and lb_ppo_steps256 (csrc/lbk8s_ppo.h, lbk8s_steps64.h,
lbk8s_ppo256.h) directly to the C oracle and the float64 definition of the draw.

Everything here is the oracle, numpy and torch float64 on the CPU:
  * oracle.OracleBatch (Philox mode, auto-reset on) is the env, brought to the device's starting
    phase by the same calls (tests/test_gpu_ppo_steps._env): reset, one step under the oracle's
    random policy, a reset of the odd envs;
  * a float64 deep copy of the DeepSetAgent, evaluated on the oracle's own observations, is the
    network;
  * the bookkeeping is tests/ppo_tail_ref.ppo_record_ref, called once per step: per-env float64
    ep_sum / ep_cnt with sequential adds, VecMonitor's ret32 = float32(float64(ret32) + r64) with
    the oracle's last_reward64(), ep_r32, and the episode log as a dict of rows keyed by
    (tag, env).  ep_sum, ep_cnt and ret32 start from the values the device's buffers hold before
    the first launch (non-zero: tests/test_gpu_ppo_steps.Bufs' recipe, initial_values here).

Follow the device, accept within tolerance (as tests/eval_ref.py).  Step i's draw is checked by
tests/ds_sample_ref.check_sample, tolerances unchanged and no row exempt: the plain forward of the
row's input observation (dev.forward: another kernel) near the float64 network, the row's value
equal to the plain forward's bit for bit, the action inside its inverse-CDF interval under the
float64 softmax for the row's uniform, the log-probability within the checker's bound.  The oracle
is then stepped with the validated action, so one float32 near-tie does not send the trajectories
apart and everything else is compared bit for bit: rewards, dones_next / obs_next (or last_done /
last_obs, as store_rows says), actions_out, done_out, the lb_reward64 array, ep_stats and ep_r32 of
the envs that ended, ep_sum, ep_cnt, ret32, count and every log row (columns 0 .. LB_EPLOG_TAG).
A capped log holds exactly cap distinct rows of the model's set under the full count.  Every
buffer's guard elements, the rows of the per-step buffers outside the launch, last_obs / last_done
when every row is stored, and ret32 / ep_r32 / log / count without a log must be as they were.

The device under test is anything with
    reset_obs                    the observations after the first reset, (B, R, 8)
    run(n, store_rows, tag0)     one launch of n vector steps on the rows t .. t + n - 1 of its
                                 buffers (t: the steps run so far); the first launch reads the env's
                                 observations, a later one row t - 1 of obs_next
    read()                       dict of flat numpy arrays, guards included: every buffer of
                                 test_gpu_ppo_steps.Bufs.ALL (sizes()' layout), "reward64" (the
                                 lb_reward64 array, (B,)) and "obs" (the env's own observation buffer)
    forward(x) -> (logits, value)   the plain float32 forward of observations x (B, R, 8)
    stats(), field(name), status()
(tests/test_gpu_ppo_oracle.py: the HIP kernels; tests/test_ppo_ref_harness.py: a CPU stand-in.)
"""
import copy

import numpy as np
import torch

import ds_ref
import ds_sample_ref as sr
from dqn_ref import FIELDS
from ds_sample_ref import Case, Setup
from eval_ref import bits
from ppo_tail_ref import LB_EPLOG_ENV, LB_EPLOG_TAG, LB_EPLOG_W, LB_ST_K, ppo_record_ref
from test_gpu_ppo_steps import PAD, Bufs

TAG_BASE = 1000  # the first launch's tag0: a log row's tag is tag0 + i, not the step index
STEP_BUFS = ("actions_f32", "logprobs", "values", "rewards")
DTYPES = dict({k: np.float32 for k in Bufs.F32}, **{k: np.float64 for k in Bufs.F64}, actions_out=np.int32,
              done_out=np.uint8, count=np.int32)


def sizes(B, R, steps, S, cap):
    """The live elements of each buffer (test_gpu_ppo_steps.Bufs.n): PAD guard elements follow."""
    return dict(actions_f32=steps * B, logprobs=steps * B, values=steps * B, rewards=steps * B,
                obs_next=S * B * R * 8, dones_next=S * B, last_obs=B * R * 8, last_done=B, ret32=B, ep_r32=B,
                ep_stats=B * LB_ST_K, ep_sum=B, ep_cnt=B, log=max(cap, 1) * LB_EPLOG_W, actions_out=B, done_out=B,
                count=1)


def initial_values(B):
    """Bufs' non-zero starting ret32, ep_sum and ep_cnt."""
    return dict(ret32=torch.randn(B, generator=torch.Generator().manual_seed(B)).numpy(),
                ep_sum=np.arange(B, dtype=np.float64) * 0.25, ep_cnt=(np.arange(B) % 3).astype(np.float64))


def uniforms(steps, B, seed):
    """(steps, B) float32: a seeded torch.rand; env 0 draws 0 and env 1 draws 1 - 2^-24 at step 0."""
    u = torch.rand((steps, B), generator=torch.Generator().manual_seed(seed))
    u[0, 0] = 0.0
    if B >= 2:
        u[0, 1] = sr.U_ONE
    return u


def make_agent(wseed):
    """The case's DeepSetAgent (default init, on the CPU)."""
    from lbk8s.deepsets import DeepSetAgent
    torch.manual_seed(wseed)
    return DeepSetAgent(8)


def batch_size(B):
    """A case table's B: a number, or "8c+3" (more env groups than resident waves: 8 per CU and a rest)."""
    return 8 * ds_ref.device_cus() + 3 if B == "8c+3" else B


def launches(steps, store_all=False):
    """A plan's (n, store_rows) pairs: every launch but the last stores all its rows (its last
    observations are the next launch's input), the last one steps - 1 unless store_all."""
    return [(n, n) for n in steps[:-1]] + [(steps[-1], steps[-1] if store_all else steps[-1] - 1)]


def episodes_ended(B, L, steps, phase=True):
    """How many episodes end within `steps` steps: the even envs start one step into theirs."""
    start = (1 - np.arange(B) % 2) if (phase and L > 1) else np.zeros(B, np.int64)
    return int(((start + steps) // L).sum())


class PPOChecker:
    def __init__(self, oracle_mod, agent, kw, B, seed, plan, u, cap, with_log=True, phase=True):
        """plan: the launches, (n, store_rows) each; u: (sum n, B) uniforms; cap: the log's rows."""
        self.orc = oracle_mod.OracleBatch(kw, B, trace=False, auto_reset=True, seed=seed)
        self.orc.init()
        self.reset_obs = self.obs = self.orc.reset()
        self.L = int(kw["episode_length"])
        if phase and self.L > 1:  # test_gpu_ppo_steps._env
            o1 = self.orc.step(self.orc.policy_random())[0]
            odd = (np.arange(B) % 2).astype(np.uint8)
            o2 = self.orc.reset(mask=odd)
            self.obs = np.where(odd.astype(bool)[:, None, None], o2, o1)
        self.n64 = copy.deepcopy(agent).double().cpu()
        self.B, self.R = B, self.orc.R
        self.plan = [tuple(p) for p in plan]
        assert all(s == n for n, s in self.plan[:-1]), "a launch that is followed stores all its rows"
        self.T = sum(n for n, _ in self.plan)
        self.S = self.T - (self.plan[-1][0] - self.plan[-1][1])
        self.u = np.asarray(u, np.float32)
        assert self.u.shape == (self.T, B)
        self.cap, self.with_log = cap, with_log
        self.n = sizes(B, self.R, self.T, self.S, cap)
        self.t = 0
        self.log = {}
        self.ended = np.zeros(B, np.int64)
        self.twice_in_a_launch = self.longer_than_an_episode = False
        self.first_rows = self.last_rows = 0
        self.margins = {}
        self.image = self.prev = None

    # ---- before the first launch ---------------------------------------------------------------
    def start(self, dev):
        eq = np.testing.assert_array_equal
        eq(bits(np.asarray(dev.reset_obs)), bits(self.reset_obs), err_msg="reset obs")
        s = dev.read()
        eq(bits(s["obs"].reshape(self.obs.shape)), bits(self.obs), err_msg="obs after the masked reset")
        for k in Bufs.ALL:
            assert s[k].dtype == DTYPES[k] and s[k].shape == (self.n[k] + PAD,), (k, s[k].dtype, s[k].shape)
        self.image = {k: s[k].copy() for k in Bufs.ALL}
        self.prev = self.image
        B = self.B
        self.ret32, self.ep_r32 = s["ret32"][:B].copy(), s["ep_r32"][:B].copy()
        self.ep_sum, self.ep_cnt = s["ep_sum"][:B].copy(), s["ep_cnt"][:B].copy()
        self.rows = s["ep_stats"][:B * LB_ST_K].reshape(B, LB_ST_K).copy()
        assert np.isfinite(self.ret32).all() and np.isfinite(self.ep_sum).all() and np.isfinite(self.ep_cnt).all()
        assert (self.ret32 != 0).any() and (B < 3 or ((self.ep_sum != 0).any() and (self.ep_cnt != 0).any()))
        assert int(s["count"][0]) == 0

    # ---- one step's draw -----------------------------------------------------------------------
    def check_draw(self, dev, g, s, what):
        B, R = self.B, self.R
        row = slice(g * B, (g + 1) * B)
        a_f32 = s["actions_f32"][row]
        assert np.isfinite(a_f32).all(), f"{what}: actions_f32 not written"
        a = a_f32.astype(np.int32)
        logits, value = dev.forward(self.obs)
        logits, value = np.asarray(logits, np.float32), np.asarray(value, np.float32)
        assert logits.shape == (B, R) and value.shape == (B,)
        with torch.no_grad():
            x64 = torch.from_numpy(self.obs).double()
            ref = {"logits": self.n64.actor(x64).numpy(), "value": self.n64.critic(x64).numpy()}
        su = Setup(Case("sample", "ac", R, f"B{B}", (0, 1, 0), False), B, None, None, None, ref)
        got = sr.as_numpy(sr.alloc_outputs(B, R, "ac"))
        got["actions"][:B], got["actions_f32"][:B] = a, a_f32
        got["logprob"][:B], got["value"][:B] = s["logprobs"][row], s["values"][row]
        got["logits"][:B * R] = logits.reshape(-1)
        margins = sr.check_sample(su, None, self.u[g], got, fwd={"logits": logits, "value": value})
        assert all(v <= 1.0 for v in margins.values()), (what, margins)
        for k, v in margins.items():
            self.margins[k] = max(self.margins.get(k, 0.0), v)
        self.first_rows += int((a == 0).sum())
        self.last_rows += int((a == R - 1).sum())
        return a

    # ---- one launch ----------------------------------------------------------------------------
    def launch(self, dev, n, store_rows):
        """Run one launch of n vector steps on dev and check all it wrote."""
        assert self.image is not None, "start(dev) first"
        assert (n, store_rows) == self.plan[0] and store_rows in (n, n - 1)
        self.plan.pop(0)
        eq = np.testing.assert_array_equal
        B, R = self.B, self.R
        dev.run(n, store_rows, TAG_BASE + self.t)
        s = dev.read()
        for k in Bufs.ALL:
            assert s[k].dtype == DTYPES[k] and s[k].shape == (self.n[k] + PAD,), (k, s[k].dtype, s[k].shape)
        a = r2 = d2 = r64 = None
        in_launch = np.zeros(B, np.int64)
        for i in range(n):
            g, tag = self.t + i, TAG_BASE + self.t + i
            what = f"step {g} (launch step {i} of {n})"
            row = slice(g * B, (g + 1) * B)
            a = self.check_draw(dev, g, s, what)
            o2, r2, d2, _, st2 = self.orc.step(a)
            r64 = self.orc.last_reward64()
            eq(bits(s["rewards"][row]), bits(r2), err_msg=f"{what}: rewards")
            self.rows[d2] = st2[d2]
            log = None
            if self.with_log:
                log = dict(reward=r2, reward64=r64, actions=a, ret32=self.ret32, ep_r32=self.ep_r32, tag=tag, rows=[],
                           count=0)
            ndone = ppo_record_ref(d2.astype(np.uint8), self.rows, self.ep_sum, self.ep_cnt, log)
            if log is not None:
                for r in log["rows"]:
                    self.log[(tag, int(r[LB_EPLOG_ENV]))] = r[:LB_EPLOG_TAG + 1]
                assert log["count"] == int(d2.sum())
            if i < store_rows:
                eq(bits(s["dones_next"][row]), bits(ndone), err_msg=f"{what}: dones_next")
                eq(bits(s["obs_next"][g * B * R * 8:(g + 1) * B * R * 8].reshape(B, R, 8)), bits(o2),
                   err_msg=f"{what}: obs_next")
            else:
                eq(bits(s["last_done"][:B]), bits(ndone), err_msg=f"{what}: last_done")
                eq(bits(s["last_obs"][:B * R * 8].reshape(B, R, 8)), bits(o2), err_msg=f"{what}: last_obs")
            in_launch += d2
            self.obs = o2
        lo, hi = self.t, self.t + n
        self.t += n
        self.ended += in_launch
        self.longer_than_an_episode |= self.L < n
        self.twice_in_a_launch |= bool(in_launch.max() >= 2)
        what = f"after step {self.t - 1}"
        # the rows of other launches, and of none yet, are as they were
        for k, w, top in [(k, B, hi) for k in STEP_BUFS] + [("dones_next", B, min(lo + store_rows, self.S)),
                                                           ("obs_next", B * R * 8, min(lo + store_rows, self.S))]:
            eq(bits(s[k][:lo * w]), bits(self.prev[k][:lo * w]), err_msg=f"{what}: {k} before the launch's rows")
            eq(bits(s[k][top * w:]), bits(self.prev[k][top * w:]), err_msg=f"{what}: {k} past the launch's rows")
        if store_rows == n:  # last_* keep their NaN fill
            for k in ("last_obs", "last_done"):
                eq(bits(s[k]), bits(self.image[k]), err_msg=f"{what}: {k} with every row stored")
        eq(s["actions_out"][:B], a, err_msg=f"{what}: actions_out")
        eq(s["done_out"][:B].astype(bool), d2, err_msg=f"{what}: done_out")
        assert (s["done_out"][:B] <= 1).all(), f"{what}: done_out"
        eq(bits(np.asarray(s["reward64"], np.float64)), bits(r64), err_msg=f"{what}: the lb_reward64 array")
        e = self.ended > 0
        eq(bits(s["ep_stats"][:B * LB_ST_K].reshape(B, LB_ST_K)[e]), bits(self.rows[e]), err_msg=f"{what}: ep_stats")
        eq(bits(s["ep_sum"][:B]), bits(self.ep_sum), err_msg=f"{what}: ep_sum")
        eq(bits(s["ep_cnt"][:B]), bits(self.ep_cnt), err_msg=f"{what}: ep_cnt")
        if self.with_log:
            eq(bits(s["ret32"][:B]), bits(self.ret32), err_msg=f"{what}: ret32")
            eq(bits(s["ep_r32"][:B][e]), bits(self.ep_r32[e]), err_msg=f"{what}: ep_r32")
            self.check_log(s, what)
        else:
            for k in ("ret32", "ep_r32", "log", "count"):
                eq(bits(s[k]), bits(self.image[k]), err_msg=f"{what}: {k} without a log")
        for k in Bufs.ALL:
            eq(bits(s[k][self.n[k]:]), bits(self.image[k][self.n[k]:]), err_msg=f"{what}: {k}'s guard elements")
        self.prev = {k: s[k].copy() for k in Bufs.ALL}

    def check_log(self, s, what):
        eq = np.testing.assert_array_equal
        count, W = int(s["count"][0]), LB_EPLOG_W
        assert count == len(self.log), f"{what}: log count {count} != {len(self.log)}"
        stored = min(count, self.cap)
        body = s["log"][:self.n["log"]]
        eq(bits(body[stored * W:]), bits(self.image["log"][stored * W:self.n["log"]]),
           err_msg=f"{what}: log past its rows")
        got = {}
        for r in body[:stored * W].reshape(stored, W):
            assert np.isfinite(r[:LB_EPLOG_TAG + 1]).all(), f"{what}: a log row not written in full"
            got[(int(r[LB_EPLOG_TAG]), int(r[LB_EPLOG_ENV]))] = r
        assert len(got) == stored, f"{what}: {stored - len(got)} of {stored} stored log rows repeat a (tag, env) key"
        if count <= self.cap:
            assert set(got) == set(self.log), f"{what}: log rows' (tag, env) keys"
        for key, r in got.items():
            assert key in self.log, f"{what}: log row (tag, env) = {key} is none of the model's"
            eq(bits(r[:LB_EPLOG_TAG + 1]), bits(self.log[key]), err_msg=f"{what}: log row (tag, env) = {key}")

    # ---- the end of a case ---------------------------------------------------------------------
    def finish(self, dev, last_row=True):
        """last_row=False: the case's weights leave the last row less than the draw's tolerance
        (tests/test_gpu_ppo256_oracle.py's given seeds), so no action there is asked for."""
        eq = np.testing.assert_array_equal
        assert not self.plan and self.t == self.T, "launches of the plan left"
        eq(bits(dev.stats()), bits(self.orc.stats()), err_msg="stats")
        for f, g in FIELDS:
            eq(bits(dev.field(f)), bits(self.orc.field(g)), err_msg=f)
        assert dev.status() == 0
        # the coverage the case is there for: conditions, not measurements
        assert self.ended.min() >= 1, "an env never ended"
        if self.longer_than_an_episode:
            assert self.twice_in_a_launch, "no env ended twice inside one launch"
        assert self.last_rows >= 1 or not last_row, "no action was the last row"
        assert self.first_rows >= 1, "no action was row 0"
        if self.with_log:
            assert len(self.log) > 0, "no log row"
        assert self.margins and max(self.margins.values()) <= 1.0, self.margins

    def summary(self):
        m = "  ".join(f"{k} {v:.2f}" for k, v in sorted(self.margins.items()))
        return f"{self.T * self.B} draws, {int(self.ended.sum())} episodes ended; worst margins: {m}"


def run_plan(ref, dev, plan, last_row=True):
    """start, every launch of the plan, finish."""
    ref.start(dev)
    for n, store_rows in plan:
        ref.launch(dev, n, store_rows)
    ref.finish(dev, last_row)
    return ref
