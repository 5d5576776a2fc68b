"""The reference side of a greedy evaluation's vector steps (run_test_deepset.py:83-98), for the
tests that pin lb_eval_steps (csrc/lbk8s_eval.h) directly to the C oracle.

Everything here is the oracle, numpy and torch float64 on the CPU:
  * oracle.OracleBatch (Philox mode, auto-reset on or off) is the env;
  * a float64 copy of the actor (a DeepSetAgent's) or the Q network (a DQNDeepSetAgent's), the same
    module, evaluated on the oracle's own observations, is the network;
  * ep_sum / ep_cnt are float64 per-env accumulators of the finished episodes' ep_stats[:, 0];
  * ret32 is VecMonitor's float32 running return (one rounding per step of the float64 sum with the
    oracle's float64 reward), and the episode log is a dict of rows keyed by (tag, env).

Follow the device, accept within tolerance (as tests/dqn_ref.py, whose rules and bounds these are:
action_tol, same_rows, random_masks and MAX_DISAGREE_SHARE are imported, and a decision is checked
by StepChecker.check_action itself, never exploring).  The device under test supplies each step's
actions in actions_all; the checker validates them -- valid under the mask (action 0 where no row
is valid), the float64 masked value within action_tol of the maximum, no lower index with an
identical row -- and then steps the oracle with them, so one float32 near-tie does not send the
two trajectories apart and everything else stays a bit-for-bit comparison: rewards_all, dones_all,
the final observations, actions_out / reward_out / done_out, ep_stats, ep_sum / ep_cnt, ret32 /
ep_r32, the log rows, stats() and the state fields.  finish() allows at most MAX_DISAGREE_SHARE of
a case's decisions to differ from the float64 argmax: a condition, not a measurement.

With auto-reset off lb_step writes no ep_stats row (the buffer keeps what it held: zeros here), so
ep_sum adds that and the log rows carry it, as lb_ppo_record does after such a step.

The device under test is anything with
    run(n, tag0)     one launch of n vector steps, the log rows tagged tag0 .. tag0 + n - 1
    read()           dict of numpy arrays: obs, actions_all / rewards_all / dones_all (n, B) of the
                     last launch, act, rew, done, ep_stats, ep_sum, ep_cnt, ret32, ep_r32,
                     log (the stored rows so far, (k, 24)) and the int count
    stats(), field(name), status()
(tests/test_gpu_eval_oracle.py: the HIP kernel; tests/test_eval_ref_harness.py: a CPU stand-in.)
"""
import copy

import numpy as np

import dqn_ref  # noqa: F401
from dqn_ref import FIELDS, MAX_DISAGREE_SHARE, StepChecker, action_tol, random_masks, same_rows  # noqa: F401

LOG_W = 24
LOG_RET32, LOG_REWARD, LOG_ACTION, LOG_ENV, LOG_TAG = 16, 17, 18, 19, 20


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


class EvalChecker(StepChecker):
    """dqn_ref.StepChecker's decision rules (check_action, never exploring) over lb_eval_steps'
    outputs."""

    def __init__(self, oracle_mod, network, kw, B, seed, masks=None, auto_reset=True):
        self.oracle = oracle_mod
        self.orc = oracle_mod.OracleBatch(kw, B, trace=False, auto_reset=auto_reset, seed=seed)
        self.orc.init()
        self.obs = self.orc.reset()
        self.q64 = copy.deepcopy(network).double().cpu()
        self.B, self.R, self.auto = B, self.orc.R, auto_reset
        self.mask = np.ones((B, self.R), bool) if masks is None else np.asarray(masks).astype(bool)
        self.ep_sum = np.zeros(B, np.float64)
        self.ep_cnt = np.zeros(B, np.float64)
        self.ret32 = np.zeros(B, np.float32)
        self.ep_r32 = np.zeros(B, np.float32)
        self.rows = np.zeros((B, 16), np.float64)
        self.ended_ever = np.zeros(B, bool)
        self.log = {}
        self.t = 0
        self.explored_steps = self.greedy_steps = 0
        self.greedy_decisions = self.disagreements = 0
        self.max_shortfall = self.max_q = self.max_tol = 0.0

    def launch(self, dev, n):
        """Run one launch of n vector steps on dev and check all it wrote."""
        dev.run(n, self.t)
        s = dev.read()
        eq = np.testing.assert_array_equal
        B = self.B
        for k, dt in (("actions_all", np.int32), ("rewards_all", np.float32), ("dones_all", np.uint8)):
            assert s[k].shape == (n, B) and s[k].dtype == dt, k
        a = r2 = d2 = None
        for i in range(n):
            tag = self.t + i
            what = f"step {tag} (launch step {i} of {n})"
            a = np.asarray(s["actions_all"][i]).astype(np.int64)
            self.check_action(a, False, what)
            o2, r2, d2, _, st2 = self.orc.step(a.astype(np.int32))
            r64 = self.orc.last_reward64()
            eq(bits(s["rewards_all"][i]), bits(r2), err_msg=f"{what}: rewards_all")
            eq(s["dones_all"][i], d2.astype(np.uint8), err_msg=f"{what}: dones_all")
            if self.auto:
                self.rows[d2] = st2[d2]
            self.ended_ever |= d2
            self.ep_sum[d2] += self.rows[d2, 0]
            self.ep_cnt[d2] += 1.0
            r32 = (self.ret32.astype(np.float64) + r64).astype(np.float32)
            for env in np.flatnonzero(d2):
                self.log[(tag, int(env))] = np.concatenate(
                    [self.rows[env], [float(r32[env]), float(r2[env]), float(a[env]), float(env), float(tag)]])
            self.ep_r32[d2] = r32[d2]
            self.ret32 = np.where(d2, np.float32(0), r32)
            self.obs = o2
        self.t += n
        what = f"after step {self.t - 1}"
        eq(s["act"], a, err_msg=f"{what}: actions_out")
        eq(bits(s["obs"]), bits(self.obs), err_msg=f"{what}: obs <- the observations after the last step")
        eq(bits(s["rew"]), bits(r2), err_msg=f"{what}: reward_out")
        eq(s["done"].astype(bool), d2, err_msg=f"{what}: done_out")
        e = self.ended_ever
        eq(bits(s["ep_stats"][e]), bits(self.rows[e]), err_msg=f"{what}: ep_stats")
        eq(bits(s["ep_sum"]), bits(self.ep_sum), err_msg=f"{what}: ep_sum")
        eq(s["ep_cnt"], self.ep_cnt, err_msg=f"{what}: ep_cnt")
        eq(bits(s["ret32"]), bits(self.ret32), err_msg=f"{what}: ret32")
        eq(bits(s["ep_r32"][e]), bits(self.ep_r32[e]), err_msg=f"{what}: ep_r32")
        assert s["count"] == len(self.log), f"{what}: log count {s['count']} != {len(self.log)}"
        got = {(int(r[LOG_TAG]), int(r[LOG_ENV])): r for r in s["log"]}
        assert len(got) == len(s["log"]) and set(got) == set(self.log), f"{what}: log rows' (tag, env) keys"
        for key, row in self.log.items():
            eq(bits(got[key][:LOG_TAG + 1]), bits(row), err_msg=f"{what}: log row (tag, env) = {key}")

    def finish(self, dev):
        eq = np.testing.assert_array_equal
        eq(bits(dev.stats()), bits(self.orc.stats()), err_msg="stats")
        for f, g in FIELDS:
            eq(bits(dev.field(f)), bits(self.orc.field(g)), err_msg=f)
        assert dev.status() == 0
        assert self.explored_steps == 0 and self.greedy_decisions == self.t * self.B
        assert self.ep_cnt.sum() > 0, "no episode ended inside the window"
        assert self.disagreements <= MAX_DISAGREE_SHARE * self.greedy_decisions, self.summary()
        assert self.max_shortfall <= self.max_tol

    def share(self):
        return self.disagreements / max(1, self.greedy_decisions)
