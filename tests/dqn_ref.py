"""The reference side of one DQN vector step (envs/dqn_deepset.py:122-174), for the tests that
pin lb_dqn_step / lb_dqn_steps (csrc/lbk8s_dqn.h) directly to the C oracle.

Everything here is the oracle, numpy and torch float64 on the CPU:
  * oracle.OracleBatch (Philox mode, auto_reset) is the env;
  * oracle.dqn_explore(seed, start, slope, end, t) is the explore decision of global step t;
  * OracleBatch.policy_random() gives an exploring step's actions;
  * a float64 copy of the DQNDeepSetAgent is the Q network, evaluated on the oracle's own
    observations;
  * a numpy ring (slots, B, ...) stands for the replay buffer: step i of a launch writes
    slot (pos + i) % slots;
  * ep_sum / ep_cnt are float64 per-env accumulators of ep_stats[:, 0] on done.

Follow the device, accept within tolerance.  The device under test supplies each step's
action; StepChecker validates it and then steps the oracle with it, so one float32 near-tie
does not send the two trajectories apart and everything else stays a bit-for-bit comparison.

  exploring step   the action equals policy_random() exactly, for every env.
  greedy step      with Q = q64(obs), Qm = where(mask, Q, -1e8), the action a is accepted when
                     - mask[a] is true (or no entry is valid and a == 0),
                     - Qm[a] >= Qm.max() - tol,
                     - no lower index that could be chosen holds a bit-identical observation
                       row (the first index wins, dqn_deepset.py:134-142).
                   tol = 2 (2e-5 + 4e-6 max|Q|), max|Q| over the step: the absolute floor
                   tests/test_gpu_fused.py grants this forward, doubled because a gap is the
                   difference of two values.  Not tuned on any kernel.
  disagreements    a decision with a != Qm.argmax() is counted; finish() allows at most
                   MAX_DISAGREE_SHARE of the case's greedy decisions.

The device under test is anything with
    run(n, single)   one launch of n vector steps (single: lb_dqn_step, n == 1)
    read()           dict of numpy arrays: obs, next_obs, act, rew, done, terminal_obs, ep_stats,
                     ep_sum, ep_cnt, rb_obs, rb_next_obs, rb_actions, rb_rewards, rb_dones and
                     the ints vstep, pos, flag, sync
    stats(), field(name), status()
(tests/test_gpu_dqn_oracle.py: the HIP kernels; tests/test_dqn_ref_harness.py: a CPU stand-in.)
"""
import collections
import copy

import numpy as np
import torch

HUGE_NEG = -1e8
MAX_DISAGREE_SHARE = 1e-3
FIELDS = (("endpoint_latency", "ep_lat"), ("endpoint_cpu_usage_percentage", "ep_cpu"),
          ("avg_load_served", "loads"), ("current_time", "t"))

Schedule = collections.namedtuple("Schedule", "seed start slope end")
# eps from 0.9 down to 0.05 over 40 steps: early steps mostly explore, later ones are greedy
DEFAULT_SCHEDULE = Schedule(77, 0.9, -(0.9 - 0.05) / 40.0, 0.05)
ALWAYS_EXPLORE = Schedule(77, 1.0, 0.0, 1.0)
NEVER_EXPLORE = Schedule(77, 0.0, 0.0, 0.0)

SLOTS = 40
# the launches of one case, (n, single): lb_dqn_step twice (mostly exploring steps), lb_dqn_steps
# with n = 1, 2, 7, 32, 32, then lb_dqn_step three times (mostly greedy steps): 79 steps, so the
# ring of 40 slots wraps inside a launch and across launches
MIXED = [(1, True)] * 2 + [(1, False), (2, False), (7, False), (32, False), (32, False)] + [(1, True)] * 3


def action_tol(q_abs_max):
    return 2.0 * (2e-5 + 4e-6 * q_abs_max)


def random_masks(B, R, seed=0):
    """(B, R) uint8, ~30 % invalid; env 0 all invalid, env 1 only its last row valid."""
    m = (np.random.default_rng(seed).random((B, R)) >= 0.3).astype(np.uint8)
    m[0] = 0
    if B > 1:
        m[1] = 0
        m[1, R - 1] = 1
    return m


def same_rows(obs, idx):
    """(B, R) bool: row r of env b is bit-identical to row idx[b]."""
    bits = np.ascontiguousarray(obs).view(np.uint32)
    pick = bits[np.arange(len(bits)), idx]
    return (bits == pick[:, None, :]).all(-1)


class StepChecker:
    def __init__(self, oracle_mod, q_network, kw, B, seed, slots, schedule=DEFAULT_SCHEDULE, masks=None):
        self.oracle = oracle_mod
        self.orc = oracle_mod.OracleBatch(kw, B, trace=False, auto_reset=True, seed=seed)
        self.orc.init()
        self.obs = self.orc.reset()
        self.q64 = copy.deepcopy(q_network).double().cpu()
        self.B, self.R, self.slots, self.schedule = B, self.orc.R, slots, schedule
        self.mask = np.ones((B, self.R), bool) if masks is None else np.asarray(masks).astype(bool)
        R = self.R
        self.rb_obs = np.zeros((slots, B, R, 8), np.float32)
        self.rb_next_obs = np.zeros((slots, B, R, 8), np.float32)
        self.rb_actions = np.zeros((slots, B), np.int64)
        self.rb_rewards = np.zeros((slots, B), np.float32)
        self.rb_dones = np.zeros((slots, B), np.float32)
        self.ep_sum = np.zeros(B, np.float64)
        self.ep_cnt = np.zeros(B, np.float64)
        self.term = np.zeros((B, R, 8), np.float32)
        self.rows = np.zeros((B, 16), np.float64)
        self.ended_ever = np.zeros(B, bool)
        self.t = self.pos = 0
        self.explored_steps = self.greedy_steps = 0
        self.greedy_decisions = self.disagreements = 0
        self.max_shortfall = self.max_q = self.max_tol = 0.0

    # ---- one step's action -------------------------------------------------------------------
    def explores(self, t):
        s = self.schedule
        return bool(self.oracle.dqn_explore(s.seed, s.start, s.slope, s.end, t))

    def q_values(self, obs):
        with torch.no_grad():
            return self.q64(torch.from_numpy(obs).double()).numpy()

    def check_action(self, a, explore, what):
        B, R = self.B, self.R
        assert a.shape == (B,) and ((a >= 0) & (a < R)).all(), f"{what}: action out of range"
        if explore:
            np.testing.assert_array_equal(a, self.orc.policy_random(), err_msg=f"{what}: exploring action")
            self.explored_steps += 1
            return
        Q = self.q_values(self.obs)
        Qm = np.where(self.mask, Q, HUGE_NEG)
        tol = action_tol(np.abs(Q).max())
        env = np.arange(B)
        some_valid = self.mask.any(1)
        ok = np.where(some_valid, self.mask[env, a], a == 0)
        assert ok.all(), f"{what}: masked action taken by envs {np.flatnonzero(~ok)[:8]}"
        short = Qm.max(1) - Qm[env, a]
        worst = int(short.argmax())
        assert short[worst] <= tol, (f"{what}: env {worst} took action {a[worst]} with Q64 {short[worst]:.3e} "
                                     f"below the maximum (tol {tol:.3e})")
        # a lower index with the same observation row (and as eligible) has the same Q value
        dup = (same_rows(self.obs, a) & (np.arange(R)[None] < a[:, None]) & self.mask).any(1) & some_valid
        assert not dup.any(), f"{what}: envs {np.flatnonzero(dup)[:8]} took a later one of identical rows"
        self.greedy_steps += 1
        self.greedy_decisions += B
        self.disagreements += int((a != Qm.argmax(1)).sum())
        self.max_shortfall = max(self.max_shortfall, float(short[worst]))
        self.max_q = max(self.max_q, float(np.abs(Q).max()))
        self.max_tol = max(self.max_tol, tol)

    # ---- one launch --------------------------------------------------------------------------
    def check_reset(self, dev):
        np.testing.assert_array_equal(dev.read()["obs"], self.obs, err_msg="reset obs")

    def launch(self, dev, n, single=False):
        """Run one launch of n vector steps on dev and check all it wrote."""
        assert n <= self.slots and (n == 1 or not single)
        dev.run(n, single)
        s = dev.read()
        eq = np.testing.assert_array_equal
        explore = r2 = d2 = a = None
        for i in range(n):
            what = f"step {self.t + i} (launch step {i} of {n})"
            slot = (self.pos + i) % self.slots
            explore = self.explores(self.t + i)
            a = np.asarray(s["act"] if n == 1 else s["rb_actions"][slot]).astype(np.int64)
            self.check_action(a, explore, what)
            prev = self.obs
            o2, r2, d2, t2, st2 = self.orc.step(a.astype(np.int32))
            self.rb_obs[slot], self.rb_next_obs[slot], self.rb_actions[slot] = prev, o2, a
            self.rb_rewards[slot], self.rb_dones[slot] = r2, d2
            for name, exp in (("rb_obs", prev), ("rb_next_obs", o2), ("rb_actions", a), ("rb_rewards", r2),
                              ("rb_dones", d2.astype(np.float32))):
                eq(s[name][slot], exp, err_msg=f"{what}: {name} slot {slot}")
            self.term[d2], self.rows[d2] = t2[d2], st2[d2]
            self.ended_ever |= d2
            self.ep_sum[d2] += st2[d2, 0]
            self.ep_cnt[d2] += 1.0
            self.obs = o2
        self.t += n
        self.pos = (self.pos + n) % self.slots
        what = f"after step {self.t - 1}"
        # the whole ring: the slots this launch wrote, and every other slot as it was
        for name in ("rb_obs", "rb_next_obs", "rb_actions", "rb_rewards", "rb_dones"):
            eq(s[name], getattr(self, name), err_msg=f"{what}: {name}")
        eq(s["act"], a, err_msg=f"{what}: actions_out")
        eq(s["obs"], self.obs, err_msg=f"{what}: obs <- next obs")
        eq(s["next_obs"], self.obs, err_msg=f"{what}: next_obs_out")
        eq(s["rew"], r2, err_msg=f"{what}: reward_out")
        eq(s["done"].astype(bool), d2, err_msg=f"{what}: done_out")
        e = self.ended_ever
        eq(s["terminal_obs"][e], self.term[e], err_msg=f"{what}: terminal_obs")
        eq(s["ep_stats"][e], self.rows[e], err_msg=f"{what}: ep_stats")
        eq(s["ep_sum"], self.ep_sum, err_msg=f"{what}: ep_sum")
        eq(s["ep_cnt"], self.ep_cnt, err_msg=f"{what}: ep_cnt")
        assert s["vstep"] == self.t, f"{what}: vstep {s['vstep']} != {self.t}"
        assert s["pos"] == self.pos, f"{what}: pos {s['pos']} != {self.pos}"
        assert s["flag"] == int(explore), f"{what}: explore flag {s['flag']} != {int(explore)}"
        assert s["sync"] == 0, f"{what}: sync {s['sync']}"

    # ---- the end of a case -------------------------------------------------------------------
    def finish(self, dev, mixed=True):
        eq = np.testing.assert_array_equal
        eq(dev.stats(), self.orc.stats(), err_msg="stats")
        for f, g in FIELDS:
            eq(dev.field(f), self.orc.field(g), err_msg=f)
        assert dev.status() == 0
        if mixed:
            assert self.explored_steps > 0 and self.greedy_steps > 0, (self.explored_steps, self.greedy_steps)
        assert self.ep_cnt.sum() > 0, "no episode ended inside the window"
        assert self.disagreements <= MAX_DISAGREE_SHARE * self.greedy_decisions, self.summary()

    def summary(self):
        return (f"{self.explored_steps} explored + {self.greedy_steps} greedy steps, {self.greedy_decisions} greedy "
                f"decisions, {self.disagreements} disagreements, largest Q64 shortfall {self.max_shortfall:.3e} "
                f"(tol {self.max_tol:.3e} at max|Q| {self.max_q:.1f}), {int(self.ep_cnt.sum())} episodes ended")
