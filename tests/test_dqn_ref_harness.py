"""The DQN vector step's reference harness (tests/dqn_ref.py) checked on the CPU, with no GPU.

The device under test here is a stand-in: a second oracle as the env and torch's float32
forward of the same DQNDeepSetAgent as the Q network, writing the buffers lb_dqn_step /
lb_dqn_steps write (tests/test_gpu_dqn_oracle.py runs the same harness on the HIP kernels).

(a) The float64 reference accepts a correct float32 implementation: every case stays inside
    the action tolerance and the disagreement cap.
(b) The checker catches what it claims to: each deliberately broken stand-in fails it.
"""
import numpy as np
import pytest
import torch

import dqn_ref
from dqn_ref import ALWAYS_EXPLORE, DEFAULT_SCHEDULE, MIXED, NEVER_EXPLORE, SLOTS, StepChecker


def make_q(wseed):
    from lbk8s.deepsets import DQNDeepSetAgent
    torch.manual_seed(wseed)
    return DQNDeepSetAgent(8)


class StandIn:
    """A second oracle plus the float32 torch network; bug: one of the mutations of (b)."""

    def __init__(self, oracle_mod, q_network, kw, B, seed, slots, schedule=DEFAULT_SCHEDULE, masks=None, bug=None):
        self.oracle, self.q, self.schedule, self.bug = oracle_mod, q_network, schedule, bug
        self.orc = oracle_mod.OracleBatch(kw, B, trace=False, auto_reset=True, seed=seed)
        self.orc.init()
        R = self.orc.R
        self.B, self.R, self.slots = B, R, slots
        self.mask = np.ones((B, R), bool) if masks is None else np.asarray(masks).astype(bool)
        self.s = dict(
            obs=self.orc.reset(), next_obs=np.zeros((B, R, 8), np.float32), act=np.zeros(B, np.int32),
            rew=np.zeros(B, np.float32), done=np.zeros(B, np.uint8), terminal_obs=np.zeros((B, R, 8), np.float32),
            ep_stats=np.zeros((B, 16), np.float64), ep_sum=np.zeros(B, np.float64), ep_cnt=np.zeros(B, np.float64),
            rb_obs=np.zeros((slots, B, R, 8), np.float32), rb_next_obs=np.zeros((slots, B, R, 8), np.float32),
            rb_actions=np.zeros((slots, B), np.int64), rb_rewards=np.zeros((slots, B), np.float32),
            rb_dones=np.zeros((slots, B), np.float32), vstep=0, pos=0, flag=0, sync=0)
        self.rng = np.random.default_rng(1)

    def greedy(self, obs):
        with torch.no_grad():
            q = self.q(torch.from_numpy(obs)).numpy()
        qm = q if self.bug == "ignore_mask" else np.where(self.mask, q, np.float32(dqn_ref.HUGE_NEG))
        a = qm.argmax(1)
        if self.bug == "second_best":  # on 1 % of the decisions, where a second valid action exists
            hit = (self.rng.random(self.B) < 0.01) & (self.mask.sum(1) > 1)
            q2 = qm.copy()
            q2[np.arange(self.B), a] = -np.inf
            a = np.where(hit, q2.argmax(1), a)
        if self.bug == "last_duplicate":
            same = dqn_ref.same_rows(obs, a) & self.mask
            last = self.R - 1 - same[:, ::-1].argmax(1)
            a = np.where(same.any(1), last, a)
        return a.astype(np.int32)

    def run(self, n, single):
        s, sc = self.s, self.schedule
        for i in range(n):
            t = s["vstep"] + (1 if self.bug == "explore_next" else 0)
            explore = self.oracle.dqn_explore(sc.seed, sc.start, sc.slope, sc.end, t)
            a = self.orc.policy_random() if explore else self.greedy(s["obs"])
            o2, r2, d2, t2, st2 = self.orc.step(a)
            slot = (s["pos"] + (1 if self.bug == "slot_late" else 0)) % self.slots
            s["rb_obs"][slot], s["rb_next_obs"][slot], s["rb_actions"][slot] = s["obs"], o2, a
            s["rb_rewards"][slot], s["rb_dones"][slot] = r2, d2
            s["terminal_obs"][d2], s["ep_stats"][d2] = t2[d2], st2[d2]
            s["ep_sum"][d2] += st2[d2, 0] * (2 if self.bug == "ep_sum_twice" else 1)
            s["ep_cnt"][d2] += 1.0
            s.update(obs=o2, next_obs=o2, act=a, rew=r2, done=d2.astype(np.uint8), flag=int(explore),
                     vstep=s["vstep"] + 1, pos=(s["pos"] + 1) % self.slots)

    def read(self):
        return self.s

    def stats(self):
        return self.orc.stats()

    def field(self, name):
        return self.orc.field(dict(dqn_ref.FIELDS)[name])

    def status(self):
        return 0


def run_case(oracle_mod, kw, B, wseed, masks=None, schedule=DEFAULT_SCHEDULE, plan=MIXED, bug=None, mixed=True):
    q = make_q(wseed)
    R = kw.get("num_endpoints", 8) + (1 if kw.get("rejection_allowed", True) else 0)
    m = dqn_ref.random_masks(B, R, seed=B) if masks else None
    ref = StepChecker(oracle_mod, q, kw, B, 5, SLOTS, schedule, m)
    dev = StandIn(oracle_mod, q, kw, B, 5, SLOTS, schedule, m, bug)
    ref.check_reset(dev)
    for n, single in plan:
        ref.launch(dev, n, single)
    ref.finish(dev, mixed)
    print(f"{kw} B={B} masks={bool(masks)}: {ref.summary()}")
    return ref


# the GPU test's cases (tests/test_gpu_dqn_oracle.py), at B <= 1025
CASES = [
    (dict(reward_function="multi", episode_length=9), 1025, 3, False),
    (dict(reward_function="multi", episode_length=9), 1025, 11, True),
    (dict(num_endpoints=6, reward_function="multi", episode_length=7), 8, 3, False),
    (dict(episode_length=7), 1, 11, False),
    (dict(num_endpoints=1, episode_length=7), 257, 3, False),
    (dict(num_endpoints=2, reward_function="latency", episode_length=9), 1025, 11, False),
    (dict(num_endpoints=15, num_nodes=30, reward_function="multi", episode_length=9), 1025, 3, False),
    (dict(num_endpoints=15, num_nodes=30, reward_function="multi", episode_length=9), 1025, 11, True),
    (dict(num_endpoints=16, rejection_allowed=False, episode_length=7), 514, 3, False),
    (dict(num_endpoints=16, episode_length=7), 257, 11, False),
]


def case_id(c):
    kw, B, wseed, masks = c
    R = kw.get("num_endpoints", 8) + (1 if kw.get("rejection_allowed", True) else 0)
    return f"R{R}-B{B}-w{wseed}" + ("-masks" if masks else "")


@pytest.mark.parametrize("kw,B,wseed,masks", CASES, ids=[case_id(c) for c in CASES])
def test_reference_accepts_float32_forward(oracle_mod, kw, B, wseed, masks):
    ref = run_case(oracle_mod, kw, B, wseed, masks)
    assert ref.max_shortfall <= ref.max_tol


def test_reference_schedules(oracle_mod):
    kw = dict(reward_function="multi", episode_length=9)
    ref = run_case(oracle_mod, kw, 257, 3, schedule=ALWAYS_EXPLORE, plan=[(7, False)] * 7, mixed=False)
    assert ref.greedy_steps == 0 and ref.explored_steps == 49
    ref = run_case(oracle_mod, kw, 257, 3, schedule=NEVER_EXPLORE, plan=[(7, False)] * 7, mixed=False)
    assert ref.explored_steps == 0 and ref.greedy_steps == 49


BUG_KW = dict(reward_function="multi", episode_length=9)


# mutation: (with masks, the checker's message)
BUGS = {
    "second_best": (False, "below the maximum|identical rows"),  # the second-best valid action on 1 % of decisions
    "last_duplicate": (False, "identical rows"),  # the last index, not the first, of duplicated rows
    "ignore_mask": (True, "masked action"),
    "slot_late": (False, "rb_obs"),  # the replay row one slot late
    "ep_sum_twice": (False, "ep_sum"),  # a finished episode's return added twice
    "explore_next": (False, "exploring action|masked|below the maximum|explore flag"),  # step t + 1's explore draw
}


@pytest.mark.parametrize("bug", list(BUGS))
def test_checker_catches_broken_stand_in(oracle_mod, bug):
    masks, match = BUGS[bug]
    run_case(oracle_mod, BUG_KW, 1025, 3, masks)  # (the same case passes without the mutation)
    with pytest.raises(AssertionError, match=match):
        run_case(oracle_mod, BUG_KW, 1025, 3, masks, bug=bug)
