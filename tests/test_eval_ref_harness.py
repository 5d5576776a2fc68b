"""The greedy evaluation's reference harness (tests/eval_ref.py) checked on the CPU, with no GPU.

The device under test here is a stand-in: a second oracle as the env and torch's float32 forward
of the same network with first-index argmax, writing the buffers lb_eval_steps writes
(tests/test_gpu_eval_oracle.py runs the same harness on the HIP kernel).

(a) The float64 reference accepts a correct float32 implementation: every case stays inside the
    action tolerance and the disagreement cap (at most 1e-3 of a case's decisions).
(b) The checker catches what it claims to: each deliberately broken stand-in fails it.

Measured, the stand-in (decisions, disagreements with the float64 argmax, largest Q64 shortfall,
tol at the largest max|Q|); the cases of (a) are 40 steps in launches of 1, 6, 13 and 20:
    R9-B64-dqn-w3               2,560   0   0   5.5e-4 at 63.5
    R9-B64-dqn-w3-masks         2,560   0   0   5.5e-4 at 63.5
    R9-B64-ppo-w11              2,560   0   0   4.5e-4 at 50.9
    R16-B67-ppo-w3-masks        2,680   0   0   4.5e-4 at 50.8
    R7-B400-dqn-w11-no-reset    2,800   0   0   4.7e-4 at 53.6   (auto-reset off, one launch of L = 7)
    (b)'s R9-B1025-dqn-w3      41,000   0   0   6.0e-4 at 69.5   (with masks: 6.1e-4 at 71.9)
The worst share is 0 (cap 1e-3): torch's float32 forward took the float64 argmax at every decision.
"""
import numpy as np
import pytest
import torch

import eval_ref
from eval_ref import EvalChecker

PLAN = (1, 6, 13, 20)  # 40 steps: episodes of 7 steps end inside a launch, on its last step and across launches


def make_net(kind, wseed):
    from lbk8s.deepsets import DeepSetAgent, DQNDeepSetAgent
    torch.manual_seed(wseed)
    return DQNDeepSetAgent(8).q_network if kind == "dqn" else DeepSetAgent(8).actor


class StandIn:
    """A second oracle plus the float32 torch network; bug: one of the mutations of (b)."""

    def __init__(self, oracle_mod, net, kw, B, seed, masks=None, auto_reset=True, bug=None):
        self.net, self.bug, self.auto = net, bug, auto_reset
        self.orc = oracle_mod.OracleBatch(kw, B, trace=False, auto_reset=auto_reset, seed=seed)
        self.orc.init()
        R = self.orc.R
        self.B, self.R = B, R
        self.mask = np.ones((B, R), bool) if masks is None else np.asarray(masks).astype(bool)
        self.s = dict(obs=self.orc.reset(), act=np.zeros(B, np.int32), rew=np.zeros(B, np.float32),
                      done=np.zeros(B, np.uint8), ep_stats=np.zeros((B, 16), np.float64),
                      ep_sum=np.zeros(B, np.float64), ep_cnt=np.zeros(B, np.float64), ret32=np.zeros(B, np.float32),
                      ep_r32=np.zeros(B, np.float32), log=np.zeros((0, eval_ref.LOG_W)), count=0)
        self.prev_a = np.zeros(B, np.int32)
        self.prev_r = np.zeros(B, np.float32)
        self.rng = np.random.default_rng(1)

    def greedy(self, obs):
        with torch.no_grad():
            q = self.net(torch.from_numpy(obs)).numpy()
        qm = q if self.bug == "ignore_mask" else np.where(self.mask, q, np.float32(eval_ref.dqn_ref.HUGE_NEG))
        a = qm.argmax(1)
        if self.bug == "second_best":  # on 1 % of the decisions, where a second valid action exists
            hit = (self.rng.random(self.B) < 0.01) & (self.mask.sum(1) > 1)
            q2 = qm.copy()
            q2[np.arange(self.B), a] = -np.inf
            a = np.where(hit, q2.argmax(1), a)
        if self.bug == "last_duplicate":
            same = eval_ref.same_rows(obs, a) & self.mask
            last = self.R - 1 - same[:, ::-1].argmax(1)
            a = np.where(same.any(1), last, a)
        return a.astype(np.int32)

    def run(self, n, tag0):
        s, B = self.s, self.B
        acts, rews, dones = np.zeros((n, B), np.int32), np.zeros((n, B), np.float32), np.zeros((n, B), np.uint8)
        rows = [s["log"]]
        for i in range(n):
            a = self.greedy(s["obs"])
            o2, r2, d2, _, st2 = self.orc.step(a)
            r64 = self.orc.last_reward64()
            acts[i] = self.prev_a if self.bug == "action_late" else a
            rews[i] = self.prev_r if self.bug == "reward_late" else r2
            if self.bug != "dones_last_only" or i == n - 1:
                dones[i] = d2
            if self.auto:
                s["ep_stats"][d2] = st2[d2]
            s["ep_sum"][d2] += s["ep_stats"][d2, 0] * (2 if self.bug == "ep_sum_twice" else 1)
            s["ep_cnt"][d2] += 1.0
            r32 = (s["ret32"].astype(np.float64) + r64).astype(np.float32)
            for env in np.flatnonzero(d2)[::-1]:  # (rows are unordered within a call)
                row = np.zeros(eval_ref.LOG_W)
                row[:16] = s["ep_stats"][env]
                row[16:21] = r32[env], r2[env], a[env], env, tag0 + i
                rows.append(row[None])
            s["ep_r32"][d2] = r32[d2]
            s.update(obs=o2, act=a, rew=r2, done=d2.astype(np.uint8), ret32=np.where(d2, np.float32(0), r32))
            self.prev_a, self.prev_r = a, r2
        s.update(actions_all=acts, rewards_all=rews, dones_all=dones, log=np.concatenate(rows))
        s["count"] = len(s["log"])

    def read(self):
        return self.s

    def stats(self):
        return self.orc.stats()

    def field(self, name):
        return self.orc.field(dict(eval_ref.FIELDS)[name])

    def status(self):
        return 0


def run_case(oracle_mod, kw, B, kind, wseed, masks=False, auto_reset=True, plan=PLAN, bug=None):
    net = make_net(kind, wseed)
    R = kw.get("num_endpoints", 8) + (1 if kw.get("rejection_allowed", True) else 0)
    m = eval_ref.random_masks(B, R, seed=B) if masks else None
    ref = EvalChecker(oracle_mod, net, kw, B, 5, m, auto_reset)
    dev = StandIn(oracle_mod, net, kw, B, 5, m, auto_reset, bug)
    np.testing.assert_array_equal(dev.read()["obs"], ref.obs, err_msg="reset obs")
    for n in plan:
        ref.launch(dev, n)
    ref.finish(dev)
    print(f"{kw} B={B} {kind} w{wseed} masks={bool(masks)}: {ref.summary()}, share {ref.share():.2e}")
    return ref


R9 = dict(reward_function="multi", episode_length=7)
# (kw, B, network, weight seed, masks, auto-reset, plan): at least 2,000 decisions each
CASES = [
    (R9, 64, "dqn", 3, False, True, PLAN),
    (R9, 64, "dqn", 3, True, True, PLAN),
    (R9, 64, "ppo", 11, False, True, PLAN),
    (dict(num_endpoints=15, num_nodes=30, reward_function="multi", episode_length=7), 67, "ppo", 3, True, True, PLAN),
    # run_test's: auto-reset off, the episode in one launch
    (dict(num_endpoints=6, reward_function="multi", episode_length=7), 400, "dqn", 11, False, False, (7,)),
]


def case_id(c):
    kw, B, kind, wseed, masks, auto, plan = c
    R = kw.get("num_endpoints", 8) + (1 if kw.get("rejection_allowed", True) else 0)
    return f"R{R}-B{B}-{kind}-w{wseed}" + ("-masks" if masks else "") + ("" if auto else "-no-reset")


@pytest.mark.parametrize("kw,B,kind,wseed,masks,auto,plan", CASES, ids=[case_id(c) for c in CASES])
def test_reference_accepts_float32_forward(oracle_mod, kw, B, kind, wseed, masks, auto, plan):
    ref = run_case(oracle_mod, kw, B, kind, wseed, masks, auto, plan)
    assert ref.greedy_decisions >= 2000
    assert ref.max_shortfall <= ref.max_tol and ref.share() <= eval_ref.MAX_DISAGREE_SHARE


# mutation: (with masks, the checker's message)
BUGS = {
    "ignore_mask": (True, "masked action"),
    "last_duplicate": (False, "identical rows"),  # the last index, not the first, of duplicated rows
    "second_best": (False, "below the maximum|identical rows"),  # the second-best valid action on 1 % of decisions
    # step i - 1's action in row i of actions_all: the oracle follows another action than the device took
    "action_late": (False, "below the maximum|identical rows|rewards_all|dones_all"),
    "reward_late": (False, "rewards_all"),  # rewards_all one row late
    "ep_sum_twice": (False, "ep_sum"),  # a finished episode's return added twice
    "dones_last_only": (False, "dones_all"),  # dones_all written only on the launch's last step
}


@pytest.mark.parametrize("bug", list(BUGS))
def test_checker_catches_broken_stand_in(oracle_mod, bug):
    masks, match = BUGS[bug]
    # (B = 1025: duplicated observation rows are rare; the same case passes without the mutation)
    run_case(oracle_mod, R9, 1025, "dqn", 3, masks)
    with pytest.raises(AssertionError, match=match):
        run_case(oracle_mod, R9, 1025, "dqn", 3, masks, bug=bug)
