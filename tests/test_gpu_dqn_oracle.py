"""k_dqn_step (csrc/lbk8s_dqn.h: lb_dqn_step / lb_dqn_steps, config 5's whole vector step in one
launch) pinned DIRECTLY to the C oracle and a float64 Q network.

test_gpu_dqn_step.py shows the one-launch step equal to lb_dqn_act + lb_step + lb_replay_add,
HIP against HIP, at R = 9 or 7, even B and all-ones masks.  Here the other side is
tests/dqn_ref.py: oracle.OracleBatch as the env, oracle.dqn_explore as the explore decision,
policy_random() as an exploring step's actions, the float64 copy of the Q network on the
oracle's observations for the greedy ones, a numpy ring for the replay buffer.  The device
supplies each step's action; the reference validates it (exactly on an exploring step; valid,
within tol of the float64 maximum and the first of identical rows on a greedy one), then
follows it, so every replay row, output buffer, terminal obs, episode-statistics row,
finished-episode sum and device word of every launch is compared bit for bit
(tests/test_dqn_ref_harness.py shows on the CPU that the checker accepts a correct float32
implementation and refuses six broken ones).

Shapes: the smallest that reach each path of the kernel -- odd B (the last group of P = 2 holds
one env), fewer envs than one block's waves, one env, R = 2 / 3 / 7 / 9 / 16 (the fusable limit,
with and without the reject row), masks with ~30 % invalid entries, an all-invalid env and a
last-row-only env, launches of n = 1 (lb_dqn_step, sync NULL) and lb_dqn_steps n = 1, 2, 7, 32
(twice), an all-explore launch (no weight staging) and all-greedy launches, a ring of 40 slots
that wraps inside and across launches; R = 17 takes lb_dqn_step's three-launch fallback
through the same harness.

Measured (tol = 2 (2e-5 + 4e-6 max|Q|), cap 1e-3 of a case's greedy decisions):
  CPU, the reference alone, torch's float32 forward standing in for the kernel, before the
  tests were written (48 steps following the float64 argmax, E in {1, 2, 3, 6, 8, 12, 15},
  B 257 .. 8192, with and without masks): 0-5 disagreements per case (a share <= 2.1e-5),
  largest Q64 shortfall 1.4e-5 against tol 5e-4 .. 7e-4 at max|Q| 54 .. 82, |q32 - q64| <= 6e-5.
  CPU, the same forward as the device of this harness (tests/test_dqn_ref_harness.py, these
  cases at B <= 1025): 0-2 disagreements per case (a share <= 3.3e-5), largest Q64 shortfall
  6.1e-6 against tol 3.3e-4 .. 6.7e-4 at max|Q| 37 .. 78.
  MI355X, the HIP kernels (this file; explored + greedy steps, greedy decisions, disagreements,
  largest Q64 shortfall, tol at the largest max|Q|):
    R9-B4097            19 + 60   245,820   1   5.5e-6    6.7e-4 at 78.5
    R9-B4097-masks      19 + 60   245,820   1   6.5e-6    4.9e-4 at 56.5
    R7-B8               19 + 60       480   0   0         3.5e-4 at 38.3
    R9-B1               19 + 60        60   0   0         4.2e-4 at 47.2
    R2-B257             19 + 60    15,420   0   0         3.9e-4 at 44.2
    R3-B1025            19 + 60    61,500   0   0         7.1e-4 at 83.6
    R16-B1025           19 + 60    61,500   1   1.07e-5   4.7e-4 at 53.9
    R16-B1025-masks     19 + 60    61,500   1   1.9e-6    6.2e-4 at 72.6
    R16-norej-B514      19 + 60    30,840   1   4.2e-6    6.1e-4 at 71.7
    R9-B4097-explore    53 +  0         0   -   -         -
    R9-B4097-greedy      0 + 49   200,753   1   4.8e-7    4.8e-4 at 55.1
    R17-B257-fallback   17 + 31     7,967   0   0         4.2e-4 at 47.1
  Every case: a disagreeing share <= 3.3e-5 (cap 1e-3) and a shortfall at least 40 times under
  tol; every other compared value equal bit for bit.  No kernel was changed.
"""
import numpy as np
import pytest
import torch

import dqn_ref
from dqn_ref import ALWAYS_EXPLORE, DEFAULT_SCHEDULE, MIXED, NEVER_EXPLORE, SLOTS, StepChecker

pytestmark = pytest.mark.gpu


class HipDevice:
    """LBVecEnv.dqn_step / dqn_steps with their buffers, set up as test_gpu_dqn_step.py::_setup."""

    def __init__(self, kw, B, seed, wseed, slots, schedule, masks):
        from lbk8s import LBVecEnv, _native, fused
        from lbk8s.deepsets import DQNDeepSetAgent
        from lbk8s.dqn import DeviceReplayBuffer
        self.native, self.schedule = _native, schedule
        env = self.env = LBVecEnv(B, seed=seed, as_tensors=True, **kw)
        env.reset()
        torch.manual_seed(wseed)  # default init, not quantised
        self.q = DQNDeepSetAgent(8).to(env.device)
        self.frag = fused.frag_buffer(env.device)
        fused.pack_q_into(self.q, self.frag)
        R = self.R = env.cfg.obs_rows
        self.rb = DeviceReplayBuffer(slots * B, B, (R, 8), env.device, None)
        assert self.rb.size == slots
        dev = env.device
        self.masks = None if masks is None else torch.from_numpy(masks).to(dev)
        self.obs = env.obs.clone()
        self.next_obs = torch.zeros_like(env.obs)
        self.act = torch.zeros(B, dtype=torch.int32, device=dev)
        self.rew = torch.zeros(B, device=dev)
        self.done = torch.zeros(B, dtype=torch.uint8, device=dev)
        self.ep_sum = torch.zeros(B, dtype=torch.float64, device=dev)
        self.ep_cnt = torch.zeros(B, dtype=torch.float64, device=dev)
        self.vpp = torch.zeros(2, dtype=torch.int64, device=dev)
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.sync = torch.zeros(1, dtype=torch.int32, device=dev)
        self.parity = 0

    def supported(self):
        return self.env.dqn_steps_supported(self.R)

    def run(self, n, single):
        # the step and slot words ping-pong: a launch reads word `parity` and writes word `end`
        # (lb_dqn_steps over an even n: the same word)
        p, end = self.parity, self.parity ^ (n & 1)
        s, v, pp = self.schedule, self.vpp.data_ptr(), self.rb.pos_pp.data_ptr()
        ex = self.native.LBDQNExploreC(s.start, s.slope, s.end, s.seed, v + 8 * p, v + 8 * end, self.flag.data_ptr())
        args = (self.frag, self.obs, self.masks, ex, self.act, self.next_obs, self.rew, self.done, self.rb,
                pp + 8 * p, pp + 8 * end, self.ep_sum, self.ep_cnt)
        if single:
            self.env.dqn_step(*args)
        else:
            self.env.dqn_steps(n, *args, self.sync)
        self.parity = end

    def words(self):
        return (self.vpp.cpu().numpy().copy(), self.rb.pos_pp.cpu().numpy().copy(), int(self.flag.item()),
                int(self.sync.item()))

    def read(self):
        torch.cuda.synchronize()

        def c(t):
            return t.cpu().numpy()
        rb, env, p = self.rb, self.env, self.parity
        return dict(obs=c(self.obs), next_obs=c(self.next_obs), act=c(self.act), rew=c(self.rew), done=c(self.done),
                    terminal_obs=c(env.terminal_obs), ep_stats=c(env.ep_stats), ep_sum=c(self.ep_sum),
                    ep_cnt=c(self.ep_cnt), rb_obs=c(rb.obs), rb_next_obs=c(rb.next_obs), rb_actions=c(rb.actions),
                    rb_rewards=c(rb.rewards), rb_dones=c(rb.dones), vstep=int(self.vpp[p].item()),
                    pos=int(rb.pos_pp[p].item()), flag=int(self.flag.item()), sync=int(self.sync.item()))

    def stats(self):
        return self.env.stats().cpu().numpy()

    def field(self, name):
        return self.env.field(name).cpu().numpy()

    def status(self):
        return self.env.status()


def run_case(oracle_mod, name, kw, B, wseed, masks=False, schedule=DEFAULT_SCHEDULE, plan=MIXED, mixed=True,
             fusable=True):
    R = kw.get("num_endpoints", 8) + (1 if kw.get("rejection_allowed", True) else 0)
    m = dqn_ref.random_masks(B, R, seed=B) if masks else None
    dev = HipDevice(kw, B, 5, wseed, SLOTS, schedule, m)
    # the path under test is the one-launch kernel (else lb_dqn_step runs its three launches)
    assert dev.supported() == fusable
    ref = StepChecker(oracle_mod, dev.q, kw, B, 5, SLOTS, schedule, m)
    ref.check_reset(dev)
    assert sum(n for n, _ in plan) >= 48
    for n, single in plan:
        ref.launch(dev, n, single)
    print(f"\n{name}: {ref.summary()}")
    ref.finish(dev, mixed)
    assert ref.max_shortfall <= ref.max_tol
    return ref


R9 = dict(reward_function="multi", episode_length=9)
R16 = dict(num_endpoints=15, num_nodes=30, reward_function="multi", episode_length=9)
# name: (kw, B, weight seed, masks)
CASES = {
    "R9-B4097": (R9, 4097, 3, False),  # odd B: the last group holds one env
    "R9-B4097-masks": (R9, 4097, 11, True),
    "R7-B8": (dict(num_endpoints=6, reward_function="multi", episode_length=7), 8, 11, False),  # run.py's setup
    "R9-B1": (dict(episode_length=7), 1, 3, False),
    "R2-B257": (dict(num_endpoints=1, episode_length=7), 257, 11, False),  # the smallest set
    "R3-B1025": (dict(num_endpoints=2, reward_function="latency", episode_length=9), 1025, 3, False),
    "R16-B1025": (R16, 1025, 11, False),  # the fusable limit: all 16 lanes and columns live
    "R16-B1025-masks": (R16, 1025, 3, True),
    "R16-norej-B514": (dict(num_endpoints=16, rejection_allowed=False, episode_length=7), 514, 3, False),
}


@pytest.mark.parametrize("name", list(CASES))
def test_dqn_step_equals_oracle(oracle_mod, name):
    kw, B, wseed, masks = CASES[name]
    run_case(oracle_mod, name, kw, B, wseed, masks)


def test_dqn_step_all_explore(oracle_mod):
    """eps == 1: every launch is all explore (exm == all: the weight image is not staged), at
    n = 7 and at n = 32 (all = ~0u)."""
    ref = run_case(oracle_mod, "R9-B4097-explore", R9, 4097, 3, schedule=ALWAYS_EXPLORE,
                   plan=[(7, False)] * 3 + [(32, False)], mixed=False)
    assert ref.greedy_steps == 0


def test_dqn_step_all_greedy(oracle_mod):
    ref = run_case(oracle_mod, "R9-B4097-greedy", R9, 4097, 11, schedule=NEVER_EXPLORE, plan=[(7, False)] * 7,
                   mixed=False)
    assert ref.explored_steps == 0


def test_dqn_step_fallback_equals_oracle(oracle_mod):
    """R = 17: no one-launch step; lb_dqn_step runs lb_dqn_act + lb_step + lb_replay_add."""
    run_case(oracle_mod, "R17-B257-fallback", dict(num_endpoints=16, episode_length=7), 257, 11,
             plan=[(1, True)] * 48, fusable=False)


def test_dqn_steps_33_is_refused():
    """n = 33 (over lb_dqn_steps' longest launch) returns the error and launches nothing: the
    device words, the observations and the replay ring stay as they were."""
    dev = HipDevice(dict(num_endpoints=6, reward_function="multi", episode_length=7), 8, 5, 3, SLOTS,
                    DEFAULT_SCHEDULE, None)
    assert dev.supported()
    dev.run(2, False)
    before, words = dev.read(), dev.words()
    parity = dev.parity
    with pytest.raises(RuntimeError, match="steps must be in"):
        dev.run(33, False)
    dev.parity = parity
    after, words2 = dev.read(), dev.words()
    for a, b in zip(words, words2):
        np.testing.assert_array_equal(a, b)
    for k in before:
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)
