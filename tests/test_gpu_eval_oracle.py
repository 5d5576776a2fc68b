"""k_eval_steps (csrc/lbk8s_eval.h: lb_eval_steps, a greedy evaluation's vector steps in one
launch) pinned DIRECTLY to the C oracle and a float64 network.

test_gpu_eval_steps.py shows the launch equal to steps x (lb_ds_q_argmax, lb_step,
lb_ppo_record), HIP against HIP.  Here the other side is tests/eval_ref.py: oracle.OracleBatch as
the env, the float64 copy of the actor / Q network on the oracle's observations, numpy for the
sums, VecMonitor's float32 return and the log.  The device supplies each step's actions in
actions_all; the reference validates them with tests/dqn_ref.py's rules and bounds (valid under
the mask, within action_tol of the float64 maximum, the first of identical rows; at most 1e-3 of
a case's decisions off the float64 argmax), then follows them, so rewards_all, dones_all, the
final observations, the per-env outputs, ep_stats, ep_sum / ep_cnt, ret32 / ep_r32, every log row,
stats() and the state fields are compared bit for bit (tests/test_eval_ref_harness.py shows on the
CPU that the checker accepts a correct float32 implementation and refuses seven broken ones).

Cases: at least 2,000 decisions each; 40 steps of 7-step episodes in launches of 1, 6, 13 and 20
(episodes end inside a launch, on its last step and across launches), masks on and off, odd B,
R = 2, 7, 9 and 16 (with and without the reject row), a DQN Q network and a PPO actor, and
run_test's own form: auto-reset off, the episode in one launch.

Measured on an MI355X (decisions, disagreements with the float64 argmax, largest Q64 shortfall, tol
at the largest max|Q|; tol = 2 (2e-5 + 4e-6 max|Q|), cap 1e-3 of a case's decisions):
    R9-B64-dqn                    2,560   0   0   5.5e-4 at 63.5
    R9-B64-dqn-masks              2,560   0   0   5.5e-4 at 63.5
    R9-B65-ppo                    2,600   0   0   4.5e-4 at 50.9
    R7-B131-ppo-masks             5,240   0   0   5.4e-4 at 62.2
    R2-B257-dqn                  10,280   0   0   4.0e-4 at 45.3
    R16-B67-ppo-masks             2,680   0   0   4.5e-4 at 50.8
    R16-norej-B66-dqn             2,640   0   0   4.4e-4 at 49.7
    R7-B400-dqn-no-reset          2,800   0   0   4.7e-4 at 53.6
    R9-B301-ppo-masks-no-reset    2,107   0   0   4.7e-4 at 54.1
  Every case: no decision off the float64 argmax, every other compared value equal bit for bit.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import eval_ref
from eval_ref import EvalChecker

pytestmark = pytest.mark.gpu

PLAN = (1, 6, 13, 20)
STEPS_MAX = max(PLAN)


class HipDevice:
    """lb_eval_steps through the C ABI on buffers of its own (zeros at the start)."""

    def __init__(self, kw, B, seed, kind, wseed, masks, auto_reset):
        from lbk8s import LBVecEnv, _native, evaluate
        from lbk8s.deepsets import DeepSetAgent, DQNDeepSetAgent
        self.native = _native
        env = self.env = LBVecEnv(B, seed=seed, as_tensors=True, auto_reset=auto_reset, **kw)
        env.reset()
        torch.manual_seed(wseed)  # default init, not quantised
        self.agent = (DQNDeepSetAgent if kind == "dqn" else DeepSetAgent)(8).to(env.device)
        self.net, self.frag = evaluate.eval_image(self.agent, env.device)
        dev, R = env.device, env.cfg.obs_rows
        self.B, self.R = B, R
        self.masks = None if masks is None else torch.from_numpy(masks).to(dev)
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)
        self.obs = env.obs.clone()
        self.actions_all, self.rewards_all = z(STEPS_MAX, B, dt=torch.int32), z(STEPS_MAX, B)
        self.dones_all = z(STEPS_MAX, B, dt=torch.uint8)
        self.act, self.rew, self.done = z(B, dt=torch.int32), z(B), z(B, dt=torch.uint8)
        self.ep_stats = z(B, 16, dt=torch.float64)
        self.ep_sum, self.ep_cnt = z(B, dt=torch.float64), z(B, dt=torch.float64)
        self.ret32, self.ep_r32 = z(B), z(B)
        self.cap = B * (sum(PLAN) // 7 + 2)
        self.log = z(self.cap, eval_ref.LOG_W, dt=torch.float64)
        self.count = z(1, dt=torch.int32)
        self.n = 0

    def run(self, n, tag0):
        env, p = self.env, lambda t: None if t is None else t.data_ptr()
        self.n = n
        self.native.check(self.native.lib().lb_eval_steps(
            p(self.frag), p(self.obs), p(env.state), C.byref(env._c), self.B, self.R, p(self.masks), n,
            p(self.actions_all), p(self.rewards_all), p(self.dones_all), p(self.act), p(self.rew), p(self.done),
            p(self.ep_stats), p(self.ep_sum), p(self.ep_cnt), p(self.ret32), p(self.ep_r32), tag0, p(self.log),
            self.cap, p(self.count), None))

    def read(self):
        torch.cuda.synchronize()

        def c(t):
            return t.cpu().numpy()
        n, count = self.n, int(self.count.item())
        assert count <= self.cap
        return dict(obs=c(self.obs), actions_all=c(self.actions_all[:n]), rewards_all=c(self.rewards_all[:n]),
                    dones_all=c(self.dones_all[:n]), act=c(self.act), rew=c(self.rew), done=c(self.done),
                    ep_stats=c(self.ep_stats), ep_sum=c(self.ep_sum), ep_cnt=c(self.ep_cnt), ret32=c(self.ret32),
                    ep_r32=c(self.ep_r32), log=c(self.log[:count]), count=count)

    def stats(self):
        return self.env.stats().cpu().numpy()

    def field(self, name):
        return self.env.field(name).cpu().numpy()

    def status(self):
        return self.env.status()


R9 = dict(reward_function="multi", episode_length=7)
R16 = dict(num_endpoints=15, num_nodes=30, reward_function="multi", episode_length=7)
R7 = dict(num_endpoints=6, reward_function="multi", episode_length=7)
# name: (kw, B, network, weight seed, masks, auto-reset, plan)
CASES = {
    "R9-B64-dqn": (R9, 64, "dqn", 3, False, True, PLAN),
    "R9-B64-dqn-masks": (R9, 64, "dqn", 3, True, True, PLAN),
    "R9-B65-ppo": (R9, 65, "ppo", 11, False, True, PLAN),  # odd B: the last group holds one env
    "R7-B131-ppo-masks": (R7, 131, "ppo", 3, True, True, PLAN),  # run.py's env
    "R2-B257-dqn": (dict(num_endpoints=1, episode_length=7), 257, "dqn", 11, False, True, PLAN),  # the smallest set
    "R16-B67-ppo-masks": (R16, 67, "ppo", 3, True, True, PLAN),  # the limit: all 16 lanes and columns live
    "R16-norej-B66-dqn": (dict(num_endpoints=16, rejection_allowed=False, episode_length=7), 66, "dqn", 3, False, True,
                          PLAN),
    "R7-B400-dqn-no-reset": (R7, 400, "dqn", 11, False, False, (7,)),  # run_test's: the episode in one launch
    "R9-B301-ppo-masks-no-reset": (R9, 301, "ppo", 3, True, False, (7,)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_eval_steps_equals_oracle(oracle_mod, name):
    kw, B, kind, wseed, masks, auto, plan = CASES[name]
    R = kw.get("num_endpoints", 8) + (1 if kw.get("rejection_allowed", True) else 0)
    m = eval_ref.random_masks(B, R, seed=B) if masks else None
    dev = HipDevice(kw, B, 5, kind, wseed, m, auto)
    assert dev.env.eval_steps_supported(R)
    ref = EvalChecker(oracle_mod, dev.net, kw, B, 5, m, auto)
    np.testing.assert_array_equal(dev.read()["obs"], ref.obs, err_msg="reset obs")
    for n in plan:
        ref.launch(dev, n)
    print(f"\n{name}: {ref.summary()}, share {ref.share():.2e}")
    assert ref.greedy_decisions >= 2000
    ref.finish(dev)
