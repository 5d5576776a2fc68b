"""lb_dqn_steps64 (csrc/lbk8s_dqn64.h): n DQN vector steps in ONE launch for envs of up to 64
endpoints == n x lb_dqn_step, bit for bit.  At these shapes lb_dqn_step is its three-launch
fallback (lb_dqn_act + lb_step + lb_replay_add: each case asserts that lb_dqn_steps does not cover
the shape), so the yardstick is the three existing launches.  The buffers and comparisons are those
of tests/test_gpu_dqn_step.py: the actions, next observations, rewards, dones, obs <- next obs, the
finished-episode sums, the terminal observations and episode-statistics rows, the whole replay
ring, the step / slot / explore words with sync left 0, env.stats() and four env fields.

Shapes: one per (W, TS) kernel and per path (R = 17 on 16 lanes, the first VALU image at R = 33,
config 4's R = 65, one env, more envs than resident waves).  Episode lengths 2 and 3 (envs end
several times per launch), an explore schedule that crosses from explore to greedy, n in
{1, 2, 7, 32} (even n keeps the device words in place, odd n ping-pongs them), a 16-slot ring that
wraps inside a launch, uint8 masks with about 30 % invalid entries in one case.
"""
import pytest
import torch

from test_gpu_dqn_step import _setup

pytestmark = pytest.mark.gpu

KEYS = ("act", "next_obs", "rew", "done", "obs", "ep_sum", "ep_cnt")
RING = ("obs", "next_obs", "actions", "rewards", "dones")
FIELDS = ("endpoint_latency", "endpoint_cpu_usage_percentage", "avg_load_served", "current_time")
CROSSING = (0.9, -(0.9 - 0.05) / 40.0, 0.05)  # eps from 0.9 down to 0.05 over 40 steps
ALL_EXPLORE, ALL_GREEDY = (2.0, 0.0, 2.0), (0.0, 0.0, 0.0)  # (the draw is a uniform in [0, 1))


class Side:
    """One env with test_gpu_dqn_step._setup's buffers and 16-slot ring."""

    def __init__(self, B, E, rej, L, seed=5):
        kw = dict(num_endpoints=E, rejection_allowed=rej, reward_function="multi", episode_length=L)
        self.env, self.frag, self.rb, self.st, self.nat = _setup(B, kw, seed)
        self.B, self.R = B, self.env.cfg.obs_rows
        self.sync = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.parity = 0
        self.keep = []  # (the explore structs of captured launches stay alive)

    def ex(self, sched, vin, vout):
        b = self.st["vpp"].data_ptr()
        e = self.nat.LBDQNExploreC(*sched, 77, b + 8 * vin, b + 8 * vout, self.st["flag"].data_ptr())
        self.keep.append(e)
        return e

    def steps64(self, n, masks, sched, entry="dqn_steps64"):
        """One launch of n steps through LBVecEnv.dqn_steps64 (or dqn_steps)."""
        st, p = self.st, self.rb.pos_pp.data_ptr()
        end = self.parity ^ (n & 1)
        getattr(self.env, entry)(n, self.frag, st["obs"], masks, self.ex(sched, self.parity, end), st["act"],
                                 st["next_obs"], st["rew"], st["done"], self.rb, p + 8 * self.parity, p + 8 * end,
                                 st["ep_sum"], st["ep_cnt"], self.sync)
        self.parity = end

    def singles(self, n, masks, sched):
        """n x lb_dqn_step with the ping-pong words; returns the steps' explore flags."""
        st, p = self.st, self.rb.pos_pp.data_ptr()
        flags = []
        for _ in range(n):
            q = self.parity
            self.env.dqn_step(self.frag, st["obs"], masks, self.ex(sched, q, 1 - q), st["act"], st["next_obs"],
                              st["rew"], st["done"], self.rb, p + 8 * q, p + 8 * (1 - q), st["ep_sum"], st["ep_cnt"])
            flags.append(st["flag"].clone())
            self.parity = 1 - q
        return [int(f.item()) for f in flags]

    def snapshot(self):
        ts = dict(self.st, state=self.env.state, ep_stats=self.env.ep_stats, term=self.env.terminal_obs,
                  pos_pp=self.rb.pos_pp, **{"rb_" + k: getattr(self.rb, k) for k in RING})
        return {k: (v, v.clone()) for k, v in ts.items()}, self.parity

    def restore(self, snap):
        for t, saved in snap[0].values():
            t.copy_(saved)
        self.parity = snap[1]


def _same_now(a, b, where):
    """What a launch leaves, against the single steps (the words in the current parity's slot)."""
    assert a.parity == b.parity
    assert int(a.sync.item()) == 0, where
    assert int(a.st["flag"].item()) == int(b.st["flag"].item()), where
    assert int(a.st["vpp"][a.parity].item()) == int(b.st["vpp"][b.parity].item()), where
    assert int(a.rb.pos_pp[a.parity].item()) == int(b.rb.pos_pp[b.parity].item()), where
    for k in KEYS:
        assert torch.equal(a.st[k], b.st[k]), (where, k)
    assert torch.equal(a.env.terminal_obs, b.env.terminal_obs), where
    assert torch.equal(a.env.ep_stats, b.env.ep_stats), where


def _same_end(a, b):
    for name in RING:
        assert torch.equal(getattr(a.rb, name), getattr(b.rb, name)), name
    assert torch.equal(a.env.stats(), b.env.stats())
    for f in FIELDS:
        assert torch.equal(a.env.field(f), b.env.field(f)), f
    assert torch.equal(a.env.state, b.env.state)


def _masks(B, R, seed=11):
    g = torch.Generator().manual_seed(seed)
    m = (torch.rand((B, R), generator=g) >= 0.3).to(torch.uint8)
    m[:, 0] = 1  # (every env keeps a valid action)
    return m.cuda()


def _pair(B, E, rej, L, seed=5):
    a, b = Side(B, E, rej, L, seed), Side(B, E, rej, L, seed)
    assert torch.equal(a.env.state, b.env.state) and torch.equal(a.st["obs"], b.st["obs"])
    assert a.env.dqn_steps64_supported(a.R) and not a.env.dqn_steps_supported(a.R)
    return a, b


# (B, E, rejection, n, episode length, masks); B "8c+3": 8 x the CU count + 3, more envs than waves
CASES = {
    "a_r17_w16": (67, 16, True, 7, 3, False),
    "b_w32": (5, 17, False, 32, 2, False),
    "c_r32": (67, 32, False, 2, 3, False),
    "d_r33_valu_masks": (33, 32, True, 7, 2, True),
    "e_w64": (9, 33, False, 1, 2, False),
    "f_r49_ts4": (19, 48, True, 32, 3, False),
    "g_r64": (17, 64, False, 2, 3, False),
    "h_r65_config4": (16, 64, True, 7, 3, False),
    "i_one_env": (1, 64, True, 32, 2, False),
    "j_more_envs_than_waves": ("8c+3", 64, True, 7, 3, False),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_dqn_steps64_equals_single_steps(name):
    B, E, rej, n, L, masked = CASES[name]
    if B == "8c+3":
        B = 8 * torch.cuda.get_device_properties(0).multi_processor_count + 3
    a, b = _pair(B, E, rej, L)
    masks = _masks(B, a.R) if masked else torch.ones((B, a.R), dtype=torch.uint8, device="cuda")
    flags = []
    for k in range(-(-42 // n)):  # 42 steps and more: the schedule's 40 and past them
        a.steps64(n, masks, CROSSING)
        flags += b.singles(n, masks, CROSSING)
        _same_now(a, b, k)
    _same_end(a, b)
    assert 0 < sum(flags) < len(flags)  # explore and greedy steps both ran
    if n > 1:
        assert any(0 < sum(flags[i:i + n]) < n for i in range(0, len(flags), n))  # ... inside one launch
    # every env ended several times: the ring's done column, and the sums
    assert int(a.st["ep_cnt"].min().item()) >= 42 // L - 1
    assert a.rb.dones.sum().item() > 0
    if masked:  # the greedy steps kept to the valid actions
        greedy = [i for i, f in enumerate(flags) if not f and i >= len(flags) - 16]  # (the ring holds 16 steps)
        assert greedy
        for i in greedy:
            act = a.rb.actions[i % 16]
            assert masks.gather(1, act[:, None]).all()


@pytest.mark.parametrize("sched,flag", ((ALL_EXPLORE, 1), (ALL_GREEDY, 0)))
@pytest.mark.parametrize("B,E,rej", ((16, 64, True), (33, 32, True), (67, 32, False)))
def test_all_explore_and_all_greedy_launches(B, E, rej, sched, flag):
    """An all-explore launch stages no weight image; an all-greedy one runs the forward in every
    step."""
    a, b = _pair(B, E, rej, 3)
    masks = _masks(B, a.R)
    if flag:  # (no step reads the image: one full of NaNs gives the same bits)
        a.frag = torch.full_like(a.frag, float("nan"))
    for k, n in enumerate((7, 2)):
        a.steps64(n, masks, sched)
        assert b.singles(n, masks, sched) == [flag] * n
        _same_now(a, b, k)
    _same_end(a, b)


def test_two_launches_equal_one():
    """4 + 5 steps == 9 steps: the env, the observations, the ring slot and the step word carry
    across launches (an even launch in place, then an odd one)."""
    a, b = _pair(16, 64, True, 3)
    c = Side(16, 64, True, 3)
    masks = _masks(16, a.R)
    a.steps64(9, masks, CROSSING)
    c.steps64(4, masks, CROSSING)
    c.steps64(5, masks, CROSSING)
    _same_now(c, a, "4 + 5")
    _same_end(c, a)
    b.singles(9, masks, CROSSING)
    _same_now(a, b, "9")
    _same_end(a, b)


def test_graph_replay_twice_from_a_restored_state():
    """The launch captured in a graph and replayed, twice from the same restored state == the eager
    launch, both times."""
    n = 7
    a, _ = _pair(16, 64, True, 3)
    c = Side(16, 64, True, 3)
    masks = _masks(16, a.R)
    for s in (a, c):  # past the first steps: a mixed launch at t = 14
        s.steps64(n, masks, CROSSING)
        s.steps64(n, masks, CROSSING)
    torch.cuda.synchronize()
    snap = c.snapshot()
    a.steps64(n, masks, CROSSING)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c.steps64(n, masks, CROSSING)
    end = c.parity
    for k in range(2):
        c.restore(snap)
        g.replay()
        torch.cuda.synchronize()
        c.parity = end
        _same_now(c, a, k)
        _same_end(c, a)


def test_16_lane_shape_equals_lb_dqn_steps():
    """On a shape lb_dqn_steps supports, lb_dqn_steps64 runs its kernel: the same bits."""
    a, b = Side(8, 6, True, 3), Side(8, 6, True, 3)
    assert a.env.dqn_steps_supported(a.R) and a.env.dqn_steps64_supported(a.R)
    masks = _masks(8, a.R)
    for k, n in enumerate((7, 10, 32)):
        a.steps64(n, masks, CROSSING)
        b.steps64(n, masks, CROSSING, entry="dqn_steps")
        _same_now(a, b, k)
    _same_end(a, b)


def test_vec_env_dqn_steps64_checks_its_arguments():
    B, E = 16, 64
    a, b = _pair(B, E, True, 3)
    R, st, p = a.R, a.st, a.rb.pos_pp.data_ptr()
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda")
    masks = _masks(B, R)
    good = dict(n=5, frag=a.frag, obs=st["obs"], masks=masks, ex=a.ex(CROSSING, 0, 1), actions=st["act"],
                next_obs=st["next_obs"], reward=st["rew"], done=st["done"], rb=a.rb, pos_in=p, pos_out=p + 8,
                ep_sum=st["ep_sum"], ep_cnt=st["ep_cnt"], sync=a.sync)

    class Ring:  # a ring with one tensor of another shape or dtype
        def __init__(self, **kw):
            self.size = a.rb.size
            for k in RING:
                setattr(self, k, kw.get(k, getattr(a.rb, k)))

    state = a.env.state.clone()
    for kw in (dict(n=0), dict(n=33), dict(obs=z(B, R, 4)), dict(obs=z(B * R, 8)), dict(frag=a.frag.cpu()),
               dict(masks=masks.float()), dict(masks=masks[:, :-1].contiguous()), dict(actions=z(B, dt=torch.int64)),
               dict(next_obs=z(B, R + 1, 8)), dict(reward=z(B, dt=torch.float64)), dict(done=z(B)),
               dict(ep_sum=None), dict(ep_cnt=z(B)), dict(sync=z(1)), dict(sync=z(2, dt=torch.int32)),
               dict(ex=None), dict(rb=Ring(actions=z(16, B, dt=torch.int32))), dict(rb=Ring(obs=z(16, B, R, 4))),
               dict(rb=Ring(dones=z(B, 16).t()))):
        with pytest.raises(ValueError, match="dqn_steps64:"):
            a.env.dqn_steps64(**dict(good, **kw))
    assert torch.equal(a.env.state, state) and int(st["vpp"].sum().item()) == 0  # a refused call launched nothing
    with pytest.raises(RuntimeError, match="lb_dqn_steps_supported"):
        a.env.dqn_steps(**good)  # (the 16-lane entry point keeps refusing the shape)
    assert a.env.dqn_steps64(**dict(good, masks=masks.bool())) is st["act"]  # bool masks: the same bytes
    a.parity = 1
    b.singles(5, masks, CROSSING)
    _same_now(a, b, "wrapper")
    _same_end(a, b)


def test_learner_multi_step_e64_follows_the_same_trajectory():
    """DQN_DeepSets(multi_step_e64=True) against off at E = 64 with 16 envs over a few train periods:
    the same replay ring, Q-network parameters, episode sums and device words."""
    from lbk8s import LBVecEnv
    from lbk8s.dqn import DQN_DeepSets
    runs = []
    for on in (True, False):
        env = LBVecEnv(16, seed=4, as_tensors=True, num_endpoints=64, rejection_allowed=True, reward_function="multi",
                       episode_length=7)
        algo = DQN_DeepSets(env, seed=2, learning_starts=10, buffer_size=16 * 24, batch_size=32, multi_step_e64=on)
        assert algo.multi_step_e64 is on and env.dqn_steps64_supported(65) and not env.dqn_steps_supported(65)
        calls = []
        real = env.dqn_steps64
        env.dqn_steps64 = lambda n, *a, **k: (calls.append(n), real(n, *a, **k))[1]
        algo.learn(45)
        torch.cuda.synchronize()
        assert (len(calls) > 0) is on and set(calls) <= {1, algo.train_frequency}
        runs.append((algo, env))
    (x, ex), (y, ey) = runs
    assert x.train_steps == y.train_steps > 0
    for name in RING:
        assert torch.equal(getattr(x.rb, name), getattr(y.rb, name)), name
    for (k, p), q in zip(x.q_network.named_parameters(), y.q_network.parameters()):
        assert torch.equal(p, q), k
    assert x.episode_returns == y.episode_returns and len(x.episode_returns) > 0
    for k in ("_ep_sum", "_ep_cnt", "_vstep_pp", "_explore_flag", "_obs", "_dqn_sync"):
        assert torch.equal(getattr(x, k), getattr(y, k)), k
    assert torch.equal(x.rb.pos_pp, y.rb.pos_pp) and int(x._dqn_sync.item()) == 0
    assert torch.equal(ex.state, ey.state) and torch.equal(ex.stats(), ey.stats())
