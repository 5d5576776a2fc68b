"""lb_dqn_steps256 (csrc/lbk8s_dqn256.h): n DQN vector steps in ONE launch for envs of up to 256
endpoints == n x lb_dqn_step, bit for bit.  At these shapes lb_dqn_step is its three-launch
fallback (lb_dqn_act + lb_step + lb_replay_add: each case asserts that lb_dqn_steps64 does not
cover the shape), so the yardstick is the three existing launches.  The buffers and comparisons are
tests/test_gpu_dqn_steps64.py's, by import: the actions, next observations, rewards, dones,
obs <- next obs, the finished-episode sums, the terminal observations and episode-statistics rows,
the whole replay ring, the step / slot / explore words with sync left 0, env.stats() and four env
fields.

Shapes: the first and last row count of each k_dqn_steps256<EPL, CHUNK> instance (R = 66 and 80
without chunks, 81 and 129 on two endpoints per lane, 129 and 257 on four), full 32-row chunks and
one row past them (R = 96, 97), one env, more envs than resident waves (a wave's second env reuses
its one LDS observation buffer).  Episode lengths 2 and 3 (envs end several times per launch), an
explore schedule that crosses from explore to greedy, n in {1, 2, 7, 32} (even n keeps the device
words in place, odd n ping-pongs them), a 16-slot ring that wraps inside a launch, uint8 masks with
about 30 % invalid entries in five cases.
"""
import pytest
import torch

from test_gpu_dqn_steps64 import ALL_EXPLORE, ALL_GREEDY, CROSSING, RING, Side, _masks, _same_end, _same_now

pytestmark = pytest.mark.gpu

E256 = "dqn_steps256"


def _pair(B, E, rej, L, seed=5):
    a, b = Side(B, E, rej, L, seed), Side(B, E, rej, L, seed)
    assert torch.equal(a.env.state, b.env.state) and torch.equal(a.st["obs"], b.st["obs"])
    assert a.env.dqn_steps256_supported(a.R) and not a.env.dqn_steps64_supported(a.R)
    return a, b


# (B, E, rejection, n, episode length, masks); B "8c+3": 8 x the CU count + 3, more envs than waves
CASES = {
    "a_r66_first_epl2": (9, 65, True, 7, 3, False),
    "b_r80_last_valu": (17, 80, False, 2, 3, True),
    "c_r81_first_chunked": (19, 80, True, 32, 2, False),
    "d_r96_full_chunks": (5, 96, False, 1, 2, False),
    "e_r97_masks": (7, 96, True, 7, 3, True),
    "f_r128_lanes_full": (16, 128, False, 2, 3, False),
    "g_r129_epl2_masks": (16, 128, True, 7, 3, True),
    "h_r129_epl4": (9, 129, False, 7, 2, False),
    "i_r181_masks": (16, 180, True, 32, 3, True),
    "j_r256": (5, 256, False, 7, 3, False),
    "k_r257_masks": (16, 256, True, 7, 3, True),
    "l_one_env": (1, 256, True, 32, 2, False),
    "m_more_envs_than_waves_r66": ("8c+3", 65, True, 7, 3, False),
    "n_more_envs_than_waves_r257": ("8c+3", 256, True, 2, 3, False),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_dqn_steps256_equals_single_steps(name):
    B, E, rej, n, L, masked = CASES[name]
    if B == "8c+3":
        B = 8 * torch.cuda.get_device_properties(0).multi_processor_count + 3
    a, b = _pair(B, E, rej, L)
    masks = _masks(B, a.R) if masked else torch.ones((B, a.R), dtype=torch.uint8, device="cuda")
    flags = []
    for k in range(-(-42 // n)):  # 42 steps and more: the schedule's 40 and past them
        a.steps64(n, masks, CROSSING, entry=E256)
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
@pytest.mark.parametrize("B,E,rej", ((16, 72, True), (16, 100, True), (16, 180, True)))  # one shape per instance
def test_all_explore_and_all_greedy_launches(B, E, rej, sched, flag):
    """An all-explore launch stages no weight image; an all-greedy one runs the forward in every
    step."""
    a, b = _pair(B, E, rej, 3)
    masks = _masks(B, a.R)
    if flag:  # (no step reads the image: one full of NaNs gives the same bits)
        a.frag = torch.full_like(a.frag, float("nan"))
    for k, n in enumerate((7, 2)):
        a.steps64(n, masks, sched, entry=E256)
        assert b.singles(n, masks, sched) == [flag] * n
        _same_now(a, b, k)
    _same_end(a, b)


def test_two_launches_equal_one():
    """4 + 5 steps == 9 steps: the env, the observations, the ring slot and the step word carry
    across launches (an even launch in place, then an odd one)."""
    a, b = _pair(16, 180, True, 3)
    c = Side(16, 180, True, 3)
    masks = _masks(16, a.R)
    a.steps64(9, masks, CROSSING, entry=E256)
    c.steps64(4, masks, CROSSING, entry=E256)
    c.steps64(5, masks, CROSSING, entry=E256)
    _same_now(c, a, "4 + 5")
    _same_end(c, a)
    b.singles(9, masks, CROSSING)
    _same_now(a, b, "9")
    _same_end(a, b)


def test_graph_replay_twice_from_a_restored_state():
    """The launch captured in a graph and replayed, twice from the same restored state == the eager
    launch, both times."""
    n = 7
    a, _ = _pair(16, 128, True, 3)
    c = Side(16, 128, True, 3)
    masks = _masks(16, a.R)
    for s in (a, c):  # past the first steps: a mixed launch at t = 14
        s.steps64(n, masks, CROSSING, entry=E256)
        s.steps64(n, masks, CROSSING, entry=E256)
    torch.cuda.synchronize()
    snap = c.snapshot()
    a.steps64(n, masks, CROSSING, entry=E256)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c.steps64(n, masks, CROSSING, entry=E256)
    end = c.parity
    for k in range(2):
        c.restore(snap)
        g.replay()
        torch.cuda.synchronize()
        c.parity = end
        _same_now(c, a, k)
        _same_end(c, a)


@pytest.mark.parametrize("B,E,entry", ((16, 64, "dqn_steps64"), (8, 6, "dqn_steps")))
def test_narrower_shape_equals_its_own_entry_point(B, E, entry):
    """On a shape lb_dqn_steps64 (or lb_dqn_steps) supports, lb_dqn_steps256 runs its kernel: the
    same bits."""
    a, b = Side(B, E, True, 3), Side(B, E, True, 3)
    assert a.env.dqn_steps256_supported(a.R) and a.env.dqn_steps64_supported(a.R)
    assert a.env.dqn_steps_supported(a.R) is (entry == "dqn_steps")
    masks = _masks(B, a.R)
    for k, n in enumerate((7, 10, 32)):
        a.steps64(n, masks, CROSSING, entry=E256)
        b.steps64(n, masks, CROSSING, entry=entry)
        _same_now(a, b, k)
    _same_end(a, b)


def test_vec_env_dqn_steps256_checks_its_arguments():
    B, E = 16, 128
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
        with pytest.raises(ValueError, match="dqn_steps256:"):
            a.env.dqn_steps256(**dict(good, **kw))
    assert torch.equal(a.env.state, state) and int(st["vpp"].sum().item()) == 0  # a refused call launched nothing
    with pytest.raises(RuntimeError, match="dqn_steps64_supported"):
        a.env.dqn_steps64(**good)  # (the narrower entry point keeps refusing the shape)
    assert int(st["vpp"].sum().item()) == 0
    assert a.env.dqn_steps256(**dict(good, masks=masks.bool())) is st["act"]  # bool masks: the same bytes
    a.parity = 1
    b.singles(5, masks, CROSSING)
    _same_now(a, b, "wrapper")
    _same_end(a, b)


def test_learner_multi_step_e256_follows_the_same_trajectory():
    """DQN_DeepSets(multi_step_e256=True) against off at E = 128 with 16 envs over a few train
    periods: the same replay ring, Q-network parameters, episode returns, device words and env."""
    from lbk8s import LBVecEnv
    from lbk8s.dqn import DQN_DeepSets
    runs = []
    for on in (True, False):
        env = LBVecEnv(16, seed=4, as_tensors=True, num_endpoints=128, rejection_allowed=True, reward_function="multi",
                       episode_length=7)
        algo = DQN_DeepSets(env, seed=2, learning_starts=10, buffer_size=16 * 24, batch_size=32, multi_step_e256=on)
        assert algo.multi_step_e256 is on and algo.multi_step_e64 is False
        assert env.dqn_steps256_supported(129) and not env.dqn_steps64_supported(129)
        calls = []
        real = env.dqn_steps256
        env.dqn_steps256 = lambda n, *a, **k: (calls.append(n), real(n, *a, **k))[1]
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
