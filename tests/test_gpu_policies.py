"""The on-device policies LB_POLICY_ROUND_ROBIN .. LB_POLICY_REWARD_GREEDY (include/lbk8s.h) on the
GPU: lb_policy against numpy on the env's fields (kinds 4..6) and against the reward lb_step itself
returns (reward greedy: the C oracle by brute force, and lb_step on a cloned state where the
replayed oracle is too slow), lb_rollout against K x (lb_policy + lb_step), and run_baselines.
Every comparison is exact (tests/policies_ref.py).
"""
import numpy as np
import pytest
import torch

import policies_ref as pr

pytestmark = pytest.mark.gpu

K8S = ("round_robin", "least_loaded", "least_latency", "reward_greedy")


def _env(B, kw, geometry, L, seed=21, **more):
    from lbk8s import LBVecEnv
    env = LBVecEnv(B, seed=seed, as_tensors=True, episode_length=L, geometry=geometry, **kw, **more)
    env.reset()
    return env


def _policy(env, kind):
    out = torch.full((env.num_envs,), -1, dtype=torch.int32, device="cuda")  # every env is written
    got = env.policy(kind, out=out)
    assert got is out
    return out.cpu().numpy()


# (B, env, layout): E = 1; run_baselines' env; one lane per env; no rejection; W = 32; W = 64;
# W = 64 with two endpoints per lane; E = 256; four envs per wave; one lane per env, many envs
FIELD_SHAPES = [
    (257, dict(num_endpoints=1), "auto"),
    (257, dict(num_endpoints=6, num_nodes=48, num_zones=12), "auto"),
    (300, {}, "tpe"),
    (257, dict(num_endpoints=16, rejection_allowed=False), "auto"),
    (130, dict(num_endpoints=17), "auto"),
    (67, dict(num_endpoints=64), "auto"),
    (33, dict(num_endpoints=65), "auto"),
    (9, dict(num_endpoints=256), "auto"),
    (32771, dict(num_endpoints=20), "auto"),
    (40000, dict(num_endpoints=6), "tpe"),
]


@pytest.mark.parametrize("B,kw,geometry", FIELD_SHAPES)
def test_field_policies_equal_numpy(B, kw, geometry):
    """round_robin / least_loaded / least_latency == numpy on env.field(...), after 0, 1, 3 and
    L - 1 random steps and again after the auto-reset (L = 5)."""
    L = 5
    env = _env(B, kw, geometry, L)
    E = env.cfg.num_endpoints
    for s in range(L + 3):
        if s in (0, 1, 3, L - 1, L, L + 2):
            f = lambda name: env.field(name).cpu().numpy()
            if s == L:
                assert (f("current_step") == 0).all() and (f("avg_load_served") == 0).all()  # auto-reset
            for kind, ref in pr.K8S_REFS.items():
                got = _policy(env, kind)
                np.testing.assert_array_equal(got, ref(f, E), err_msg=f"{kind} after {s} steps")
                assert got.min() >= 0 and got.max() < E  # never the reject action
        env.step_device(None)
    assert env.status() == 0


@pytest.mark.parametrize("name", list(pr.GREEDY_CASES))
def test_reward_greedy_equals_oracle_brute_force(oracle_mod, name):
    """lb_policy(reward_greedy) is the first argmax over a of the float64 reward a fresh oracle
    returns for step(a) after replaying the history: 16 decisions per env with L = 7, the GPU env
    stepped along the same trajectory."""
    B, kw, geometry = pr.GREEDY_CASES[name]
    env = _env(B, kw, geometry, pr.L_GREEDY, seed=pr.GREEDY_SEED)
    ck = pr.GreedyChecker(oracle_mod, dict(kw, episode_length=pr.L_GREEDY), B, pr.GREEDY_SEED)

    def follow(t, r, want):
        env.step_device(torch.from_numpy(want).cuda())

    wrong = ck.run(lambda c, r: _policy(env, "reward_greedy"), pr.T_GREEDY, follow)
    assert wrong == 0
    np.testing.assert_array_equal(env.field("avg_load_served").cpu().numpy(), ck.cur.field("loads"))  # in step
    assert env.status() == 0


def _reward64(env):
    """The float64 rewards of the last lb_step (lb_reward64: an array inside the state blob)."""
    off = env._rew64.value - env.state.data_ptr()
    return env.state[off:off + 8 * env.num_envs].view(torch.float64)


@pytest.mark.parametrize("B,kw,geometry", [
    (67, dict(num_endpoints=64, reward_function="multi"), "auto"),
    (9, dict(num_endpoints=256, reward_function="fairness"), "auto"),
    (32771, dict(num_endpoints=20, reward_function="multi"), "auto"),
    (40000, dict(num_endpoints=6, reward_function="multi"), "tpe"),
])
def test_reward_greedy_equals_step_on_cloned_state(B, kw, geometry):
    """The sizes the replayed oracle is too slow for: for each action a, lb_step(a) on a copy of
    the state blob and its float64 reward; the policy's action is the first argmax.  Three
    states: after the reset, mid-episode, and in the episode after an auto-reset."""
    L = 5
    env = _env(B, kw, geometry, L)
    A = env.cfg.num_actions
    rew64 = _reward64(env)
    for s in range(L + 2):
        if s in (0, 3, L + 1):
            saved = env.state.clone()
            got = _policy(env, "reward_greedy")
            assert torch.equal(env.state, saved)  # the policy reads only
            r = torch.empty((A, B), dtype=torch.float64, device="cuda")
            for a in range(A):
                env.state.copy_(saved)
                env.step_device(torch.full((B,), a, dtype=torch.int32, device="cuda"))
                r[a] = rew64
            env.state.copy_(saved)
            r = r.cpu().numpy().T
            np.testing.assert_array_equal(got, pr.first_argmax(r), err_msg=f"after {s} steps")
            if kw["reward_function"] == "multi":
                assert (got != 0).mean() > 0.3  # (the check has something to find)
        env.step_device(None)
    assert env.status() == 0


ROLLOUT_SHAPES = [
    (4096, {}, "auto"),                                                        # slice layout, 16 lanes per env
    (3000, dict(num_endpoints=64, reward_function="multi"), "auto"),
    (40000, dict(num_endpoints=20, reward_function="fairness"), "auto"),       # 4-envs-per-wave slice
    (40000, dict(num_endpoints=6), "tpe"),                                     # k_rollout_tpe, 64-thread blocks
    (70000, {}, "tpe"),                                                        # k_rollout_tpe, 256-thread blocks
    (131072, {}, "tpe"),                                                       # a lean shape: falls to k_rollout_tpe
    (40000, dict(num_nodes=100), "tpe"),                                       # N > 64: K policy + step launches
]


@pytest.mark.parametrize("B,kw,geometry", ROLLOUT_SHAPES)
@pytest.mark.parametrize("kind", K8S)
@pytest.mark.parametrize("K,L", [(13, 5), (8, 20)])  # in-loop resets (L < K); next episodes drawn first (L >= K)
def test_rollout_equals_policy_plus_step(B, kw, geometry, kind, K, L):
    """lb_rollout under the new kinds == K x (lb_policy + lb_step), bit for bit, across auto-resets
    (the body of tests/test_gpu_api.py::test_rollout_equals_policy_plus_step)."""
    from lbk8s import LBVecEnv
    a_env = LBVecEnv(B, seed=21, as_tensors=True, episode_length=L, geometry=geometry, **kw)
    b_env = LBVecEnv(B, seed=21, as_tensors=True, episode_length=L, geometry=geometry, **kw)
    a_env.reset()
    b_env.reset()
    if B == 131072:  # the kinds 0..3 run a lean kernel here where L >= K; the new kinds have none
        assert a_env.rollout_kernel(K).startswith("k_rollout_lean") == (L >= K)
        assert a_env.rollout_kernel(K, kind=kind) == "k_rollout_tpe"
    elif geometry == "tpe":
        assert a_env.rollout_kernel(K, kind=kind) == ("policy+step launches" if kw.get("num_nodes", 24) > 64
                                                      else "k_rollout_tpe")
    else:
        assert a_env.rollout_kernel(K, kind=kind) == "k_rollout_slice"
    R = a_env.cfg.obs_rows
    obs = torch.empty((K, B, R, 8), device="cuda")
    rew = torch.empty((K, B), device="cuda")
    dn = torch.empty((K, B), dtype=torch.uint8, device="cuda")
    act = torch.empty((K, B), dtype=torch.int32, device="cuda")
    a_env.rollout(kind, K, obs_out=obs, reward_out=rew, done_out=dn, actions_out=act)
    for k in range(K):
        ak = b_env.policy(kind)
        assert torch.equal(act[k], ak), k
        b_env.step_device(ak)
        assert torch.equal(obs[k], b_env.obs), k
        assert torch.equal(rew[k], b_env.rewards), k
        assert torch.equal(dn[k], b_env.dones), k
    assert torch.equal(a_env.stats(), b_env.stats())
    assert torch.equal(a_env.terminal_obs, b_env.terminal_obs)
    assert torch.equal(a_env.ep_stats, b_env.ep_stats)
    for f in ("endpoint_latency", "endpoint_cpu_usage_percentage", "avg_load_served"):
        assert torch.equal(a_env.field(f), b_env.field(f)), f
    # the env goes on from where the rollout left it
    a_env.step_device(act[0])
    b_env.step_device(act[0])
    assert torch.equal(a_env.obs, b_env.obs)
    assert a_env.status() == 0


@pytest.mark.parametrize("policy,extra", [("least_latency", {}), ("reward_greedy", {}),
                                          ("reward_greedy", dict(reward_function="multi"))])
def test_run_baselines_new_policies(tmp_path, policy, extra):
    """run_baselines under a new kind: the returns of a per-step policy + step loop on an
    identically seeded env, and one CSV row per episode."""
    from lbk8s import LBVecEnv
    from lbk8s.info import ST_RETURN
    from lbk8s.run_baselines import CFG1, baseline_file_name, run_baselines, write_csvs
    n = 50
    res = run_baselines(policy=policy, n_episodes=n, num_endpoints=6, **extra)
    kw = dict(CFG1, num_endpoints=6, **extra)
    env = LBVecEnv(n, seed=42, env_id_offset=0, auto_reset=False, as_tensors=True, geometry="slice", **kw)
    env.reset()
    for _ in range(env.cfg.episode_length):
        env.step_device(env.policy(policy))
    np.testing.assert_array_equal(res["returns"], env.stats()[:, ST_RETURN].cpu().numpy())
    if kw["reward_function"] == "naive":
        assert (res["returns"] == 100.0).all()  # every accept pays 1.0; reward_greedy plays action 0
    assert len(res["csv_results"]) == len(res["csv_no_cost_updated"]) == n
    name = baseline_file_name(0, policy, 6)
    write_csvs(res, name, str(tmp_path))
    for f in (name + ".csv", "no_cost_updated.csv"):
        assert len((tmp_path / f).read_text().splitlines()) == n
