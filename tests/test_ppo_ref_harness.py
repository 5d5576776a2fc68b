"""The PPO rollout's reference harness (tests/ppo_ref.py) checked on the CPU, with no GPU.

The device under test here is a stand-in: a second oracle as the env, torch's float32 CPU forward
of the same agent, the header's draw in float32 numpy (tests/test_ds_sample_ref.draw32) and
tests/ppo_tail_ref.ppo_record_ref, writing the buffers lb_ppo_steps writes, NaN / sentinel filled
with guard elements (tests/test_gpu_ppo_oracle.py runs the same harness on the three HIP kernels).

(a) The reference accepts a correct float32 implementation on every case of the GPU test: CASES is
    that test's table, validated here first -- the margins stay <= 1 and finish()'s coverage
    conditions hold (every env ended, one ended twice inside a launch longer than an episode, an
    action on row 0 and one on the last row, log rows in the logged cases).
(b) The checker catches what it claims to: fourteen stand-ins with one planted defect each change
    at least one output bit of the case and are refused.

CASES: (entry point, B, E, reject, L, steps of the launches, variant), from the tables of
tests/test_gpu_ppo_steps.py, test_gpu_ppo_steps64.py and test_gpu_ppo_steps256.py, every env with
reward_function="multi" and the envs out of phase (R = 1 on 3 envs, not that table's 1: an odd env
and the u = 1 - 2^-24 set are then there).  A plan of two launches feeds the second the
first's last observations (store_rows = steps on the first).  Variants, one case per kernel each:
"no_log" (log = NULL: ret32, ep_r32, log and count untouched), "cap" (the log holds half the
finished episodes) and "store_all" (store_rows = steps on the last launch too; the others steps - 1).
The two *_two_launches cases are the "4 + 5" plans of the HIP-against-HIP files.
"""
import numpy as np
import pytest
import torch

import ppo_ref
from dqn_ref import FIELDS
from ppo_ref import PAD, Bufs, PPOChecker
from ppo_tail_ref import LB_EPLOG_W, ppo_record_ref
from test_ds_sample_ref import draw32
from test_gpu_ppo_steps import CASES as C16
from test_gpu_ppo_steps64 import CASES as C64
from test_gpu_ppo_steps256 import CASES as C256

# The env seed is test_gpu_ppo_steps._env's.  The weight seed: a default-init agent gives the reject
# row (the last) a float64 probability far below the draw's tolerance under many seeds (5, _frag's,
# among them: 9e-8 at R = 129), and whether u = 1 - 2^-24 then takes it is a matter of float32
# rounding.  Under seed 6 the last row of that set holds at least 30 tol_of(R) in every case (the
# least: 34 at i_r129_epl4), so any implementation inside the tolerance takes it.
SEED, WSEED = 11, 6


def _rows(fn, table, names, plans=None, variants=None):
    out = {}
    for name in names:
        B, E, rej, L, steps = table[name]
        out[f"{fn[3:]}-{name}"] = (fn, B, E, rej, L, (plans or {}).get(name, (steps,)), (variants or {}).get(name))
    return out


CASES = {}
CASES.update(_rows("lb_ppo_steps", dict(C16, r1=(3,) + C16["r1"][1:]), ("r1", "run_py", "ragged", "r16", "r16_reject"),
                   dict(run_py=(7, 4), r16=(5, 3), r16_reject=(5, 3)),
                   dict(run_py="store_all", ragged="cap", r16="no_log")))
CASES.update(_rows("lb_ppo_steps64", C64, ("a_r17_w16", "b_w32", "c_r32", "d_r33_valu", "e_w64", "f_r49_ts4", "g_r64",
                                           "h_r65_config4", "j_more_groups_than_waves"),
                   None, dict(f_r49_ts4="no_log", h_r65_config4="cap", e_w64="store_all")))
CASES.update(_rows("lb_ppo_steps256", C256, ("b_r66", "d_r81", "h_r129_epl2", "i_r129_epl4", "k_r193_slot4", "m_r257",
                                             "o_more_envs_than_waves_r66"),
                   None, dict(i_r129_epl4="no_log", m_r257="cap", k_r193_slot4="store_all")))
CASES["ppo_steps64-c_r32_two_launches"] = ("lb_ppo_steps64",) + C64["c_r32"][:4] + ((4, 5), None)
CASES["ppo_steps256-d_r81_two_launches"] = ("lb_ppo_steps256",) + C256["d_r81"][:4] + ((4, 5), None)
assert C64["h_r65_config4"][3:] == (2, 9) and C256["o_more_envs_than_waves_r66"][0] == "8c+3"


def case_setup(case):
    """(kw, B, plan, uniforms, cap, with_log) of a CASES row."""
    fn, B, E, rej, L, steps, variant = case
    B = ppo_ref.batch_size(B)
    kw = dict(num_endpoints=E, rejection_allowed=rej, episode_length=L, reward_function="multi")
    plan = ppo_ref.launches(steps, variant == "store_all")
    T = sum(steps)
    ended = ppo_ref.episodes_ended(B, L, T)
    cap = ended // 2 if variant == "cap" else ended + 3
    assert cap >= 1
    return kw, B, plan, ppo_ref.uniforms(T, B, T * 1000 + B), cap, variant != "no_log"


BUGS = ("action_one_row_off", "logprob_of_another_row", "value_of_previous_obs", "uniforms_next_row",
        "ret32_two_roundings", "ret32_not_restarted", "ep_sum_adds_step_reward", "log_tag_off_by_one", "log_columns_of_previous_step",
        "dones_next_shifted", "obs_next_terminal", "last_obs_not_written", "reward64_of_step_before_last",
        "log_row_duplicated")


class StandIn:
    """A second oracle, the float32 torch forward, draw32 and ppo_record_ref; bug: one of BUGS."""

    def __init__(self, oracle_mod, agent, kw, B, seed, plan, u, cap, with_log=True, bug=None, phase=True):
        assert bug is None or bug in BUGS
        self.agent, self.bug, self.cap, self.with_log = agent, bug, cap, with_log
        self.orc = oracle_mod.OracleBatch(kw, B, trace=False, auto_reset=True, seed=seed)
        self.orc.init()
        self.reset_obs = self.obs = self.orc.reset()
        if phase and kw["episode_length"] > 1:
            o1 = self.orc.step(self.orc.policy_random())[0]
            odd = (np.arange(B) % 2).astype(np.uint8)
            self.obs = np.where(odd.astype(bool)[:, None, None], self.orc.reset(mask=odd), o1)
        self.env_obs = self.obs
        R = self.R = self.orc.R
        self.B, self.u = B, u.numpy()
        self.T = sum(n for n, _ in plan)
        S = self.T - (plan[-1][0] - plan[-1][1])
        self.n = ppo_ref.sizes(B, R, self.T, S, cap)
        fill = dict(actions_out=-77, done_out=0xAB, count=0)
        self.s = {k: np.full(self.n[k] + PAD, fill.get(k, np.nan), ppo_ref.DTYPES[k]) for k in Bufs.ALL}
        for k, v in ppo_ref.initial_values(B).items():
            self.s[k][:B] = v
        self.s["reward64"] = np.zeros(B, np.float64)
        self.t = 0
        self.log_rows = []
        self.prev_obs = self.prev_a = self.prev_r = self.prev_done = None
        self.planted = bug not in ("action_one_row_off",)

    def forward(self, x):
        with torch.no_grad():
            x = torch.from_numpy(np.ascontiguousarray(x))
            return self.agent.actor(x).numpy(), self.agent.critic(x).numpy()

    def draw(self, g, logits):
        B, R = self.B, self.R
        u = self.u[(g + 1) % self.T] if self.bug == "uniforms_next_row" else self.u[g]
        a, logprob = draw32(logits, None, u)
        env = np.arange(B)
        m = logits.max(1)
        lse = m + np.log(np.cumsum(np.exp(logits - m[:, None]), 1, dtype=np.float32)[:, -1])
        if self.bug == "action_one_row_off" and not self.planted and R > 1:
            # one set whose u lies at least 10 tol inside its interval takes the next row
            l64 = logits.astype(np.float64)
            p = np.exp(l64 - l64.max(1, keepdims=True))
            C = np.concatenate([np.zeros((B, 1)), np.cumsum(p / p.sum(1, keepdims=True), 1)], 1)
            room = np.minimum(u - C[env, a], C[env, a + 1] - u)
            inside = np.flatnonzero(room >= 10 * ppo_ref.sr.tol_of(R))
            if inside.size:
                b = inside[0]
                a[b] = (a[b] + 1) % R
                logprob[b] = logits[b, a[b]] - lse[b]
                self.planted = True
        if self.bug == "logprob_of_another_row":
            logprob = logits[env, (a + 1) % R] - lse
        return a.astype(np.int32), logprob.astype(np.float32)

    def run(self, n, store_rows, tag0):
        s, B, R, bug = self.s, self.B, self.R, self.bug
        x = self.env_obs if self.t == 0 else s["obs_next"][(self.t - 1) * B * R * 8:self.t * B * R * 8].reshape(B, R, 8)
        if bug != "obs_next_terminal":
            assert np.array_equal(x, self.obs)
        r64s = []
        for i in range(n):
            g = self.t + i
            row = slice(g * B, (g + 1) * B)
            logits, value = self.forward(self.obs)
            if bug == "value_of_previous_obs" and self.prev_obs is not None:
                value = self.forward(self.prev_obs)[1]
            a, logprob = self.draw(g, logits)
            s["actions_f32"][row], s["logprobs"][row], s["values"][row] = a, logprob, value
            o2, r2, d2, term, st2 = self.orc.step(a)
            r64s.append(self.orc.last_reward64())
            s["rewards"][row] = r2
            stats = s["ep_stats"][:B * 16].reshape(B, 16)
            stats[d2] = st2[d2]
            log = None
            if self.with_log:
                prev = bug == "log_columns_of_previous_step" and self.prev_a is not None
                log = dict(reward=self.prev_r if prev else r2,
                           reward64=None if bug == "ret32_two_roundings" else r64s[-1], actions=self.prev_a if prev else a, ret32=s["ret32"][:B], ep_r32=s["ep_r32"][:B],
                           tag=tag0 + i + (1 if bug == "log_tag_off_by_one" else 0), rows=[], count=0)
            own_sum = bug == "ep_sum_adds_step_reward"
            ndone = ppo_record_ref(d2.astype(np.uint8), stats, None if own_sum else s["ep_sum"][:B],
                                   None if own_sum else s["ep_cnt"][:B], log)
            if own_sum:
                s["ep_sum"][:B][d2] += r2[d2]
                s["ep_cnt"][:B][d2] += 1.0
            if log is not None:
                self.log_rows += log["rows"][::-1]  # (rows are unordered within a call)
                if bug == "ret32_not_restarted":
                    s["ret32"][:B][d2] = s["ep_r32"][:B][d2]
            obs_row = np.where(d2[:, None, None], term, o2) if bug == "obs_next_terminal" else o2
            done_row = ndone
            if bug == "dones_next_shifted":
                done_row = np.zeros(B, np.float32) if self.prev_done is None else self.prev_done
            if i < store_rows:
                s["dones_next"][row] = done_row
                s["obs_next"][g * B * R * 8:(g + 1) * B * R * 8] = obs_row.reshape(-1)
            else:
                s["last_done"][:B] = done_row
                if bug != "last_obs_not_written":
                    s["last_obs"][:B * R * 8] = obs_row.reshape(-1)
            s["actions_out"][:B], s["done_out"][:B] = a, d2
            self.prev_obs, self.prev_a, self.prev_r, self.prev_done = self.obs, a, r2, ndone
            self.obs = o2
        s["reward64"] = r64s[-2] if bug == "reward64_of_step_before_last" and n > 1 else r64s[-1]
        if self.with_log:
            s["count"][0] = len(self.log_rows)
            stored = min(len(self.log_rows), self.cap)
            if stored:
                rows = np.array(self.log_rows[:stored])
                if bug == "log_row_duplicated" and stored > 1:
                    rows[1] = rows[0]
                s["log"][:stored * LB_EPLOG_W] = rows.reshape(-1)
        self.t += n

    def read(self):
        return dict({k: v.copy() for k, v in self.s.items()}, obs=self.env_obs)

    def stats(self):
        return self.orc.stats()

    def field(self, name):
        return self.orc.field(dict(FIELDS)[name])

    def status(self):
        return 0


def run_case(oracle_mod, case, bug=None, check=True):
    """The case on a stand-in: under the checker, or (check=False) alone, returning what it wrote."""
    kw, B, plan, u, cap, with_log = case_setup(case)
    agent = ppo_ref.make_agent(WSEED)
    dev = StandIn(oracle_mod, agent, kw, B, SEED, plan, u, cap, with_log, bug)
    if not check:
        for n, store_rows in plan:
            dev.run(n, store_rows, ppo_ref.TAG_BASE + dev.t)
        assert dev.planted, "the defect found no place in this case"
        return dev.read()
    ref = PPOChecker(oracle_mod, agent, kw, B, SEED, plan, u, cap, with_log)
    return ppo_ref.run_plan(ref, dev, plan)


@pytest.mark.parametrize("name", list(CASES))
def test_reference_accepts_float32_stand_in(oracle_mod, name):
    ref = run_case(oracle_mod, CASES[name])
    print(f"\nppo-margin {name}: {ref.summary()}")
    assert max(ref.margins.values()) <= 1.0


def test_reference_accepts_stand_in_on_the_plain_reset_cases(oracle_mod):
    """tests/test_gpu_ppo256_oracle.py's four cases: a plain reset, every row stored, no log."""
    import ds_sample_ref as sr
    from test_gpu_ppo256_oracle import CASES as PLAIN, STEPS, B, L
    for R, (E, rej, wseed) in sorted(PLAIN.items()):
        kw = dict(num_endpoints=E, rejection_allowed=rej, reward_function="multi", episode_length=L)
        plan = [(STEPS, STEPS)]
        u = torch.rand((STEPS, B), generator=torch.Generator().manual_seed(R))
        u[0, 0], u[0, 1] = 0.0, sr.U_ONE
        agent = ppo_ref.make_agent(wseed)
        dev = StandIn(oracle_mod, agent, kw, B, 5, plan, u, 1, with_log=False, phase=False)
        ref = PPOChecker(oracle_mod, agent, kw, B, 5, plan, u, 1, with_log=False, phase=False)
        ppo_ref.run_plan(ref, dev, plan, last_row=False)
        assert ref.R == R and ref.ended.min() >= STEPS // L - 1 and ref.ended.max() >= 2


# the case of (b): two launches, the last with store_rows = steps - 1; the capped variant for the log
DEFECT_CASE = ("lb_ppo_steps", 67, 15, True, 2, (5, 3), None)
DEFECT_CASE_CAPPED = DEFECT_CASE[:6] + ("cap",)
# defect: the checker's message
MATCH = {
    "action_one_row_off": "interval",
    "logprob_of_another_row": "logprob",
    "value_of_previous_obs": "value",
    "uniforms_next_row": "interval",
    "ret32_two_roundings": "ret32|ep_r32",
    "ret32_not_restarted": "ret32",
    "ep_sum_adds_step_reward": "ep_sum",
    "log_tag_off_by_one": "log row",
    "log_columns_of_previous_step": "log row",
    "dones_next_shifted": "dones_next|last_done",
    "obs_next_terminal": "obs_next|last_obs",
    "last_obs_not_written": "last_obs",
    "reward64_of_step_before_last": "lb_reward64",
    "log_row_duplicated": "repeat",
}
assert set(MATCH) == set(BUGS)


@pytest.mark.parametrize("bug", BUGS)
def test_checker_catches_broken_stand_in(oracle_mod, bug):
    case = DEFECT_CASE_CAPPED if bug == "log_row_duplicated" else DEFECT_CASE
    clean, broken = run_case(oracle_mod, case, check=False), run_case(oracle_mod, case, bug, check=False)
    changed = [k for k in clean if not np.array_equal(ppo_ref.bits(clean[k]), ppo_ref.bits(broken[k]))]
    assert changed, f"{bug} changes no output bit of the case"
    run_case(oracle_mod, case)  # (the same case passes without the defect)
    with pytest.raises(AssertionError, match=MATCH[bug]):
        run_case(oracle_mod, case, bug)
