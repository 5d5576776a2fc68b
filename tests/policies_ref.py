"""References for the on-device policies LB_POLICY_ROUND_ROBIN .. LB_POLICY_REWARD_GREEDY
(include/lbk8s.h), shared by tests/test_policies_host.py (CPU) and tests/test_gpu_policies.py.

* round_robin / least_loaded / least_latency: numpy on the env's fields, first index on ties.
* reward_greedy: the C oracle by brute force.  For a decision after the action history h, a fresh
  OracleBatch of the same seed replays h and then steps action a, for every a in [0, A): its
  float64 reward (last_reward64) is what step(a) returns on that state.  The policy's action must
  be the first argmax.  Nothing of the reward's formula is restated on this side.
* reward_model: the reward's formula in numpy, with switchable defects, for the harness only
  (tests/test_policies_host.py shows the checker rejects each defect, and that the defect-free
  model equals the brute force bit for bit).

All comparisons are exact: both sides are float64 IEEE without contraction.
"""
import numpy as np

# the reward-greedy cases of the oracle check: name -> (B, env kwargs, geometry)
L_GREEDY, T_GREEDY = 7, 16  # episode length and decisions per env: the run crosses two episode ends
GREEDY_CASES = {
    "multi": (64, dict(reward_function="multi", latency_weight=0.7, cpu_weight=0.1, gini_weight=0.2), "auto"),
    "fairness_e6_tpe": (33, dict(num_endpoints=6, reward_function="fairness"), "tpe"),
    "latency_e3_norej": (40, dict(num_endpoints=3, reward_function="latency", rejection_allowed=False), "auto"),
    "multi100_e15": (20, dict(num_endpoints=15, reward_function="multi", latency_weight=1.0, cpu_weight=0.0,
                              gini_weight=0.0), "auto"),
    "naive": (16, dict(reward_function="naive"), "auto"),
    # a negative latency weight makes an accept pay down to -1.25, below the reject action's -1: the
    # one setting in which reject can be the argmax (with weights >= 0 every accept pays more than
    # the reject constant under all four reward functions)
    "multi_negative_reject": (24, dict(num_endpoints=5, reward_function="multi", latency_weight=-1.25, cpu_weight=0.0,
                                       gini_weight=0.0), "auto"),
}
GREEDY_SEED = 77


# ---- kinds 4..6 ---------------------------------------------------------------------------------

def round_robin(current_step, E):
    return (np.asarray(current_step).astype(np.int64) % E).astype(np.int32)


def least_loaded(avg_load_served):
    return np.argmin(np.asarray(avg_load_served), axis=1).astype(np.int32)  # first minimum


def least_latency(endpoint_latency, endpoint_topology_latency):
    s = np.asarray(endpoint_latency, np.float64) + np.asarray(endpoint_topology_latency).astype(np.float64)
    return np.argmin(s, axis=1).astype(np.int32)


K8S_REFS = {
    "round_robin": lambda f, E: round_robin(f("current_step"), E),
    "least_loaded": lambda f, E: least_loaded(f("avg_load_served")),
    "least_latency": lambda f, E: least_latency(f("endpoint_latency"), f("endpoint_topology_latency")),
}


def first_argmax(rewards):
    return np.argmax(rewards, axis=1).astype(np.int32)  # numpy: the first maximum


# ---- reward greedy: brute force on the oracle ---------------------------------------------------

class GreedyChecker:
    """Plays T decisions of B envs along the first-argmax trajectory and, at each, hands the
    policy under test the current state and compares its actions with the brute force."""

    def __init__(self, oracle_mod, kw, B, seed):
        self.oracle, self.kw, self.B, self.seed = oracle_mod, dict(kw), B, seed
        self.history = []
        self.cur = self._fresh()
        self.A = self.cur.R
        self.E = self.cur.E

    def _fresh(self):
        orc = self.oracle.OracleBatch(self.kw, self.B, trace=False, auto_reset=True, seed=self.seed)
        orc.init()
        orc.reset()
        return orc

    def rewards(self):
        """(B, A) float64: the reward step(a) returns on the current state, for every a."""
        out = np.empty((self.B, self.A), np.float64)
        for a in range(self.A):
            orc = self._fresh()
            for h in self.history:
                orc.step(h)
            orc.step(np.full(self.B, a, np.int32))
            out[:, a] = orc.last_reward64()
        return out

    def advance(self, actions):
        actions = np.asarray(actions, np.int32)
        self.history.append(actions)
        return self.cur.step(actions)

    def run(self, policy, T, on_decision=None):
        """policy(checker, rewards) -> (B,) actions.  Returns the number of decisions (env, t)
        at which the policy's action is not the first argmax; the trajectory follows the
        reference's choice either way.  on_decision(t, rewards, want) sees every decision."""
        wrong = 0
        for t in range(T):
            r = self.rewards()
            want = first_argmax(r)
            got = np.asarray(policy(self, r))
            wrong += int((got != want).sum())
            if on_decision is not None:
                on_decision(t, r, want)
            self.advance(want)
        return wrong


# ---- the reward's formula with switchable defects (harness only) --------------------------------

def _gini(loads, acc, E):
    """utils.py:132-143 as the kernels evaluate it: numerator sum_ij |x_i - x_j| (an integer)."""
    num = np.abs(loads[:, :, None] - loads[:, None, :]).sum(axis=(1, 2)).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        g = num / (np.float64(2 * E * E) * (acc.astype(np.float64) / np.float64(E)))
    return np.where(acc == 0, 0.0, g)


def _latency_after_increment(lat):
    """increase_endpoint_latency then decrease (the LAT table's recurrence)."""
    clamp = lambda v: np.maximum(np.minimum(v, 500.0), 1.0)
    return clamp(np.trunc(clamp(np.trunc(lat) * 1.5)) / 1.15)


def reward_model(orc, kw, defect=None):
    """(B, A) float64 rewards of every action on the oracle's current state, from its fields.
    defect: None, "gini_pre" (Gini of the loads before the accept), "cnt_lt" (the numerator update
    counts j' < j in place of j' <= j), "lat_after" (the selected latency after its increment),
    "wrong_zone" (the topology term of the next endpoint's zone)."""
    E, B = orc.E, orc.B
    fn = kw.get("reward_function", "naive")
    lw, cw, gw = (np.float64(kw.get(k, d)) for k, d in (("latency_weight", 0.7), ("cpu_weight", 0.1),
                                                       ("gini_weight", 0.2)))
    lat, topo, cpu = orc.field("ep_lat"), orc.field("ep_topo"), orc.field("ep_cpu")
    loads = orc.field("loads").astype(np.int64)
    if defect == "lat_after":
        lat = _latency_after_increment(lat)
    if defect == "wrong_zone":
        topo = np.roll(topo, -1, axis=1)
    acc = loads.sum(axis=1)
    out = np.empty((B, orc.R), np.float64)
    for e in range(E):
        after = loads.copy()
        after[:, e] += 1
        if defect == "gini_pre":
            g = _gini(loads, acc, E)
        elif defect == "cnt_lt":
            num = np.abs(loads[:, :, None] - loads[:, None, :]).sum(axis=(1, 2))
            cnt = (loads < loads[:, e:e + 1]).sum(axis=1)
            num = (num + 2 * (2 * cnt - (E - 1))).astype(np.float64)
            g = num / (np.float64(2 * E * E) * ((acc + 1).astype(np.float64) / np.float64(E)))
        else:
            g = _gini(after, acc + 1, E)
        s = lat[:, e] + topo[:, e]
        if fn == "naive":
            r = np.ones(B)
        elif fn == "latency":
            r = -s
        elif fn == "fairness":
            r = 1.0 - g
        else:
            r = (lw * (1.0 - (s - 2.0) / 998.0) + cw * (1.0 - (cpu[:, e] - 1.0) / 99.0)) + gw * (1.0 - g)
        out[:, e] = r
    if orc.R > E:
        out[:, E] = -1000.0 if fn == "latency" else -1.0
    return out
