"""An independent float32 reference of GAE with the time-limit bootstrap (lb_gae_tl,
include/lbk8s_abi_ppo_tl.h), written segment by segment and not as the header's recurrence.

Each env's timeline is split at its `done` boundaries: step t closes a segment when the flag after
it is set (dones[t + 1], or next_done at t = T - 1).  Inside a segment plain GAE runs backwards from
the segment's last step with last = 0; a segment that a done closed bootstraps its last step from
term_values there, the open segment at the end of the rollout from next_value.  No product with
(1 - done) appears anywhere.  The float32 operations are the header's in the header's order --
delta = (r + g * bv) - v, last = delta + gl * last -- and a segment's last step takes
last = delta + 0, which is what the recurrence's (gl * 0) * last term adds for finite inputs (up to
the sign of an exactly zero delta, which random data does not produce).  So the two agree bit for
bit on the test inputs, and an implementation that bootstraps from the wrong value, does not cut
the chain, or reads another row differs in at least one bit there.
"""
import numpy as np

F = np.float32


def constants(gamma, gae_lambda):
    """g = (float)gamma, gl = (float)(gamma * gae_lambda), the product in double."""
    return F(gamma), F(float(gamma) * float(gae_lambda))


def gae_tl_ref(rewards, values, dones, next_value, next_done, term_values, gamma, gae_lambda):
    """(advantages, returns), (T, B) float32 each, from float32 numpy inputs."""
    rewards, values, dones, term_values = (np.asarray(x, F) for x in (rewards, values, dones, term_values))
    next_value, next_done = np.asarray(next_value, F).reshape(-1), np.asarray(next_done, F).reshape(-1)
    T, B = rewards.shape
    g, gl = constants(gamma, gae_lambda)
    adv = np.full((T, B), np.nan, F)
    for b in range(B):
        after = [dones[t + 1, b] if t + 1 < T else next_done[b] for t in range(T)]  # the flag after step t
        ends = [t for t in range(T) if after[t] != 0]
        if not ends or ends[-1] != T - 1:
            ends.append(T - 1)  # the open segment
        start = 0
        for e in ends:
            closed = after[e] != 0
            boot = term_values[e, b] if closed else next_value[b]
            last = F(0)
            for t in range(e, start - 1, -1):
                nxt = boot if t == e else values[t + 1, b]
                delta = F(F(rewards[t, b] + F(g * nxt)) - values[t, b])
                last = F(delta + F(0)) if t == e else F(delta + F(gl * last))
                adv[t, b] = last
            start = e + 1
    assert not np.isnan(adv).any()
    return adv, (adv + values).astype(F)


def make_case(T, B, seed, no_done=False):
    """Random float32 inputs with the dones where an implementation can go wrong: per env index mod
    6 -- the first step ends an episode (dones[1]), the last one does (next_done), two consecutive
    steps do, next_done alone, a random pattern, none (T = 1: next_done in place of dones[1]).
    term_values is nonzero everywhere (an implementation must ignore it where no done is set) and
    unlike values."""
    rng = np.random.default_rng(seed)
    c = dict(rewards=rng.standard_normal((T, B)), values=rng.standard_normal((T, B)) * 3,
             next_value=rng.standard_normal(B) * 3, term_values=rng.standard_normal((T, B)) * 5 + 20)
    dones, next_done = np.zeros((T, B)), np.zeros(B)
    if not no_done:
        for b in range(B):
            k = b % 6
            if k == 0 and T > 1:
                dones[1, b] = 1
            elif k == 0:
                next_done[b] = 1  # (a one-step rollout: its only boundary)
            elif k == 1:
                next_done[b] = 1
                if T > 1:
                    dones[T - 1, b] = 1  # the step before the last ended one too
            elif k == 2 and T > 2:
                m = 1 + (b // 6) % (T - 2)
                dones[m, b] = dones[m + 1, b] = 1
            elif k == 3:
                next_done[b] = 1
            elif k == 4:
                dones[:, b] = rng.random(T) < 0.3
                next_done[b] = rng.random() < 0.5
        dones[0] = rng.random(B) < 0.5  # (the flag before step 0: GAE does not read it)
    c.update(dones=dones, next_done=next_done)
    return {k: np.ascontiguousarray(v, F) for k, v in c.items()}


ORDER = ("rewards", "values", "dones", "next_value", "next_done", "term_values")
GAMMA, LAMBDA = 0.95, 0.97  # PPO_DeepSets' defaults


def bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def check_gae_tl(fn, case, gamma=GAMMA, gae_lambda=LAMBDA):
    """fn(rewards, values, dones, next_value, next_done, term_values, gamma, gae_lambda) ->
    (advantages, returns) as arrays: bit-equal to gae_tl_ref on the case, else AssertionError."""
    want_adv, want_ret = gae_tl_ref(*(case[k] for k in ORDER), gamma, gae_lambda)
    adv, ret = fn(*(case[k] for k in ORDER), gamma, gae_lambda)
    for name, got, want in (("advantages", adv, want_adv), ("returns", ret, want_ret)):
        got = np.asarray(got)
        assert got.shape == want.shape, f"gae_tl: {name} has shape {got.shape}, not {want.shape}"
        bad = np.argwhere(bits(got) != bits(want))
        assert bad.size == 0, (f"gae_tl: {name}[{bad[0][0]}][{bad[0][1]}] = {got[tuple(bad[0])]!r}, the reference has "
                               f"{want[tuple(bad[0])]!r} ({len(bad)} of {want.size} differ)")
