"""Numpy models of lb_gae and lb_ppo_record (include/lbk8s.h, ABI 17): the yardsticks of
tests/test_gpu_ppo_tail.py, themselves pinned on the CPU by tests/test_ppo_tail_ref.py.

gae_ref: the recurrence of envs/ppo_deepset.py:192-205 in float32, in exactly the op order the
header documents (every intermediate a float32 array, so numpy rounds after each op and cannot
contract).  ppo_record_ref: the per-env bookkeeping with sequential float64 adds, and the
episode log as lb_episode_log documents it.
"""
import os

import numpy as np

LB_ST_K, LB_ST_RETURN = 16, 0
LB_EPLOG_W = 24
LB_EPLOG_RET32, LB_EPLOG_REWARD, LB_EPLOG_ACTION, LB_EPLOG_ENV, LB_EPLOG_TAG = 16, 17, 18, 19, 20

GOLDEN_GAE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nn_gae.npz")


def gae_ref(rewards, values, dones, next_value, next_done, gamma, gae_lambda):
    """(advantages, returns), float32 (T, B)."""
    f32 = np.float32
    r, v, d = (np.ascontiguousarray(x, dtype=f32) for x in (rewards, values, dones))
    T, B = r.shape
    nv = np.asarray(next_value, dtype=f32).reshape(B)
    nd = np.asarray(next_done, dtype=f32).reshape(B)
    g = f32(gamma)
    gl = f32(float(gamma) * float(gae_lambda))  # the product in double, rounded once
    adv = np.zeros((T, B), f32)
    ret = np.zeros((T, B), f32)
    last = np.zeros(B, f32)
    one = f32(1.0)
    for t in reversed(range(T)):
        nnt = one - (nd if t == T - 1 else d[t + 1])
        nxt = nv if t == T - 1 else v[t + 1]
        delta = (r[t] + (g * nxt) * nnt) - v[t]
        last = delta + (gl * nnt) * last
        assert last.dtype == f32 and delta.dtype == f32
        adv[t] = last
        ret[t] = last + v[t]
    return adv, ret


def gae_inputs(T, B, p_done, seed, scale=100.0):
    """Seeded inputs: rewards ~ N(0, 1), values ~ scale * N(0, 1), dones / next_done Bernoulli(p_done)."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    return dict(rewards=rng.standard_normal((T, B)).astype(f32),
                values=(scale * rng.standard_normal((T, B))).astype(f32),
                dones=(rng.random((T, B)) < p_done).astype(f32),
                next_value=(scale * rng.standard_normal(B)).astype(f32),
                next_done=(rng.random(B) < p_done).astype(f32))


def gae_fixture():
    """The reference's own learn() tensors (tests/golden/gen_golden_gae.py): T = 24, B = 4."""
    d = np.load(GOLDEN_GAE)
    return {k: d[k] for k in d.files}


def ppo_record_ref(done, ep_stats, ep_sum, ep_cnt, log=None):
    """One lb_ppo_record call.  done (B,) u8, ep_stats (B, LB_ST_K) f64; ep_sum / ep_cnt (B,) f64
    or None, updated in place.  log: None, or a dict(reward f32, reward64 f64 | None, actions i32,
    ret32 f32, ep_r32 f32 | None, tag, rows (list, appended in env order), count (int)), updated
    in place (no cap: which rows a full log keeps is unordered, 'count' counts them all).
    Returns next_done (B,) f32."""
    B = done.shape[0]
    next_done = np.where(done != 0, np.float32(1), np.float32(0)).astype(np.float32)
    for b in range(B):
        if done[b] and ep_sum is not None:
            ep_sum[b] = ep_sum[b] + ep_stats[b, LB_ST_RETURN]
            ep_cnt[b] = ep_cnt[b] + 1.0
    if log is None:
        return next_done
    if log["reward64"] is not None:  # VecMonitor: one rounding of the float64 sum
        r32 = (log["ret32"].astype(np.float64) + log["reward64"]).astype(np.float32)
    else:
        r32 = (log["ret32"] + log["reward"]).astype(np.float32)
    for b in range(B):
        if not done[b]:
            log["ret32"][b] = r32[b]
            continue
        log["ret32"][b] = 0.0
        if log["ep_r32"] is not None:
            log["ep_r32"][b] = r32[b]
        row = np.zeros(LB_EPLOG_W)
        row[:LB_ST_K] = ep_stats[b]
        row[LB_EPLOG_RET32], row[LB_EPLOG_REWARD] = float(r32[b]), float(log["reward"][b])
        row[LB_EPLOG_ACTION], row[LB_EPLOG_ENV], row[LB_EPLOG_TAG] = float(log["actions"][b]), float(b), float(log["tag"])
        log["rows"].append(row)  # (the caller applies cap: which rows a full log keeps is unordered)
        log["count"] += 1
    return next_done


def sort_rows(rows):
    """Log rows ordered by (tag, env): rows are unordered within a call."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, LB_EPLOG_W)
    return rows[np.lexsort((rows[:, LB_EPLOG_ENV], rows[:, LB_EPLOG_TAG]))]


def done_pattern(kind, B, rng):
    """The done patterns of the record tests: 'none', 'all', ('one', i), ('p', prob)."""
    d = np.zeros(B, np.uint8)
    if kind == "all":
        d[:] = 1
    elif isinstance(kind, tuple) and kind[0] == "one":
        if kind[1] < B:
            d[kind[1]] = 1
    elif isinstance(kind, tuple) and kind[0] == "p":
        d[:] = rng.random(B) < kind[1]
    elif kind != "none":
        raise ValueError(kind)
    return d
