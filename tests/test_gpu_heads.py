"""lb_ppo_head, lb_dqn_head (both kernels), lb_episode_log and lb_replay_sample pinned to the
references of tests/heads_ref.py: float64 autograd for the two loss heads, an exact numpy model
for the episode log, the C oracle's draws for the replay sample
(tests/test_heads_ref_harness.py shows on the CPU that the checkers accept float32 stand-ins of
the kernels' documented formulas on every case and refuse fifteen broken ones).

The kernels are called through the C ABI (_native.lib()), where the Python wrappers hide a path:
loss_out NULL at small M, td_out / old_out NULL, masks NULL, ep_r32 / reward64 NULL.  Every
output buffer arrives filled with NaN (int64: a sentinel) and longer than the kernel may write.

Cases (heads_ref.PPO_CASE_NAMES, DQN_CASES, eplog_specs(), SAMPLE_CASES): the smallest shapes
that reach each path -- R on both sides of every 64-row register slot of k_ppo_head with the
taken action on both sides too, M = 517 (a ragged last block) and 1 .. 5, M = 4 * 8192 + 5 and
4 * 65535 + 5 (the two heads' loops over sets), exact ties of the PPO loss's max and clamp,
both DQN head kernels on the same inputs up to M = 1024 (bit for bit), episode-log waves that
are ragged, empty, full or cut by cap, and replay samples of an empty ring and of a counter
above 2^32.  The worst shares of the allowances seen on the MI355X are in DESIGN.md.
"""
import numpy as np
import pytest
import torch

import heads_ref as hr

pytestmark = pytest.mark.gpu


def _up(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _down(t):
    return None if t is None else t.cpu().numpy()


class HipDevice:
    def __init__(self):
        from lbk8s import _native
        self.native, self.L = _native, _native.lib()

    def _call(self, rc):
        self.native.check(rc)
        torch.cuda.synchronize()

    def ppo_head(self, c, bufs):
        ins = [_up(x) for x in (c.logits, c.masks, c.actions, c.oldlogp, c.adv, c.ret, c.vold, c.value)]
        out = {k: _up(v) for k, v in bufs.items()}
        self._call(self.L.lb_ppo_head(*[_ptr(t) for t in ins], c.M, c.R, float(c.clip), float(c.ent_coef),
                                      float(c.vf_coef), int(c.clip_vloss), out["dlogits"].data_ptr(),
                                      out["dvalue"].data_ptr(), out["terms"].data_ptr(), None))
        return {k: _down(v) for k, v in out.items()}

    def dqn_head(self, c, bufs, block):
        assert (bufs["loss"] is not None) == block
        ins = [_up(x) for x in (c.q, c.q_next, c.actions, c.rewards, c.dones)]
        out = {k: _up(v) for k, v in bufs.items()}
        self._call(self.L.lb_dqn_head(*[t.data_ptr() for t in ins], c.M, c.R, float(c.gamma), out["dq"].data_ptr(),
                                      out["sq_err"].data_ptr(), _ptr(out["td"]), _ptr(out["old"]), _ptr(out["loss"]),
                                      None))
        return {k: _down(v) for k, v in out.items()}

    def episode_log(self, B, done, ep_stats, reward, reward64, actions, ret32, ep_r32, tag, log, cap, count):
        done, ep_stats, reward, reward64, actions = (_up(x) for x in (done, ep_stats, reward, reward64, actions))
        ret32, ep_r32, log = _up(ret32), _up(ep_r32), _up(log)
        cnt = _up(count.view(np.int32))
        self._call(self.L.lb_episode_log(B, done.data_ptr(), ep_stats.data_ptr(), reward.data_ptr(), _ptr(reward64),
                                         actions.data_ptr(), ret32.data_ptr(), _ptr(ep_r32), tag, log.data_ptr(), cap,
                                         cnt.data_ptr(), None))
        return _down(ret32), _down(ep_r32), _down(log), _down(cnt).view(np.uint32)

    def replay_sample(self, c, ring, bufs):
        key = (c.B, c.F, c.S)
        if getattr(self, "_ring_key", None) != key:   # (the 10 MB rings go up once)
            self._ring_key, self._ring = key, {k: _up(v) for k, v in ring.items()}
        r = self._ring
        out = {k: _up(v) for k, v in bufs.items()}
        vstep, base = _up(np.array([c.vstep], np.int64)), _up(np.array([c.base], np.int64))
        self._call(self.L.lb_replay_sample(
            c.B, c.F, c.S, c.batch, c.seed, vstep.data_ptr(), base.data_ptr(), r["rb_obs"].data_ptr(),
            r["rb_next_obs"].data_ptr(), r["rb_actions"].data_ptr(), r["rb_rewards"].data_ptr(),
            r["rb_dones"].data_ptr(), out["obs"].data_ptr(), out["next_obs"].data_ptr(), out["actions"].data_ptr(),
            out["rewards"].data_ptr(), out["dones"].data_ptr(), None))
        return {k: _down(v) for k, v in out.items()}


@pytest.fixture(scope="module")
def dev():
    return HipDevice()


def _fmt(shares):
    return " ".join(f"{k}={v:.3f}" for k, v in shares.items())


@pytest.mark.parametrize("name", hr.PPO_CASE_NAMES)
def test_ppo_head_matches_float64(dev, name):
    shares = hr.run_ppo(dev, name)
    print(f"ppo {name}: worst {max(shares.values()):.3f} | {_fmt(shares)}")


@pytest.mark.parametrize("spec", hr.DQN_CASES, ids=hr.dqn_case_id)
def test_dqn_head_matches_float64_and_kernels_agree(dev, spec):
    shares, bitwise = hr.run_dqn(dev, spec)
    assert bitwise is (True if spec[0] <= 1024 else None)
    for k, s in shares.items():
        print(f"dqn {hr.dqn_case_id(spec)} {k}: worst {max(s.values()):.3f} | {_fmt(s)}"
              + (" | kernels bit-equal" if bitwise else ""))


@pytest.mark.parametrize("spec", hr.eplog_specs(), ids=hr.eplog_id)
def test_episode_log_matches_exact_reference(dev, spec):
    hr.run_eplog(dev, spec)


@pytest.mark.parametrize("spec", hr.SAMPLE_CASES, ids=lambda s: s[0])
def test_replay_sample_matches_oracle_draws(dev, oracle_mod, spec):
    hr.run_sample(dev, spec, oracle_mod)
