"""The CLI's --test-fused-e256 and --test-sweep (lbk8s/cli.py): parsing only, no GPU.  What the flags
run is tests/test_gpu_eval256_fused.py's.
"""
import pytest


def _parse(*argv):
    from lbk8s import cli
    return cli.build_parser().parse_args(list(argv))


def test_flags_parse_and_default_off():
    from lbk8s import cli
    off = _parse()
    assert off.test_fused_e256 is False and off.test_sweep is None and cli.sweep_endpoints(off) is None
    assert cli.eval_launch_flags(off) == dict(fused=False, e64=False, e256=False)
    on = _parse("--test-fused-e256")
    assert on.test_fused_e256 is True and on.test_fused_e64 is False and on.test_fused is False
    assert cli.eval_launch_flags(on) == dict(fused=True, e64=False, e256=True)
    # the older flags keep their meaning
    assert cli.eval_launch_flags(_parse("--test-fused-e64")) == dict(fused=True, e64=True, e256=False)
    assert cli.eval_launch_flags(_parse("--test-fused")) == dict(fused=True, e64=False, e256=False)


def test_sweep_without_a_value_is_the_reference_list():
    from lbk8s import cli, evaluate
    args = _parse("--testing", "--test-sweep")
    assert cli.sweep_endpoints(args) == evaluate.SWEEP_ENDPOINTS == (6, 12, 16, 24, 32, 48, 64, 80, 128, 150, 180)
    # (the bare flag in front of another flag too)
    assert cli.sweep_endpoints(_parse("--test-sweep", "--test-fused-e256")) == evaluate.SWEEP_ENDPOINTS


def test_sweep_comma_list():
    from lbk8s import cli
    assert cli.sweep_endpoints(_parse("--test-sweep", "6,80,180")) == (6, 80, 180)
    assert cli.sweep_endpoints(_parse("--test-sweep=128")) == (128,)
    for bad in ("6,x", "", "0,6", "6;80"):
        with pytest.raises(SystemExit):
            _parse("--test-sweep", bad)


def test_test_sequential_wins():
    from lbk8s import cli
    args = _parse("--test_sequential", "--test-fused-e256", "--test-sweep", "6,80")
    assert cli.sweep_endpoints(args) is None
    assert cli.eval_launch_flags(args) == dict(fused=False, e64=False, e256=False)
