"""lb_ds_sample between the row counts tests/test_gpu_ds_sample.py pins it at: the five-tile forward
at R = 66 and the chunked kernel (k_deepsets_fwd_big<5>) at R = 96, 97 (a 32-row chunk boundary and
one row past it), 129, 130 (where the env's layout goes from two to four endpoints per lane), 193
(the first row of ds_sample_wave's fourth slot) and 256, against the float64 definition through
tests/ds_sample_ref.py's checker, with every mask kind and the checker's tolerances as they are.
k_ppo_steps256 (csrc/lbk8s_ppo256.h) is held bit-equal to lb_ds_sample at these row counts
(tests/test_gpu_ppo_steps256.py); this is the base that equality rests on.
"""
import numpy as np
import pytest
import torch

import ds_sample_ref as sr
from ds_sample_ref import MASK_KINDS, Case, case_id
from test_gpu_ds_sample import image_of, launch, on_device, plain_forward

pytestmark = pytest.mark.gpu

BIG_CASES = [Case("sample", "ac", R, "B1", v, False)
             for R, v in ((66, (5, 1, 0)), (96, (0, 1, 0)), (97, (0, 1, 0)), (129, (0, 1, 0)), (130, (0, 1, 0)),
                          (193, (0, 1, 0)), (256, (0, 1, 0)))]


@pytest.mark.parametrize("c", BIG_CASES, ids=case_id)
def test_sample_big(c):
    s = sr.setup(c)
    net, x = on_device(s)  # (asserts the kernel variant of the case)
    B, R = s.B, c.R
    frag, u = image_of(net, c.heads), s.u.cuda()
    fwd = plain_forward(net, x, c.heads)
    out = {}
    for kind in MASK_KINDS:
        masks = sr.sample_masks(c, kind)
        md = None if masks is None else torch.from_numpy(masks).cuda()
        bufs = sr.alloc_outputs(B, R, c.heads, "cuda")
        launch(frag, x, md, u, bufs)
        got = sr.as_numpy(bufs)
        out[kind] = sr.check_sample(s, masks, s.u.numpy(), got, fwd=fwd)
        a = got["actions"][:B]
        if masks is not None:
            assert a[9] == R - 1, a[9]  # (set 9: only row R - 1 valid)
        if masks is None and R % 2 == 0:
            assert a[3] in (R // 2 - 1, R // 2), a[3]  # (the uniform set, u = 0.5 on a boundary)
    print("ds-sample-margin", case_id(c), out)
    assert all(v <= 1.0 for o in out.values() for v in o.values())
    assert np.array_equal(got["actions_f32"][:B], got["actions"][:B].astype(np.float32))
