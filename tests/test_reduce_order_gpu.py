"""The order of the fixed-order float64 block reductions (csrc/reduce_device.h), pinned: two entry points whose addends are
exact must equal the numpy restatement of the order (tests/reduce_ref.py) bit for bit.  tests/test_reduce_ref_cpu.py shows
that the same sums in another order have other bits."""
import numpy as np
import pytest
import torch

import reduce_ref as RR
from diffsep_amd import ops

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_gram_is_the_stated_order():
    # 1024 threads = 16 waves; 3000 samples: threads hold 2 or 3 addends
    ref, est = RR.gram_case()
    got = ops.gram(torch.from_numpy(ref).cuda(), torch.from_numpy(est).cuda()).cpu().numpy()
    want = RR.gram_expected(ref, est)
    assert got.shape == want.shape == (3, 3, 2, 2)
    assert np.array_equal(bits64(got), bits64(want)), np.argwhere(bits64(got) != bits64(want))


def test_longform_cross_gram_is_the_stated_order():
    # 256 threads on each of the 16 contiguous shares of an overlap, the block partials then in block order
    win = RR.longform_case()
    c = RR.LF_CASE
    _, _, gram = ops.longform_stitch(torch.from_numpy(win).cuda(), c["T"], c["Tv"], want_gram=True)
    got = gram.cpu().numpy()
    want = RR.longform_expected(win)
    assert got.shape == want.shape == (6, 3, 3)
    assert np.array_equal(bits64(got), bits64(want)), np.argwhere(bits64(got) != bits64(want))
