"""GPU tests (-m gpu) of the encode kernel on waves whose lanes code at very different rates (tests/dry_lanes_common.py),
through the C ABI: steps with dry lanes ride the masked steady path for all 64 lanes.  Every channel of every case against oracle.orc.encode_i32: stream bytes, bit count, status."""
import os
import sys

import numpy as np
import pytest

from __graft_entry__ import load_package
from oracle import orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dry_lanes_common as dl  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; the product has no CPU fallback"
    c = load_package().Context(0)
    yield c
    c.close()


def encode_dev(ctx, x, adaptive=1):
    import torch
    T, Cn = x.shape
    cap = (orc.lib().orc_dega_worst_case_bytes(T) + 3) & ~3
    xd = torch.from_numpy(x).cuda()
    out = torch.zeros((Cn, cap), dtype=torch.uint8, device="cuda")
    bits = torch.zeros(Cn, dtype=torch.int64, device="cuda")
    err = torch.full((Cn,), 99, dtype=torch.int32, device="cuda")
    ret = load_package().library().dega_hip_encode_dev(ctx._h, xd.data_ptr(), Cn, T, Cn, adaptive, 32, out.data_ptr(), cap, bits.data_ptr(), err.data_ptr(), None)
    assert ret == 0
    torch.cuda.synchronize()
    return out.cpu().numpy(), bits.cpu().numpy().astype(np.uint64), err.cpu().numpy()


CASES = {
    "mixed192": lambda: dl.mixed_rates(192, 3000, seed=11),
    "ragged192": lambda: dl.ragged(192, 3000, seed=13),       # three full waves: the workgroup's fourth group has no channel
    "ragged164": lambda: dl.ragged(164, 3000, seed=14),       # ... and a last wave with 36 of its 64 channels
    "halving192": lambda: dl.halving_with_dry_lanes(192, 3000, seed=15),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_dry_lane_cases_equal_the_oracle(ctx, name):
    x = CASES[name]()
    out, bits, err = encode_dev(ctx, x)
    dl.assert_equals_oracle(name, x, 1, out, bits, err)


def test_three_long_channels_with_idle_helpers(ctx):
    """one wave of three channels x 20 000 samples: its helpers have nothing to do nearly all the time"""
    x = dl.from_amplitudes([50, 0, 3000], 20000, seed=16)
    out, bits, err = encode_dev(ctx, x)
    dl.assert_equals_oracle("three", x, 1, out, bits, err)


def test_mixed_rates_over_two_launches_with_saved_state(ctx):
    """dega_hip_encode_segment_dev: lanes run dry at the end of a launch that is not the last one"""
    import torch
    x = dl.mixed_rates(192, 3000, seed=11)
    out, bits, err = ctx.encode_segments(torch.from_numpy(x).cuda(), [0, 1500, 3000], adaptive=1, cap=(orc.lib().orc_dega_worst_case_bytes(3000) + 3) & ~3)
    torch.cuda.synchronize()
    dl.assert_equals_oracle("mixed192", x, 1, out.cpu().numpy(), bits.cpu().numpy().astype(np.uint64), err.cpu().numpy(), "two launches")
