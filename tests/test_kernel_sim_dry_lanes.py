"""The encode kernel under the emulator of tests/sim/ on waves whose lanes code at very different rates (see
tests/dry_lanes_common.py): steps with dry lanes ride the masked steady path for all 64 lanes.
Every channel against oracle.orc.encode_i32; the emulator's step counts say which path ran."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dry_lanes_common as dl  # noqa: E402
from sim_build import sim_library  # noqa: E402

STEADY, MASKED, OTHER, WAITS, DRY, OTHER_FOR_DRY_ONLY = range(6)


@pytest.fixture(scope="module")
def sim():
    S = sim_library("dry_lanes")  # the emulator's entry points and the getter of its step counts
    S.sim_encode.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    S.sim_set_drag.argtypes = [C.c_int, C.c_int]
    S.sim_encode_step_counts.argtypes = [C.c_void_p, C.c_int]
    S.sim_encode_step_counts.restype = None
    return S


def encode(S, x, adaptive):
    """(out, bits, err, step counts of this launch)"""
    T, Cn = x.shape
    cap = (orc.lib().orc_dega_worst_case_bytes(T) + 3) & ~3
    out = np.zeros((Cn, cap), dtype=np.uint8)
    bits = np.zeros(Cn, dtype=np.uint64)
    err = np.full(Cn, 99, dtype=np.int32)
    S.sim_encode_step_counts(None, 1)
    assert S.sim_encode(x.ctypes.data, Cn, T, Cn, adaptive, out.ctypes.data, cap, bits.ctypes.data, err.ctypes.data) == 0
    counts = np.zeros(6, dtype=np.uint64)
    S.sim_encode_step_counts(counts.ctypes.data, 1)
    return out, bits, err, counts


@pytest.fixture(scope="module")
def mixed():
    return dl.mixed_rates()


def test_mixed_rate_wave_rides_the_masked_steady_path(sim, mixed):
    """(a) the streams are the oracle's; steps with a dry lane were taken as steady ones, and none of the steps on the
    general route was there for a dry lane's sake alone.  (Many steps stay on that route here: a constant channel's counts
    are so skewed that its class is FAST4 or BITS, and a dry lane of a slow class keeps its wave there.)"""
    out, bits, err, n = encode(sim, mixed, 1)
    dl.assert_equals_oracle("mixed", mixed, 1, out, bits, err)
    print("steps", n.tolist())
    assert n[DRY] > 0
    assert n[OTHER_FOR_DRY_ONLY] == 0


def test_one_heavy_lane(sim):
    x = dl.one_heavy_lane()
    out, bits, err, n = encode(sim, x, 1)
    dl.assert_equals_oracle("heavy", x, 1, out, bits, err)
    assert n[DRY] > 0 and n[OTHER_FOR_DRY_ONLY] == 0


def test_ragged_last_wave(sim):
    x = dl.ragged()
    out, bits, err, n = encode(sim, x, 1)
    dl.assert_equals_oracle("ragged", x, 1, out, bits, err)
    assert n[OTHER_FOR_DRY_ONLY] == 0


def test_static_model(sim, mixed):
    out, bits, err, n = encode(sim, mixed, 0)
    dl.assert_equals_oracle("mixed", mixed, 0, out, bits, err)
    assert n[DRY] > 0 and n[OTHER_FOR_DRY_ONLY] == 0


@pytest.mark.parametrize("from_wave", (4, 8))
def test_slowed_waves(sim, mixed, from_wave):
    """(e) waves 4 .. 7 of a workgroup code, 8 .. 11 write.  Slow from wave 4 on: the filler idles for long stretches and
    every ring runs full.  Slow writers only: the coder waits for room in the raw ring while some of its lanes are dry."""
    sim.sim_set_drag(from_wave, 30)
    try:
        out, bits, err, n = encode(sim, mixed, 1)
    finally:
        sim.sim_set_drag(1 << 30, 0)
    dl.assert_equals_oracle("mixed", mixed, 1, out, bits, err, ("drag", from_wave))
    assert n[DRY] > 0 and n[OTHER_FOR_DRY_ONLY] == 0


def test_halving_with_dry_lanes(sim):
    x = dl.halving_with_dry_lanes()
    out, bits, err, n = encode(sim, x, 1)
    dl.assert_equals_oracle("halving", x, 1, out, bits, err)
    assert n[DRY] > 0 and n[OTHER_FOR_DRY_ONLY] == 0
