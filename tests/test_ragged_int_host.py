"""Ragged batches of integer samples without a GPU: the counted integer instantiations of the encode kernel -- int32,
the narrow value sizes, byte-swapped words, int64 containers -- compiled by g++ under the thread-per-lane emulator
(tests/sim/sim_ragged_int.cpp, through the launch table the library dispatches from), on the steered input of
tests/ragged_int_common.py, every channel bit for bit against the oracle's chain on that channel's own first count[c]
samples.  Whole channels in one launch, with the rings run full, with counts above T, and over several launches with a
segment state.  Then the new symbols of the C ABI and the Python-side assertions of encode_job(count=), which fail before
any library call.  The library itself is held to the same input in tests/test_gpu_ragged_int.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from __graft_entry__ import load_package

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ragged_int_common as ri  # noqa: E402
from sim_build import sim_library  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dega_hip_encode_var_dev", "dega_hip_encode64_var_dev", "dega_hip_encode_segment_var_dev", "dega_hip_encode_var_job_host",
               "dega_hip_group_encode_var")
CUTS = [0, 1, 8, 9, 64, 200, ri.T]


@pytest.fixture(scope="module")
def sim():
    S = sim_library("ragged_int")
    P, Z, I = C.c_void_p, C.c_size_t, C.c_int
    S.sim_encode_int_var.argtypes = [P, Z, Z, Z, P, I, I, I, I, P, Z, P, P]
    S.sim_encode_int_var_segments.argtypes = [P, Z, Z, Z, P, I, I, I, I, P, I, P, Z, P, P]
    S.sim_ragged_int_set_drag.argtypes = [I, I]
    return S


def slab_cap(kind):
    vs = ri.KINDS[kind][0]
    return 4 * ((ri.T * (2 * vs + 3) // 8 + 64) // 4 + 4)  # the worst case of T codewords of 2 * vs + 1 bits, and the coder's tail


def emulate(sim, kind, x, count, cuts=None):
    vs, ad, be, wide = ri.KINDS[kind]
    rows, Cn = x.shape
    cap = slab_cap(kind)
    out = np.full((Cn, cap), 0xA5, dtype=np.uint8)
    bits = np.full(Cn, 0xDEAD, dtype=np.uint64)
    err = np.full(Cn, 77, dtype=np.int32)
    count = np.ascontiguousarray(count, dtype=np.uint64)
    if cuts is None:
        r = sim.sim_encode_int_var(x.ctypes.data, Cn, rows, Cn, count.ctypes.data, int(wide), int(be), ad, vs, out.ctypes.data, cap, bits.ctypes.data,
                                   err.ctypes.data)
    else:
        cz = (C.c_size_t * len(cuts))(*cuts)
        r = sim.sim_encode_int_var_segments(x.ctypes.data, Cn, rows, Cn, count.ctypes.data, int(wide), int(be), ad, vs, cz, len(cuts), out.ctypes.data, cap,
                                            bits.ctypes.data, err.ctypes.data)
    assert r == 0
    return out, bits, err


# ---- the steered input is what it claims to be -----------------------------------------------------------------------------

def test_steered_counts_and_poison():
    for arrangement in ("full", "short"):
        count = ri.counts(arrangement)
        assert count.size == ri.C and count[:64].min() == 0 and count[:64].max() == ri.T
        assert set([0, 1, 3, 4, 5, 7, 8, 9, 16, ri.T - 1, ri.T]) <= set(int(n) for n in count[:64])
        assert (count[64:128] == (ri.T if arrangement == "full" else ri.T - 3)).all() and len(set(count[128:].tolist())) == 6
    count = ri.counts("short")
    for kind, (vs, ad, be, wide) in ri.KINDS.items():
        vals, x = ri.steered(kind, count)
        want = ri.expected(kind, vals, count, "short")
        bad = [c for c, w in enumerate(want) if w[0] != 0]
        assert bad == [ri.HONEST], (kind, bad)  # the honest error alone: inside the counts the walks are in range
        # a poisoned row inside the count breaks the channel: the rows beyond a count are not harmless
        c = 64
        seen = np.asarray(x[:, c]).astype(np.int64).astype(np.uint64) & np.uint64((1 << vs) - 1)
        assert ri.oracle_channel(seen, vs, ad)[0] == ri.INVALID, kind


# ---- the emulator ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", list(ri.KINDS))
@pytest.mark.parametrize("arrangement", ["full", "short"])
def test_emulated_counted_encode_is_the_oracle_on_each_channels_own_samples(sim, kind, arrangement):
    count = ri.counts(arrangement)
    vals, x = ri.steered(kind, count)
    out, bits, err = emulate(sim, kind, x, count)
    assert ri.mismatch(ri.expected(kind, vals, count, arrangement), out, bits, err) == ""


@pytest.mark.parametrize("kind", list(ri.KINDS))
def test_emulated_counted_encode_with_the_rings_run_full(sim, kind):
    count = ri.counts("short")
    vals, x = ri.steered(kind, count)
    sim.sim_ragged_int_set_drag(4, 20)  # waves 4 .. of the workgroup: coders and writers
    try:
        out, bits, err = emulate(sim, kind, x, count)
    finally:
        sim.sim_ragged_int_set_drag(1 << 30, 0)
    assert ri.mismatch(ri.expected(kind, vals, count, "short"), out, bits, err) == ""


@pytest.mark.parametrize("kind", list(ri.KINDS))
def test_emulated_counts_above_T(sim, kind):
    """such a channel: ERROR_INVALID_VALUE and 0 bits; its neighbours are what they were"""
    count = ri.counts("full")
    vals, x = ri.steered(kind, count)
    count[5], count[70], count[130] = ri.T + 1, 1 << 40, ri.T + 1
    out, bits, err = emulate(sim, kind, x, count)
    want = ri.expected(kind, vals, count)
    assert [w[0] for w in (want[5], want[70], want[130])] == [ri.INVALID] * 3
    assert ri.mismatch(want, out, bits, err, count, ri.T) == ""


@pytest.mark.parametrize("kind", list(ri.KINDS))
@pytest.mark.parametrize("cuts", [CUTS, CUTS + [ri.T]], ids=["cuts", "empty_last"])
def test_emulated_counted_segments_equal_the_single_launch(sim, kind, cuts):
    count = ri.counts("short")
    # counts inside, on and before a cut, in every wave
    for c, n in ((1, 8), (2, 9), (6, 64), (7, 63), (8, 65), (66, 200), (67, 1), (129, 9), (131, 201)):
        if c != ri.HONEST:
            count[c] = n
    count[133] = ri.T + 1  # above T_total: the same verdict in every launch
    vals, x = ri.steered(kind, count)
    single = emulate(sim, kind, x, count)
    want = ri.expected(kind, vals, count)
    assert ri.mismatch(want, *single, count, ri.T) == ""
    out, bits, err = emulate(sim, kind, x, count, cuts)
    assert ri.mismatch(want, out, bits, err, count, ri.T) == ""
    assert (bits == single[1]).all() and (err == single[2]).all()


# ---- C ABI and Python binding ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dca():
    mod = load_package()
    if not os.path.exists(mod.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return mod


def test_new_symbols_are_declared_and_exported(dca):
    with open(os.path.join(ROOT, "include", "dega_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(dega_hip_[a-z0-9_]+)\s*\(", header))
    lib = C.CDLL(dca.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in dca.exported_symbols(), name


def test_null_context_is_rejected(dca):
    L = dca.library()
    buf = (C.c_uint8 * 256)()
    p = C.cast(buf, C.c_void_p)
    job = dca.Job(1, 4, 1, 1, 32, dca.SAMPLES_I32, 100.0)
    E = dca.ERROR_INVALID_VALUE
    assert L.dega_hip_encode_var_dev(None, p, 1, 4, 1, p, 1, 32, dca.SAMPLES_I32, p, 64, p, p, None) == E
    assert L.dega_hip_encode64_var_dev(None, p, 1, 4, 1, p, 1, 40, p, 64, p, p, None) == E
    assert L.dega_hip_encode_segment_var_dev(None, p, 1, 4, 1, p, 0, 4, 1, 32, p, 64, p, p, p, 0, None) == E
    assert L.dega_hip_encode_var_job_host(None, C.byref(job), p, p, p, 64, p, p, p) == E
    assert L.dega_hip_group_encode_var(None, C.byref(job), p, p, p, 64, p, p, p) == E


def test_python_keywords_exist(dca):
    import inspect
    for cls, name in ((dca.Context, "encode"), (dca.Context, "encode_segments"), (dca.Context, "encode_job"), (dca.Group, "encode_job")):
        assert inspect.signature(getattr(cls, name)).parameters["count"].default is None, name


class _NoLibrary(object):
    """an encode_job whose every way into the library fails the test"""

    def _handle(self):
        raise AssertionError("the library was reached")

    _enc_fn = _enc_var_fn = _enc_agg_fn = _handle


@pytest.mark.parametrize("layout", ["time", "channel"])
def test_encode_job_count_assertions_need_no_library(dca, layout):
    x = np.zeros((6, 4), dtype=np.int32)
    n = 4 if layout == "time" else 6
    job = type("J", (_NoLibrary, dca._JobCalls), {})()
    good = np.zeros(n, dtype=np.uint64)
    with pytest.raises(AssertionError, match="uint64"):
        job.encode_job(x, count=good.astype(np.int64), layout=layout)
    with pytest.raises(AssertionError, match="uint64"):
        job.encode_job(x, count=[0] * n, layout=layout)
    with pytest.raises(AssertionError, match="one entry per channel"):
        job.encode_job(x, count=np.zeros(n + 1, dtype=np.uint64), layout=layout)
    with pytest.raises(AssertionError, match="num_values must be 1"):
        job.encode_job(x, count=good, num_values=2, layout=layout)
    with pytest.raises(AssertionError, match="dtype"):
        job.encode_job(x.astype(np.int64), count=good, layout=layout)
    with pytest.raises(AssertionError, match="the library was reached"):
        job.encode_job(x, count=good, layout=layout)
