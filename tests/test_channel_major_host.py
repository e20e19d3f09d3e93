"""Channel-major batches ([C][stride] <-> [T][ld]) without a GPU: the new symbols, keywords and flag of the surface, and
the LOGIC of dega_transpose_kernel -- the shipped kernel source (csrc/transpose_kernels.hpp) compiled by g++ under the
thread-per-lane emulator of tests/sim/ (tests/sim/sim_transpose.cpp) against numpy's transpose.  The parity tests proper
are tests/test_gpu_channel_major.py.

What the emulator does not cover of the 16-byte form: under DEGA_SIM a lane's 16-byte load / store is V element accesses
(tr_load / tr_store), so the alignment the real global_load_dwordx4 needs is checked by the launcher's conditions only
(sim_transpose refuses what the library would not choose), and the LDS bank behaviour is not modelled at all.  The lane to
element mapping, the edge handling of a vector that crosses the region's border and the counts are the shipped code.

Not tested here: the refusals of the entry points behind the null-context check need a live context and run in
tests/test_gpu_channel_major.py."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

from __graft_entry__ import load_package

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sim_build import sim_library  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dega_hip_to_time_major_dev", "dega_hip_to_channel_major_dev")
SHAPES = ((1, 1), (63, 65), (64, 64), (65, 63), (130, 257))  # (C, T)
DTYPES = {4: np.uint32, 8: np.uint64}
POISON = {4: 0xDEADBEEF, 8: 0xDEADBEEFCAFEF00D}
NAN = {4: 0x7FC00001, 8: 0x7FF8000000000001}  # quiet NaNs as float32 / float64 bits: what lies behind a count


@pytest.fixture(scope="module")
def dca():
    mod = load_package()
    if not os.path.exists(mod.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return mod


# ---- surface -------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_declared_and_exported(dca):
    with open(os.path.join(ROOT, "include", "dega_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(dega_hip_[a-z0-9_]+)\s*\(", header))
    lib = C.CDLL(dca.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in dca.exported_symbols(), name
    assert re.search(r"#define\s+DEGA_SAMPLES_CHANNEL_MAJOR\s+0x100\b", header)
    assert dca.SAMPLES_CHANNEL_MAJOR == 0x100
    top = header[: header.index("#ifndef DEGA_HIP_H")]
    assert "channel-major" in top  # the block comment states the contract


def test_null_context_is_rejected(dca):
    L = dca.library()
    buf = (C.c_uint8 * 256)()
    p = C.cast(buf, C.c_void_p)
    q = C.c_void_p(p.value + 128)
    assert L.dega_hip_to_time_major_dev(None, p, 2, 3, 3, 4, None, q, 2, None) == dca.ERROR_INVALID_VALUE
    assert L.dega_hip_to_channel_major_dev(None, p, 2, 3, 2, 4, None, q, 3, None) == dca.ERROR_INVALID_VALUE
    assert bytes(buf) == bytes(256)


def test_python_keywords_exist(dca):
    for cls in (dca.Context, dca.Group):
        for name in ("encode_job", "decode_job", "encode_job_levels"):
            assert inspect.signature(getattr(cls, name)).parameters["layout"].default == "time", (cls, name)
    sig = inspect.signature(dca.Context.to_time_major)
    assert list(sig.parameters)[1:] == ["x_ct", "T", "count", "ld", "out"]
    sig = inspect.signature(dca.Context.to_channel_major)
    assert list(sig.parameters)[1:] == ["x_tc", "channels", "count", "stride", "out"]


def test_layout_assertions_need_no_gpu(dca):
    """what the binding refuses before it calls the library: dtype, C-contiguity, shape, an unknown layout"""
    calls = dca._JobCalls()
    x = np.zeros((4, 6), dtype=np.int32)
    with pytest.raises(AssertionError):
        calls.encode_job(x.astype(np.int64), layout="channel")  # int32 samples need an int32 array: nothing is converted
    with pytest.raises(AssertionError):
        calls.encode_job(x.T, layout="channel")  # a transposed view is not C-contiguous
    with pytest.raises(AssertionError):
        calls.encode_job(x[0], layout="channel")
    with pytest.raises(AssertionError):
        calls.encode_job(x, layout="channel", T=7)  # more values than a row holds
    with pytest.raises(AssertionError):
        calls.encode_job(x, layout="columns")
    with pytest.raises(AssertionError):
        calls.encode_job_levels(x, [1, 4], layout="channel")  # float32 only
    with pytest.raises(AssertionError):
        calls.decode_job(np.zeros(1, np.uint8), np.zeros(5, np.uint64), np.zeros(4, np.uint64), 6, layout="channel", out=np.zeros((4, 5), np.int32))


# ---- kernel logic under the emulator ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sim():
    S = sim_library("transpose")
    Z, P = C.c_size_t, C.c_void_p
    S.sim_transpose.argtypes = [P, Z, Z, Z, Z, P, C.c_int, P, Z, C.c_int, C.c_int, Z]
    return S


def aligned(n, dtype, offset_elems=0):
    """n elements of dtype whose first lies offset_elems elements behind a 16-byte boundary"""
    esz = np.dtype(dtype).itemsize
    raw = np.zeros((n + offset_elems) * esz + 16, dtype=np.uint8)
    start = (-raw.ctypes.data) % 16 + offset_elems * esz
    return raw[start : start + n * esz].view(dtype)


def image(rows, used, pitch, dtype, fill, offset_elems=0):
    """[rows][pitch] filled with `fill`; the view of its logical [rows][used] part comes second"""
    flat = aligned(rows * pitch, dtype, offset_elems)
    flat[:] = fill
    full = flat.reshape(rows, pitch)
    return full, full[:, :used]


def run(S, to_time, src_full, Cn, T, esz, dst_full, count=None, wide=(0, 0), gx_max=2 ** 31 - 1):
    """to_time: src [C][stride] -> dst [T][ld]; else src [T][ld] -> dst [C][stride]"""
    R, K = (Cn, T) if to_time else (T, Cn)
    cp = None if count is None else count.ctypes.data
    return S.sim_transpose(src_full.ctypes.data, R, K, src_full.shape[1], esz, cp, 1 if to_time else 0, dst_full.ctypes.data, dst_full.shape[1],
                           wide[0], wide[1], gx_max)


def series(Cn, T, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(1, np.iinfo(dtype).max, size=(Cn, T), dtype=dtype)  # [C][T]; never 0, never the poison by construction of the check


SMALL = SHAPES[:4]
BIG = SHAPES[4]
FORMS = {"element": (0, 0), "wide": (1, 1)}


def odd_above(n):
    return n + 1 if n % 2 == 0 else n + 2


def counts_for(Cn, T, seed):
    rng = np.random.default_rng(seed)
    count = rng.integers(0, T + 6, size=Cn).astype(np.uint64)
    fixed = [0, T, T + 5, 1, max(T - 1, 0)]
    count[: min(Cn, len(fixed))] = fixed[:Cn]
    return count


def check(sim, to_time, esz, Cn, T, wide, pitch_case, with_count, gx_max=2 ** 31 - 1):
    """one launch against numpy.  pitch_case: 0 tight / padded, 1 padded / tight, with an element-wise side's padding odd and
    its base one element off 16 bytes; a 16-byte side's pitch is the next multiple of the vector (or one vector more).  The
    source holds NaN bits in its padding and behind every count, the destination poison that must survive in its padding."""
    dt, V = DTYPES[esz], 16 // esz
    x_ct = series(Cn, T, dt, Cn * 1000 + T + esz)
    rows_s, used_s = (Cn, T) if to_time else (T, Cn)
    up = lambda n, more: (n + V - 1) // V * V + (V if more else 0)  # noqa: E731
    ps = up(used_s, pitch_case == 1) if wide[0] else (used_s if pitch_case == 0 else odd_above(used_s))
    pd = up(rows_s, pitch_case == 0) if wide[1] else (rows_s if pitch_case == 1 else odd_above(rows_s))
    want_ct, given_ct, count = x_ct, x_ct, None
    if with_count:
        count = counts_for(Cn, T, Cn + T)
        live = np.arange(T)[None, :] < np.minimum(count, T)[:, None]  # [C][T]
        given_ct = np.where(live, x_ct, dt(NAN[esz]))
        want_ct = np.where(live, x_ct, dt(0))
    src_full, src = image(rows_s, used_s, ps, dt, NAN[esz], 0 if wide[0] else pitch_case)
    src[:] = given_ct if to_time else given_ct.T
    dst_full, dst = image(used_s, rows_s, pd, dt, POISON[esz], 0 if wide[1] else 1 - pitch_case)
    what = (to_time, esz, Cn, T, wide, pitch_case, with_count)
    assert run(sim, to_time, src_full, Cn, T, esz, dst_full, count=count, wide=wide, gx_max=gx_max) == 0, what
    assert (dst == (want_ct.T if to_time else want_ct)).all(), what
    assert (dst_full[:, rows_s:] == POISON[esz]).all(), what


# The emulator starts an OS thread per lane, 256 per tile, so every launch here is chosen: the four small shapes (six tiles)
# carry the cross product of direction, element size, form and counts, with the pitch cases alternating from shape to shape;
# the 15-tile shape carries the same cross product, its tile index split over x and y.
@pytest.mark.parametrize("with_count", (False, True))
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("esz", (4, 8))
@pytest.mark.parametrize("to_time", (True, False))
def test_small_shapes(sim, to_time, esz, form, with_count):
    for n, (Cn, T) in enumerate(SMALL):
        check(sim, to_time, esz, Cn, T, FORMS[form], (n + esz // 8 + int(with_count)) % 2, with_count)


@pytest.mark.parametrize("with_count", (False, True))
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("esz", (4, 8))
@pytest.mark.parametrize("to_time", (True, False))
def test_several_tiles_numbered_over_x_and_y(sim, to_time, esz, form, with_count):
    """(130, 257): the one shape here with tiles INSIDE the region (the path without tests) beside edge tiles, 15 tiles over a
    grid of 4 x 4 -- the flat index blockIdx.y * gridDim.x + blockIdx.x, the spare workgroup idle.  Both forms, with and
    without counts, for both directions and element sizes; the pitch case alternates."""
    check(sim, to_time, esz, BIG[0], BIG[1], FORMS[form], (esz // 8 + int(with_count) + int(to_time)) % 2, with_count, gx_max=4)


@pytest.mark.parametrize("esz", (4, 8))
def test_one_side_wide_the_other_by_elements(sim, esz):
    """the two mixed instantiations the launcher can choose, on extents that are no multiple of the vector"""
    for to_time in (True, False):
        for wide in ((1, 0), (0, 1)):
            check(sim, to_time, esz, 65, 63, wide, int(to_time), wide[0] == 1)


def test_launcher_conditions_of_the_wide_form(sim):
    """a base off 16 bytes or a pitch off the vector is not given to the 16-byte form"""
    src_full, _ = image(8, 8, 8, np.uint32, 1, 1)
    dst_full, _ = image(8, 8, 8, np.uint32, 2)
    assert run(sim, True, src_full, 8, 8, 4, dst_full, wide=(1, 0)) == -1
    src_full, _ = image(8, 8, 9, np.uint32, 1)
    assert run(sim, True, src_full, 8, 8, 4, dst_full, wide=(1, 0)) == -1
    dst_full, _ = image(8, 8, 10, np.uint32, 2)
    src_full, _ = image(8, 8, 8, np.uint32, 1)
    assert run(sim, True, src_full, 8, 8, 4, dst_full, wide=(0, 1)) == -1
    assert (dst_full == 2).all()
