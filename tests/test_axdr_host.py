"""A-XDR without a GPU: the surface of the new entry points, and the LOGIC of dega_axdr_pack_kernel / dega_axdr_unpack_kernel --
the shipped kernel source and launch code (csrc/axdr_kernels.hpp) compiled by g++ under the thread-per-lane emulator of
tests/sim/ (tests/sim/sim_axdr.cpp) -- against the oracle's `normalize` stage and a plain numpy pack that is held to it here.
The cases are those of tests/axdr_common.py; tests/test_gpu_axdr.py runs their whole product through the C ABI.

The emulator starts an OS thread per lane, 256 per tile, so every launch here is chosen: a Latin selection of (value size,
rows, channels) that still holds every value size, every T and every C of the lists.  Under DEGA_SIM a 16-byte access is V
element accesses, so the alignment the real instruction needs is checked by the launcher's conditions only, and the LDS bank
behaviour is not modelled at all.

Not tested here: the refusals behind the null-context check need a live context and run in tests/test_gpu_axdr.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from __graft_entry__ import load_package

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import axdr_common as ax  # noqa: E402
import float_edges_common as fe  # noqa: E402
from oracle import orc  # noqa: E402
from sim_build import SIM_DIR, sim_library  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dega_hip_axdr_bytes", "dega_hip_axdr_encode_dev", "dega_hip_axdr_decode_dev", "dega_hip_axdr_encode_levels_f32_dev",
               "dega_hip_axdr_encode_host", "dega_hip_axdr_decode_host")
P, Z, I, F = C.c_void_p, C.c_size_t, C.c_int, C.c_float


class Handle:
    def __init__(self, raw, view, initial):
        self.raw, self.view, self.initial = raw, view, initial


class Emulator:
    """the backend of axdr_common over tests/sim/libaxdr_sim.so: numpy arrays"""

    def __init__(self):
        self.L = sim_library("axdr")
        self.L.sim_axdr_pack.argtypes = [P, I, Z, Z, Z, P, F, I, P, Z, P, P, I, Z]
        self.L.sim_axdr_unpack.argtypes = [P, Z, P, Z, Z, Z, F, I, I, P, P, P, I, Z]

    @staticmethod
    def buf(array, offset=0):
        data = np.ascontiguousarray(array).reshape(-1).view(np.uint8)
        raw = np.zeros(data.size + 48, dtype=np.uint8)
        start = (-raw.ctypes.data) % 16 + offset
        view = raw[start:start + data.size]
        view[:] = data
        return Handle(raw, view, data.tobytes())

    @staticmethod
    def ptr(h):
        return h.view.ctypes.data

    @staticmethod
    def get(h):
        return h.view.copy()

    @staticmethod
    def initial(h):
        return h.initial

    def pack(self, x, kind, Cn, T, ld, count, factor, vs, out, cap, bits, err, wide, gx_max):
        return self.L.sim_axdr_pack(x, kind, Cn, T, ld, count or None, factor, vs, out, cap, bits, err, wide, gx_max)

    def unpack(self, s, cap, bits, Cn, max_T, ld, factor, vs, kind, x, count, err, wide, gx_max):
        return self.L.sim_axdr_unpack(s, cap, bits, Cn, max_T, ld, factor, vs, kind, x, count, err, wide, gx_max)


@pytest.fixture(scope="module")
def B():
    return Emulator()


@pytest.fixture(scope="module")
def dca():
    mod = load_package()
    if not os.path.exists(mod.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return mod


def latin(i, per=3):
    """the (T, C) pairs of value size number i: every T and every C of the lists is met over the 15 value sizes"""
    return [(ax.ROWS[(i + 5 * m) % len(ax.ROWS)], ax.CHANNELS[(i + m) % len(ax.CHANNELS)]) for m in range(per)]


def test_the_selection_holds_every_size():
    pairs = [p for i in range(len(ax.SIZES)) for p in latin(i)]
    assert {t for t, _ in pairs} == set(ax.ROWS) and {c for _, c in pairs} == set(ax.CHANNELS)
    assert {0, 1, 31, 32, 33, ax.R - 1, ax.R, ax.R + 1, 2 * ax.R + 44} <= set(ax.ROWS)
    assert {ax.R_WIDE - 1, ax.R_WIDE, ax.R_WIDE + 1, 2 * ax.R_WIDE + 44} <= set(ax.ROWS)


# ---- surface -------------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_declared_and_exported(dca):
    with open(os.path.join(ROOT, "include", "dega_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(dega_hip_[a-z0-9_]+)\s*\(", header))
    lib = C.CDLL(dca.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in dca.exported_symbols(), name
    for name in ("axdr_encode", "axdr_decode", "axdr_encode_levels_f32", "axdr_encode_host", "axdr_decode_host"):
        assert callable(getattr(dca.Context, name)), name


def test_axdr_bytes(dca):
    L = dca.library()
    for T, vs in ((0, 8), (1, 1), (1, 32), (1, 33), (31, 3), (32, 3), (300, 47), (86400, 24)):
        assert L.dega_hip_axdr_bytes(T, vs) == ax.axdr_bytes(T, vs) == dca.axdr_bytes(T, vs), (T, vs)
    assert L.dega_hip_axdr_bytes(5, 0) == 0 and L.dega_hip_axdr_bytes(5, 65) == 0 and L.dega_hip_axdr_bytes(5, -1) == 0
    # the overflow edge: T * vs + 31 has to fit 64 bits
    assert L.dega_hip_axdr_bytes((1 << 58) - 1, 64) == (1 << 61) - 8
    assert L.dega_hip_axdr_bytes(1 << 58, 64) == 0
    assert L.dega_hip_axdr_bytes((1 << 64) - 32, 1) == (1 << 61) - 4
    assert L.dega_hip_axdr_bytes((1 << 64) - 31, 1) == 0


def test_null_context_is_rejected(dca):
    """every entry refuses a null context (and whatever else is wrong with the call) without touching a device or an array"""
    L = dca.library()
    mem = (C.c_uint8 * 1024)()
    a = C.cast(mem, C.c_void_p).value
    x, out, bits, err, cnt = a, a + 256, a + 512, a + 640, a + 768
    S = dca
    calls = [
        lambda vs=8, samples=S.SAMPLES_F32, ld=4, cap=8, xx=x, oo=out: L.dega_hip_axdr_encode_dev(None, xx, samples, 4, 3, ld, None, 100.0, vs, oo, cap, bits, err, None),
        lambda vs=8, samples=S.SAMPLES_F32, ld=4, cap=8, xx=x, oo=out: L.dega_hip_axdr_decode_dev(None, oo, cap, bits, 4, 3, ld, 100.0, vs, samples, xx, cnt, err, None),
        lambda vs=8, samples=S.SAMPLES_F32, ld=4, cap=8, xx=x, oo=out: L.dega_hip_axdr_encode_host(None, xx, samples, 4, 3, ld, None, 100.0, vs, oo, cap, bits, err),
        lambda vs=8, samples=S.SAMPLES_F32, ld=4, cap=8, xx=x, oo=out: L.dega_hip_axdr_decode_host(None, oo, cap, bits, 4, 3, ld, 100.0, vs, samples, xx, cnt, err),
    ]
    for call in calls:
        assert call() == dca.ERROR_INVALID_VALUE
        for kw in (dict(vs=0), dict(vs=65), dict(vs=33, samples=S.SAMPLES_I32), dict(samples=S.SAMPLES_BE32), dict(samples=S.SAMPLES_F32 | S.SAMPLES_CHANNEL_MAJOR),
                   dict(ld=3), dict(cap=6), dict(xx=None), dict(oo=None)):
            assert call(**kw) == dca.ERROR_INVALID_VALUE, kw
    one = (Z * 1)(4)
    ptrs = (P * 1)(out)
    caps = (Z * 1)(8)
    assert L.dega_hip_axdr_encode_levels_f32_dev(None, x, 4, 3, 4, None, one, 1, 100.0, 8, ptrs, caps, ptrs, None, ptrs, None) == dca.ERROR_INVALID_VALUE
    assert bytes(mem) == bytes(1024)


def test_binding_assertions_need_no_gpu(dca):
    """what the binding refuses before it calls the library: dtype, contiguity, shape (as encode_segments has them)"""
    ctx = dca.Context.__new__(dca.Context)  # (no device behind it: the assertions come first)
    ctx._h = None
    x = np.zeros((4, 6), dtype=np.float32)
    with pytest.raises(AssertionError):
        ctx.axdr_encode_host(x.astype(np.float64), 8)
    with pytest.raises(AssertionError):
        ctx.axdr_encode_host(x.T, 8)
    with pytest.raises(AssertionError):
        ctx.axdr_encode_host(x[0], 8)
    with pytest.raises(AssertionError):
        ctx.axdr_encode_host(x, 8, channels=7)
    with pytest.raises(AssertionError):
        ctx.axdr_encode_host(x.view(np.int32), 40, samples=dca.SAMPLES_I64)  # int64 samples need an int64 array
    with pytest.raises(AssertionError):
        ctx.axdr_decode_host(np.zeros((4, 6), dtype=np.int8), np.zeros(4, np.uint64), 3, 8)
    with pytest.raises(AssertionError):
        ctx.axdr_decode_host(np.zeros((4, 8), dtype=np.uint8), np.zeros(3, np.uint64), 3, 8)  # one bit length per channel


# ---- the plain pack is the oracle's, and the oracle the reference's ------------------------------------------------------------

@pytest.mark.parametrize("vs", (1, 2, 3, 7, 8, 12, 16, 17, 24))
def test_plain_pack_is_the_oracles(vs):
    """on fields that floats reach exactly with factor 1: the integers k of the value size with k +- 0.5 inside normalize.c:21's
    range (the two ends of the range are reached from no float: their halves lie outside it)"""
    T = 67
    half = 1 << (vs - 1)
    for c in range(4):
        signed = np.clip(fe.sign_extend(ax.fields(vs, T, 4)[:, c], vs), 1 - half, max(half - 2, 1 - half))
        col = signed.view(np.uint64) & ax.mask(vs)
        v = signed.astype(np.float32)
        assert (v.astype(np.int64) == signed).all()
        r, data, n = ax.oracle_pack(fe.as_bits(v), vs, 1.0)
        assert (r, data, n) == (0,) + ax.pack_channel(col, vs), (vs, c)
        assert (ax.unpack_channel(data, n, vs) == col).all()
        assert (ax.unpack_channel(data, n, vs) == fe.unpack_fields(data, n, vs)).all() and fe.pack_fields(col.tolist(), vs)[0] == data[: (n + 7) // 8]
        r, back = ax.oracle_unpack(data, n, vs, 1.0)
        assert r == 0 and (back == fe.as_bits(v)).all()


def test_stumps_as_the_oracle_answers_them():
    data, n = ax.pack_channel(np.arange(1, 5, dtype=np.uint64), 12)
    assert [orc.stage("normalize", False, data, b, valuesize=12)[0] for b in (40, 35, 36, 48)] == [-11, -11, 0, 0]
    data, n = ax.pack_channel(np.arange(1, 7, dtype=np.uint64), 3)
    got = [orc.stage("normalize", False, data, b, valuesize=3) for b in (9, 12, 10, 11, 16)]
    assert [g[0] for g in got] == [0, 0, -11, -11, -11] and [g[2] // 32 for g in got[:2]] == [3, 4]


def test_fixture_holds_the_oracle():
    """tests/golden/axdr.npz: what the compiled reference's `encode normalize` wrote, stream and bits, and its `decode
    normalize` of that -- the oracle's stage and the plain pack give the same"""
    z = np.load(ax.GOLDEN)
    for vs in ax.GOLDEN_SIZES:
        v = ax.golden_input(vs)
        assert fe.crc(v) == z["n%d.in" % vs], "the corpus is not the one the fixture was made from"
        for c in range(ax.GOLDEN_CHANNELS):
            ref, nbits = z["n%d.c%d.stream" % (vs, c)].tobytes(), int(z["n%d.c%d.bits" % (vs, c)].ravel()[0])
            r, data, n = ax.oracle_pack(v[:, c], vs, 100.0)
            assert r == 0 and n == nbits == ax.GOLDEN_ROWS * vs and data[: (n + 7) // 8] == ref, (vs, c)
            _, fields = fe.normalize(v[:, c], 100.0, vs)
            assert ax.pack_channel(fields, vs)[0][: (n + 7) // 8] == ref, (vs, c)
            r, back = ax.oracle_unpack(ref, nbits, vs, 100.0)
            assert r == 0 and fe.same_float_bits(back, z["n%d.c%d.back" % (vs, c)]).all(), (vs, c)


# ---- kernel logic under the emulator -------------------------------------------------------------------------------------------

def test_tile_rows(B):
    assert B.L.sim_axdr_rows(0) == ax.R and B.L.sim_axdr_rows(1) == ax.R_WIDE


@pytest.mark.parametrize("i", range(len(ax.SIZES)), ids=lambda i: "vs%d" % ax.SIZES[i])
def test_pack_integers(B, i):
    """the integer entries over the full range of the value size, junk above the fields; both load forms, both pitch cases"""
    vs = ax.SIZES[i]
    for m, (T, Cn) in enumerate(latin(i)):
        ax.case_pack_int(B, vs, Cn, T, pitch_case=(i + m) % 2, wide=0)
        if T and Cn % (2 if vs > 32 else 4) == 0:
            ax.case_pack_int(B, vs, Cn, T, pitch_case=0, wide=1)
    ax.case_pack_int(B, vs, 65, ax.R + 1, pitch_case=1, wide=0)


@pytest.mark.parametrize("wide", (0, 1))
@pytest.mark.parametrize("vs", (32, 12, 40))
def test_several_tiles_numbered_over_x_and_y(B, vs, wide):
    """tiles inside the region (the path without tests) beside edge tiles, the flat index split over x and y, a spare workgroup idle"""
    ax.case_pack_int(B, vs, 132, 300, wide=wide, gx_max=4)
    ax.case_unpack(B, vs, 132, 300, ax.kind_of(vs), wide=wide, gx_max=4)


@pytest.mark.parametrize("factor", ax.FACTORS)
@pytest.mark.parametrize("vs", (8, 17, 32, 47, 64))
def test_pack_floats(B, vs, factor):
    """the float entry against the oracle's stage: bounds and neighbours, ties, NaNs, subnormals"""
    i = ax.SIZES.index(vs) + ax.FACTORS.index(factor)
    T, Cn = latin(i)[0]
    ax.case_pack_float(B, vs, factor, Cn, max(T, 1), pitch_case=i % 2, wide=0)
    ax.case_pack_float(B, vs, factor, 64, 129, wide=1)


@pytest.mark.parametrize("vs", (12, 32, 63))
def test_refusals(B, vs):
    ax.case_refusals(B, vs, 100.0)


@pytest.mark.parametrize("floats", (False, True))
@pytest.mark.parametrize("vs,T", ((3, 33), (12, 129), (32, 300), (33, 65), (64, 172)))
def test_counts(B, vs, T, floats):
    if floats and vs < 4:
        vs = 7
    ax.case_counts(B, vs, 65, T, floats)
    ax.case_counts(B, vs, 64, T, floats, short_cap=True, wide=1)


@pytest.mark.parametrize("i", range(len(ax.SIZES)), ids=lambda i: "vs%d" % ax.SIZES[i])
def test_unpack_integers(B, i):
    vs = ax.SIZES[i]
    for m, (T, Cn) in enumerate(latin(i)):
        ax.case_unpack(B, vs, Cn, T, ax.kind_of(vs), pitch_case=(i + m) % 2, wide=0)
        if Cn % (2 if vs > 32 else 4) == 0:
            ax.case_unpack(B, vs, Cn, T, ax.kind_of(vs), wide=1)
    ax.case_unpack(B, vs, 65, 131, ax.kind_of(vs), how="file")
    ax.case_unpack(B, vs, 5, 40, ax.kind_of(vs), how="zero")
    ax.case_unpack(B, vs, 7, 33, ax.kind_of(vs), how="short")


@pytest.mark.parametrize("factor", ax.FACTORS)
@pytest.mark.parametrize("vs", (3, 12, 17, 32, 47, 64))
def test_unpack_floats(B, vs, factor):
    i = ax.SIZES.index(vs) + ax.FACTORS.index(factor)
    T, Cn = latin(i)[1]
    ax.case_unpack(B, vs, Cn, T, ax.F32, factor, pitch_case=i % 2, wide=0)
    ax.case_unpack(B, vs, 64, 70, ax.F32, factor, how="file", wide=1)
    ax.case_unpack(B, vs, 6, 34, ax.F32, factor, how="short")


@pytest.mark.parametrize("vs", (3, 12, 32, 33, 64))
def test_unpack_cuts(B, vs):
    ax.case_unpack_cuts(B, vs, ax.kind_of(vs))
    ax.case_unpack_cuts(B, vs, ax.F32, 3.3)


@pytest.mark.parametrize("vs,factor", ((8, 100.0), (24, 1.0), (32, 3.3), (40, -100.0)))
def test_round_trip(B, vs, factor):
    ax.case_round_trip(B, vs, factor, 65, 130)


def test_launcher_conditions(B):
    """a base off 16 bytes or a pitch off the vector is not given the 16-byte form; kinds and value sizes that do not go together"""
    x = B.buf(np.zeros(64, dtype=np.uint32), 4)
    out, bits, err = B.buf(np.zeros(64, np.uint8)), B.buf(np.zeros(8, np.uint64)), B.buf(np.zeros(8, np.int32))
    assert B.pack(B.ptr(x), ax.I32, 4, 4, 4, 0, 1.0, 8, B.ptr(out), 4, B.ptr(bits), B.ptr(err), 1, 4) == -1
    x = B.buf(np.zeros(64, dtype=np.uint32))
    assert B.pack(B.ptr(x), ax.I32, 4, 4, 5, 0, 1.0, 8, B.ptr(out), 4, B.ptr(bits), B.ptr(err), 1, 4) == -1
    assert B.pack(B.ptr(x), ax.I32, 4, 4, 4, 0, 1.0, 33, B.ptr(out), 4, B.ptr(bits), B.ptr(err), 0, 4) == -1
    assert B.pack(B.ptr(x), ax.I64, 4, 4, 4, 0, 1.0, 32, B.ptr(out), 4, B.ptr(bits), B.ptr(err), 0, 4) == -1
    assert (B.get(out) == 0).all()


# ---- index width -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def V():
    import index_width_common as iw
    from test_index_width_host import Emulator as Images

    class Sparse(Images):
        def __init__(self):  # (the images alone: none of the other emulator libraries)
            self.lib, self.kept = {}, []
            self.images = {name: np.empty(size, dtype=np.uint8) for name, size in iw.IMAGES.items() if name in ("BIG", "MID", "TEXT")}

    v = Sparse()
    yield v
    v.close()


@pytest.mark.parametrize("what", ("ld", "cap"))
def test_offsets_are_64_bit_under_the_emulator(B, V, what):
    """ld = 2^26 at T = 70 and cap = 2^29 at C = 12: sparse images, only the logical regions touched"""
    try:
        ax.case_index_width(B, V, what)
    finally:
        V.forget()


# ---- the stand-alone program under the host sanitizers ---------------------------------------------------------------------------

SAN_FLAGS = ["-std=c++20", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
             "-static-libubsan", "-pthread", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unknown-pragmas"]


def test_fixed_selection_under_the_sanitizers(tmp_path):
    """tests/sim/sim_axdr_main.cpp: the emulated kernels on a fixed selection, built with -fsanitize=address,undefined as a
    program of its own (never loaded into Python)"""
    # the one excuse is a toolchain that cannot link the sanitizers' runtimes: probed with a trivial program; anything else
    # that keeps the real one from building is a failure
    probe = subprocess.run(["make", "-s", "-C", SIM_DIR, "sanitizer_probe"], capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the toolchain here cannot link -fsanitize=address,undefined: " + probe.stderr.strip()[-300:])
    exe = str(tmp_path / "sim_axdr_asan")
    r = subprocess.run(["g++"] + SAN_FLAGS + [os.path.join(SIM_DIR, "sim_axdr_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "axdr: ok", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
