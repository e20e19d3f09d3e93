"""Ragged batches (a count per channel through aggregate, the DEGA float entry, `encode csv` and the LZMH chain), without a
GPU: the new symbols of the C ABI, and the counted kernels' LOGIC -- the shipped kernel sources compiled by g++ under the
thread-per-lane emulator of tests/sim/ (tests/sim/sim_ragged.cpp) against the whole of tests/golden/ragged.npz, the
compiled reference's results per channel on that channel's own readings.  Every row at or beyond a channel's count holds
poison (NaN, +inf, 3e38, -0.0) in everything a kernel is given here.  The parity tests proper are tests/test_gpu_ragged.py.

Not tested here: the refusals that need a live context (a null or misaligned count and the like) are host code behind the
null-context check and run in tests/test_gpu_ragged.py.  Not tested anywhere: a count together with a segment state.  The
library's launcher refuses the pair, but no entry point of the C ABI can express it (there is no counted
dega_hip_encode_segment_dev), so no test can reach that line."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from __graft_entry__ import load_package

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from agg_common import same_floats, sequential  # noqa: E402
from ragged_common import (CASES, FACTOR, HONEST, LEVELS, POISON, SETS, Fixture, poisoned, same_rows, same_streams, same_texts,  # noqa: E402
                           untouched)
from sim_build import sim_library  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dega_hip_aggregate_levels_var_dev", "dega_hip_encode_f32_var_dev", "dega_hip_encode_levels_f32_var_dev", "dega_hip_csv_write_var_dev",
               "dega_hip_lzmh_encode_levels_f32_var_dev")
SENTINEL = np.float32(-12345.0)
INVALID = -1


@pytest.fixture(scope="module")
def dca():
    mod = load_package()
    if not os.path.exists(mod.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return mod


@pytest.fixture(scope="module")
def fx():
    return Fixture()


# ---- C ABI ---------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_declared_and_exported(dca):
    with open(os.path.join(ROOT, "include", "dega_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(dega_hip_[a-z0-9_]+)\s*\(", header))
    lib = C.CDLL(dca.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in dca.exported_symbols(), name
    top = header[: header.index("#ifndef DEGA_HIP_H")]
    assert "_var_dev" in top  # the block comment lists what each entry replaces


def test_null_context_is_rejected(dca):
    L = dca.library()
    buf = (C.c_uint8 * 256)()
    p = C.cast(buf, C.c_void_p)
    nv = (C.c_size_t * 2)(2, 4)
    two = (C.c_void_p * 2)(p, p)
    sizes = (C.c_size_t * 2)(64, 64)
    E = dca.ERROR_INVALID_VALUE
    assert L.dega_hip_aggregate_levels_var_dev(None, p, 1, 4, 1, p, nv, 2, two, sizes, two, p, None) == E
    assert L.dega_hip_encode_f32_var_dev(None, p, 1, 4, 1, p, 100.0, 1, 32, p, 64, p, p, None) == E
    assert L.dega_hip_encode_levels_f32_var_dev(None, p, 1, 4, 1, p, nv, 2, 100.0, 1, 32, two, sizes, two, two, two, None) == E
    assert L.dega_hip_csv_write_var_dev(None, p, 1, 4, 1, p, 2, 1, 44, p, 64, p, p, None) == E
    assert L.dega_hip_lzmh_encode_levels_f32_var_dev(None, p, 1, 4, 1, p, nv, 2, 2, 1, 44, sizes, two, sizes, two, two, two, two, None) == E


def test_python_keywords_exist(dca):
    import inspect
    for name in ("aggregate_levels", "aggregate", "encode_f32", "encode_f32_levels", "csv_write", "lzmh_encode_levels_f32"):
        assert inspect.signature(getattr(dca.Context, name)).parameters["count"].default is None, name


# ---- the fixture is not blind ------------------------------------------------------------------------------------------------

def test_fixture_equals_the_restatement_on_each_channels_own_readings(fx):
    for case in CASES:
        v, count = fx.v(case), fx.count(case)
        for N in LEVELS:
            rows = fx.rows(case, N)
            assert (rows == -(-count // N)).all()
            for c in range(v.shape[1]):
                own = v[: int(count[c]), c].reshape(-1, 1)
                assert same_floats(sequential(own, N)[:, 0], fx.sums(case, N)[: int(rows[c]), c]), (case, N, c)


def test_fixture_tells_cheats_apart(fx):
    """ignoring the counts (poison and all) differs on every ragged channel; padding with zeros gives more rows -- other
    counts, other texts -- on every ragged channel and every level the padding adds a group to"""
    for case in CASES:
        v, count = fx.v(case), fx.count(case)
        T = v.shape[0]
        ragged = [c for c in range(v.shape[1]) if count[c] < T]
        assert len(ragged) >= 60
        for c in ragged:
            assert np.isnan(v[int(count[c]), c])  # the first dead row
            for N in LEVELS:
                whole = sequential(v[:, c : c + 1], N)[:, 0]
                assert not same_floats(whole, fx.sums(case, N)[:, c]), (case, N, c)
        zeroed = v.copy()
        for c in range(v.shape[1]):
            zeroed[int(count[c]):, c] = 0.0
        for N in LEVELS:
            padded_rows = -(-T // N)
            assert sum(int(fx.rows(case, N)[c]) != padded_rows for c in ragged) >= 1, (case, N)
            text, text_len = fx.text(case, N)
            assert sum(int(text_len[c]) != sum(len("%.2f\n" % x) for x in sequential(zeroed[:, c : c + 1], N)[:, 0]) for c in ragged) >= 1


def test_fixture_shape_and_the_one_honest_error(fx):
    assert fx.v("long").shape == (200, 136) and fx.v("short").shape == (96, 70)
    count = fx.count("long")
    assert [int(n) for n in count[:14]] == [0, 1, 6, 7, 8, 59, 60, 61, 63, 64, 65, 127, 199, 200]
    assert (count[64:128] == 200).all() and count[128:].max() <= 50
    for case in CASES:
        assert fx.v(case)[10, HONEST] == 400.0 and fx.count(case)[HONEST] > 10
        for N in LEVELS:
            for vs, ad in SETS:
                err = fx.dega(case, N, vs, ad)[2]
                assert [c for c in range(err.size) if err[c] != 0] == ([HONEST] if vs == 16 else []), (case, N, vs, ad)
                if ad:
                    out, bits, _ = fx.dega(case, N, vs, ad)
                    for c in np.flatnonzero(fx.count(case) == 0):
                        assert int(bits[c]) == 3 and out[c, 0] == 0x20  # the reference on an empty input
    golden = os.path.join(ROOT, "tests", "golden")
    assert os.path.getsize(fx.path) <= max(os.path.getsize(os.path.join(golden, f)) for f in os.listdir(golden) if f != "ragged.npz")


# ---- kernel logic under the emulator ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sim():
    S = sim_library("ragged")
    Z, P = C.c_size_t, C.c_void_p
    S.sim_aggregate_var.argtypes = [P, Z, Z, Z, P, P, Z, P, P, P, P, C.c_int, Z]
    S.sim_csv_var.argtypes = [P, Z, Z, Z, P, C.c_uint, Z, C.c_int, P, Z, P, P, C.c_int]
    S.sim_encode_f32_var.argtypes = [P, Z, Z, Z, P, C.c_float, C.c_int, C.c_int, P, Z, P, P]
    S.sim_ragged_set_drag.argtypes = [C.c_int, C.c_int]
    return S


def sim_aggregate(S, v, count, levels, step, Cn=None, ld_out=None, wide=0):
    v = np.ascontiguousarray(v, dtype=np.float32)
    count = np.ascontiguousarray(count, dtype=np.uint64)
    T, ld = v.shape
    Cn = ld if Cn is None else Cn
    K = len(levels)
    ld_out = [Cn] * K if ld_out is None else ld_out
    outs = [np.full((max(1, -(-T // N)), ld_out[k]), SENTINEL, dtype=np.float32) for k, N in enumerate(levels)]
    counts = [np.full(Cn, 99999, dtype=np.uint64) for _ in levels]
    err = np.full(Cn, 77, dtype=np.int32)
    ret = S.sim_aggregate_var(v.ctypes.data, Cn, T, ld, count.ctypes.data, (C.c_size_t * K)(*levels), K, (C.c_void_p * K)(*[o.ctypes.data for o in outs]),
                              (C.c_size_t * K)(*ld_out), (C.c_void_p * K)(*[o.ctypes.data for o in counts]), err.ctypes.data, wide, step)
    assert ret == 0, (levels, step)
    return outs, counts, err


def check_aggregate(fx, case, got, levels, count=None, bad=()):
    outs, counts, err = got
    for k, N in enumerate(levels):
        rows = fx.rows(case, N).copy()
        rows[list(bad)] = 0
        assert (counts[k].astype(np.int64) == rows).all(), (case, N)
        assert same_rows(outs[k], fx.sums(case, N), rows), (case, N)
        assert untouched(outs[k], rows, SENTINEL), (case, N)  # a group without a reading is not stored, nothing is stored for a bad channel
        assert (outs[k][:, len(rows):] == SENTINEL).all(), (case, N)
    want_err = np.zeros(err.size, dtype=np.int32)
    want_err[list(bad)] = INVALID
    assert (err == want_err).all(), case


def test_counted_aggregate_one_level(sim, fx):
    """K = 1, both forms where C allows, ranges that cut the series and one range for all of it"""
    for case in CASES:
        v, count = fx.v(case), fx.count(case)
        T = v.shape[0]
        for N in LEVELS:
            for wide in ((0, 1) if v.shape[1] % 4 == 0 else (0,)):
                for step in sorted({N * max(1, 16 // N), N * max(1, 33 // N), 2 * N * max(1, 33 // N), T, T + 5}):
                    check_aggregate(fx, case, sim_aggregate(sim, v, count, [N], step, wide=wide), [N])


def test_counted_aggregate_three_levels_and_two(sim, fx):
    for case in CASES:
        v, count = fx.v(case), fx.count(case)
        T = v.shape[0]
        for wide in ((0, 1) if v.shape[1] % 4 == 0 else (0,)):
            for step in (T, T + 5):  # (the least common multiple of 1, 7 and 60 is above T: one range)
                check_aggregate(fx, case, sim_aggregate(sim, v, count, [60, 1, 7], step, wide=wide), [60, 1, 7])
            for step in (7, 28, 63, T):
                check_aggregate(fx, case, sim_aggregate(sim, v, count, [7, 1], step, wide=wide), [7, 1])


def test_counted_aggregate_pitches(sim, fx):
    """dword-form pitches with ld > C, a pitch of its own per level: columns beyond C are neither read into a result nor written"""
    for case in CASES:
        v, count = fx.v(case), fx.count(case)
        T, Cn = v.shape
        wide_in = np.full((T, Cn + 9), np.float32(np.inf), dtype=np.float32)
        wide_in[:, :Cn] = v
        check_aggregate(fx, case, sim_aggregate(sim, wide_in, count, [60, 1, 7], T, Cn=Cn, ld_out=[Cn + 3, Cn, Cn + 20]), [60, 1, 7])
        check_aggregate(fx, case, sim_aggregate(sim, wide_in, count, [7], 14, Cn=Cn, ld_out=[Cn + 1]), [7])


def test_counted_aggregate_count_above_T(sim, fx):
    """count[c] > T: that channel gets the error, counts of 0 and no row; its neighbours are right"""
    v, count = fx.v("long"), fx.count("long").astype(np.uint64)
    bad = (3, 70, 131)
    count[list(bad)] = [201, 2 ** 40, 2 ** 63]
    for wide in (0, 1):
        check_aggregate(fx, "long", sim_aggregate(sim, v, count, [60, 1, 7], 200, wide=wide), [60, 1, 7], bad=bad)
        check_aggregate(fx, "long", sim_aggregate(sim, v, count, [7], 21, wide=wide), [7], bad=bad)


def test_counted_aggregate_of_no_rows(sim):
    """T = 0: nothing is read, counts of 0; a count above 0 is above T"""
    outs, counts, err = sim_aggregate(sim, np.zeros((0, 8), dtype=np.float32), np.array([0, 0, 1, 0, 0, 0, 0, 5]), [4, 1], 1)
    assert all((c == 0).all() for c in counts) and [int(e) for e in err] == [0, 0, INVALID, 0, 0, 0, 0, INVALID]
    assert all((o == SENTINEL).all() for o in outs)


def sim_csv(S, v, count, Cn=None, stride=None, wide=0, decimals=2):
    v = np.ascontiguousarray(v, dtype=np.float32)
    count = np.ascontiguousarray(count, dtype=np.uint64)
    T, ld = v.shape
    Cn = ld if Cn is None else Cn
    stride = stride if stride is not None else (T * 12 + 16 + 15) // 16 * 16
    raw = np.full(Cn * stride + 16, 0xEE, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16
    out = raw[off : off + Cn * stride].reshape(Cn, stride)
    lens = np.full(Cn, 99999, dtype=np.uint64)
    err = np.full(Cn, 77, dtype=np.int32)
    assert S.sim_csv_var(v.ctypes.data, Cn, T, ld, count.ctypes.data, decimals, 1, 44, out.ctypes.data, stride, lens.ctypes.data, err.ctypes.data, wide) == 0
    return out, lens, err


def test_counted_csv_writer(sim, fx):
    """every level's text from that level's sums and counts, the rows behind a channel's count poisoned; both store forms"""
    for case in CASES:
        for N in LEVELS:
            want, want_len = fx.text(case, N)
            for wide in (0, 1):
                out, lens, err = sim_csv(sim, fx.poisoned_sums(case, N), fx.rows(case, N), wide=wide)
                assert (err == 0).all(), (case, N, wide)
                assert same_texts(out, lens, want, want_len) == "", (case, N, wide)


def test_counted_csv_writer_pitch_room_and_count_above_T(sim, fx):
    case, N = "short", 1
    sums, rows = fx.poisoned_sums(case, N), fx.rows(case, N).astype(np.uint64)
    want, want_len = fx.text(case, N)
    T, Cn = sums.shape
    wide_in = np.full((T, Cn + 5), np.float32(np.nan), dtype=np.float32)
    wide_in[:, :Cn] = sums
    out, lens, err = sim_csv(sim, wide_in, rows, Cn=Cn)
    assert (err == 0).all() and same_texts(out, lens, want, want_len) == ""
    # a stride that the long channels do not fit: they report ERROR_MEMORY, and only they -- dead rows take no room
    stride = 256
    out, lens, err = sim_csv(sim, sums, rows, stride=stride)
    fits = want_len + 16 <= stride
    assert fits.any() and (~fits).any()
    assert (err[fits] == 0).all() and (err[~fits] == -6).all() and (lens[~fits] == 0).all()
    assert same_texts(out[fits], lens[fits], want[fits], want_len[fits]) == ""
    bad = [2, 64]
    rows[bad] = [T + 1, 2 ** 50]
    out, lens, err = sim_csv(sim, sums, rows)
    keep = np.ones(Cn, dtype=bool)
    keep[bad] = False
    assert (err[bad] == INVALID).all() and (lens[bad] == 0).all() and (err[keep] == 0).all()
    assert same_texts(out[keep], lens[keep], want[keep], want_len[keep]) == ""


def sim_encode(S, v, count, vs, ad, cap):
    v = np.ascontiguousarray(v, dtype=np.float32)
    count = np.ascontiguousarray(count, dtype=np.uint64)
    T, Cn = v.shape
    out = np.zeros((Cn, cap), dtype=np.uint8)
    bits = np.full(Cn, 99999, dtype=np.uint64)
    err = np.full(Cn, 77, dtype=np.int32)
    assert S.sim_encode_f32_var(v.ctypes.data, Cn, T, Cn, count.ctypes.data, FACTOR, ad, vs, out.ctypes.data, cap, bits.ctypes.data, err.ctypes.data) == 0
    return out, bits, err


def test_counted_encoder(sim, fx, dca):
    """the float entry over every level's (poisoned) rows with that level's counts: all four sets, all six instantiations"""
    for case in CASES:
        for N in LEVELS:
            rows = fx.rows(case, N)
            v = fx.v(case) if N == 1 else fx.poisoned_sums(case, N)  # (level 1 is coded from the readings themselves)
            cap = dca.library().dega_hip_worst_case_bytes64(v.shape[0])
            for vs, ad in SETS:
                got = sim_encode(sim, v, rows, vs, ad, cap)
                assert same_streams(*got, *fx.dega(case, N, vs, ad)) == "", (case, N, vs, ad)
    # the two remaining instantiations (static x narrow, static x 64 bits) against the library-independent property: every
    # channel alone, cut to its count, through the same emulated kernel
    v, count = fx.v("short"), fx.count("short")
    cap = dca.library().dega_hip_worst_case_bytes64(v.shape[0])
    for vs in (16, 64):
        out, bits, err = sim_encode(sim, v, count, vs, 0, cap)
        for c in (0, 1, 2, HONEST, 40, 69):
            n = int(count[c])
            one = sim_encode(sim, np.ascontiguousarray(v[:n, c : c + 1]).reshape(n, 1) if n else np.zeros((0, 1), dtype=np.float32), [n], vs, 0, cap)
            assert same_streams(out[c : c + 1], bits[c : c + 1], err[c : c + 1], *one) == "", (vs, c)


def test_counted_encoder_with_a_slow_coding_wave(sim, fx, dca):
    """the rings between filler and coder run full (the coder's waves sleep at every look at their partners): a lane that has
    ended must not hold the wave's tail back, nor be taken for one that still fills"""
    case, N, vs, ad = "long", 1, 32, 1
    v = fx.v(case)
    sim.sim_ragged_set_drag(4, 20)  # waves 4 .. of the workgroup: coders and writers
    try:
        got = sim_encode(sim, v, fx.rows(case, N), vs, ad, dca.library().dega_hip_worst_case_bytes(v.shape[0]))
    finally:
        sim.sim_ragged_set_drag(1 << 30, 0)
    assert same_streams(*got, *fx.dega(case, N, vs, ad)) == ""


def test_counted_encoder_count_above_T(sim, fx, dca):
    case, N = "short", 1
    v, count = fx.v(case), fx.count(case).astype(np.uint64)
    bad = [1, 30, 66]
    count[bad] = [97, 2 ** 33, 2 ** 64 - 1]
    for vs, ad in ((32, 1), (64, 1)):
        out, bits, err = sim_encode(sim, v, count, vs, ad, dca.library().dega_hip_worst_case_bytes64(v.shape[0]))
        want_out, want_bits, want_err = fx.dega(case, N, vs, ad)
        keep = np.ones(count.size, dtype=bool)
        keep[bad] = False
        assert (err[bad] == INVALID).all() and (bits[bad] == 0).all()
        assert same_streams(out[keep], bits[keep], err[keep], want_out[keep], want_bits[keep], want_err[keep]) == "", (vs, ad)


def test_poison_is_what_the_fixture_says():
    assert np.isnan(POISON[0]) and np.isinf(POISON[1]) and POISON[2] > 2.9e38 and np.signbit(POISON[3]) and POISON[3] == 0
    a = poisoned(np.ones((5, 2), dtype=np.float32), [2, 5])
    assert np.isnan(a[2, 0]) and np.isinf(a[3, 0]) and (a[:, 1] == 1).all()
