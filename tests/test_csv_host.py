"""`encode csv` on the device, the part that needs no GPU: the new symbols of the C ABI, the size functions, the refusals
that come before any device call, and the kernel's LOGIC -- the shipped kernel source
(data-compressor_amd/csrc/csv_kernels.hpp) compiled by g++ under the thread-per-lane emulator of tests/sim/ against
tests/golden/csv.npz (what the compiled reference wrote) and against Python's formatting on random bit patterns.  Every
text comparison is exact bytes and exact lengths.  The parity tests proper are tests/test_gpu_csv.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from __graft_entry__ import load_package

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from agg_common import sequential  # noqa: E402
from csv_common import DECIMALS, SLACK, Fixture, arrange, check_channels, input_series, input_txt, py_lines  # noqa: E402
from sim_build import sim_library  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("dega_hip_csv_line_max", "dega_hip_csv_worst_case_bytes", "dega_hip_csv_write_dev", "dega_hip_csv_write_host",
               "dega_hip_lzmh_encode_f32_dev", "dega_hip_lzmh_encode_levels_f32_dev")
FLT_MAX_NEG = 0xFF7FFFFF


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
    assert "dega_hip_csv_" in top and "csv.c:46-65" in top  # the block comment lists what each entry replaces
    for method in ("csv_write", "csv_write_host", "lzmh_encode_f32", "lzmh_encode_levels_f32"):
        assert hasattr(dca.Context, method), method


def test_size_functions(dca, fx):
    assert dca.csv_line_max(6, 1) == 48 and dca.csv_line_max(0, 1) == 41 and dca.csv_line_max(2, 1) == 44
    # the longest line there is: -FLT_MAX at 6 decimals, here in column 3
    longest = py_lines([FLT_MAX_NEG], 6, 3, ";")[0]
    assert len(longest) == 50 == dca.csv_line_max(6, 3)
    for d in DECIMALS:
        assert len(py_lines([FLT_MAX_NEG], d)[0]) == dca.csv_line_max(d, 1)
        for name in fx.lists():
            column, sep = fx.options(name)
            assert max(len(s) for s in fx.lines(name, d)[1]) <= dca.csv_line_max(d, column), (name, d)
    for T, d, column in ((0, 2, 1), (1, 0, 1), (7, 6, 3), (86400, 2, 1), (86400, 6, 1)):
        n = dca.csv_worst_case_bytes(T, d, column)
        assert n % 16 == 0 and T * dca.csv_line_max(d, column) + SLACK <= n < T * dca.csv_line_max(d, column) + SLACK + 16
    assert dca.csv_worst_case_bytes(86400, 6, 1) == 86400 * 48 + 16
    # out of range, and sizes beyond size_t: 0
    assert dca.csv_line_max(7, 1) == 0 and dca.csv_line_max(2, 0) == 0 and dca.csv_line_max(2, 2 ** 64 - 1) == 0
    assert dca.csv_worst_case_bytes(10, 7, 1) == 0 and dca.csv_worst_case_bytes(10, 2, 0) == 0
    assert dca.csv_worst_case_bytes(2 ** 60, 2, 1) == 0 and dca.csv_worst_case_bytes(2 ** 64 - 1, 0, 1) == 0
    assert dca.csv_worst_case_bytes((2 ** 64 - 1) // 44, 2, 1) == 0  # (the product fits, the slack and the rounding do not)


def test_null_context_is_rejected(dca):
    L = dca.library()
    buf = (C.c_uint8 * 256)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    nv = (C.c_size_t * 2)(2, 4)
    two = (C.c_void_p * 2)(p, p)
    sizes = (C.c_size_t * 2)(64, 64)
    E = dca.ERROR_INVALID_VALUE
    assert L.dega_hip_csv_write_dev(None, p, 1, 4, 1, 2, 1, 44, p, 64, p, p, None) == E
    assert L.dega_hip_csv_write_host(None, p, 1, 4, 1, 2, 1, 44, p, 64, p, p) == E
    assert L.dega_hip_lzmh_encode_f32_dev(None, p, 1, 4, 1, 2, 1, 44, 64, p, 64, p, p, p, None) == E
    assert L.dega_hip_lzmh_encode_levels_f32_dev(None, p, 1, 4, 1, nv, 2, 2, 1, 44, sizes, two, sizes, two, two, two, None) == E


# ---- kernel logic under the emulator ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sim():
    S = sim_library("csv")
    S.sim_csv.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                          C.c_int]
    return S


def sim_csv(S, batch, Cn, d, column=1, sep=",", stride=None, wide=0):
    """batch: uint32 [T][ld] bit patterns.  Returns (text rows uint8 [Cn][stride], lens, err)."""
    batch = np.ascontiguousarray(batch, dtype=np.uint32)
    T, ld = batch.shape
    if stride is None:
        stride = (T * (column - 1 + 48) + SLACK + 15) // 16 * 16
    raw = np.full(Cn * stride + 16, 0xEE, dtype=np.uint8)
    at = (-raw.ctypes.data) % 16
    out = raw[at: at + Cn * stride].reshape(Cn, stride)
    lens = np.full(Cn, 2 ** 63, dtype=np.uint64)
    err = np.full(Cn, 77, dtype=np.int32)
    assert S.sim_csv(batch.ctypes.data, Cn, T, ld, d, column, ord(sep), out.ctypes.data, stride, lens.ctypes.data, err.ctypes.data, wide) == 0
    return out, lens, err


def test_kernel_source_matches_the_reference_text(sim, fx):
    """every list of the fixture at every num_decimal_places, both store forms; 37 channels (no multiple of 64 or 4), ld > C"""
    lines_checked = 0
    for name in fx.lists():
        column, sep = fx.options(name)
        for d in DECIMALS:
            bits, lines = fx.lines(name, d)
            batch, want = arrange(bits, lines, 37, 41, py_lines([0], d, column, sep)[0])
            for wide in (0, 1):
                out, lens, err = sim_csv(sim, batch, 37, d, column, sep, wide=wide)
                assert check_channels(out, lens, err, want, out.shape[1], (name, d, wide)) == (37, 0)
            lines_checked += len(lines)
    assert lines_checked >= 20000 and set(fx.lists()) >= {"edge", "binades", "col3"} | {"ties_d%d" % d for d in DECIMALS}


def test_kernel_source_on_lines_the_reference_cannot_write(sim, fx):
    """lines of 48 characters and more overrun the reference's buffer (csv.c:11) and are not in the fixture: against Python"""
    n = 0
    for d in DECIMALS:
        bits = np.concatenate([fx.left_out(name, d) for name in ("edge", "binades")])
        n += bits.size
        if bits.size == 0:
            continue
        assert d == 6 and all(len(s) >= 48 for s in py_lines(bits, d))
        batch, want = arrange(bits, py_lines(bits, d), 3, 3, b"0.000000\n")
        for wide in (0, 1):
            out, lens, err = sim_csv(sim, batch, 3, d, wide=wide)
            assert check_channels(out, lens, err, want, out.shape[1], (d, wide)) == (3, 0)
    assert n > 0


def test_kernel_source_more_than_one_workgroup_and_short_series(sim, fx):
    bits, lines = fx.lines("binades", 2)
    for Cn, ld in ((300, 300), (257, 260), (1, 1), (64, 64)):
        batch, want = arrange(bits, lines, Cn, ld, b"0.00\n")
        for wide in (0, 1):
            out, lens, err = sim_csv(sim, batch, Cn, 2, wide=wide)
            assert check_channels(out, lens, err, want, out.shape[1], (Cn, wide)) == (Cn, 0)
    # fewer rows than the kernel keeps in flight, exactly as many, one more
    for T in (1, 2, 15, 16, 17, 31, 32, 33):
        batch, want = arrange(bits[: 5 * T], lines[: 5 * T], 5, 8, b"0.00\n")
        assert batch.shape[0] == T
        for wide in (0, 1):
            out, lens, err = sim_csv(sim, batch, 5, 2, wide=wide)
            assert check_channels(out, lens, err, want, out.shape[1], (T, wide)) == (5, 0)


def test_kernel_source_a_stride_some_channels_outgrow(sim, fx):
    """ERROR_MEMORY and length 0 for the channels whose text + 16 does not fit, the exact text for their neighbours"""
    bits, lines = fx.lines("binades", 6)
    batch, want = arrange(bits, lines, 37, 41, b"0.000000\n")
    sizes = sorted(len(w) for w in want)
    for stride in ((sizes[18] + SLACK + 15) // 16 * 16, (sizes[0] + SLACK + 15) // 16 * 16, 16, (sizes[-1] + SLACK - 1) // 16 * 16):
        for wide in (0, 1):
            out, lens, err = sim_csv(sim, batch, 37, 6, stride=stride, wide=wide)
            fit, over = check_channels(out, lens, err, want, stride, (stride, wide))
            assert over >= 1 and (fit >= 1 or stride <= (sizes[0] + SLACK + 15) // 16 * 16), (stride, fit, over)
    # the boundary itself: text + 16 == stride fits, one byte more does not
    one = [len(s) for s in lines[:64]]
    for T in range(1, 40):
        total = sum(one[:T])
        if (total + SLACK) % 16 == 0:
            batch1, want1 = arrange(bits[:T], lines[:T], 1, 1, b"")
            batch1 = batch1.reshape(T, 1)
            for wide in (0, 1):
                out, lens, err = sim_csv(sim, batch1, 1, 6, stride=total + SLACK, wide=wide)
                assert check_channels(out, lens, err, [b"".join(lines[:T])], total + SLACK, T) == (1, 0)
                out, lens, err = sim_csv(sim, batch1, 1, 6, stride=total, wide=wide)
                assert int(err[0]) == -6 and int(lens[0]) == 0
            break
    else:
        raise AssertionError("no prefix of the list ends 16 bytes before a multiple of 16")


def test_kernel_source_matches_python_on_random_bit_patterns(sim):
    """10^5 random bit patterns per num_decimal_places in {0, 2, 6}, the over-long lines included; 250 channels"""
    rng = np.random.default_rng(50)
    for d in (0, 2, 6):
        bits = rng.integers(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32)
        lines = py_lines(bits, d)
        batch, want = arrange(bits, lines, 250, 250, b"")
        wide = 1 if d == 2 else 0
        out, lens, err = sim_csv(sim, batch, 250, d, wide=wide)
        assert check_channels(out, lens, err, want, out.shape[1], d) == (250, 0)
        if d == 6:
            assert any(len(s) >= 48 for s in lines)
    # and where the readings of the study live: two-decimal values and their neighbours in float32
    base = (np.round(rng.uniform(0.0, 70000.0, 100000) * 100.0) / 100.0).astype(np.float32).view(np.uint32)
    bits = base + rng.integers(-2, 3, base.size).astype(np.uint32)
    for d, wide in ((2, 0), (1, 1), (3, 0)):
        batch, want = arrange(bits, py_lines(bits, d), 250, 250, b"")
        out, lens, err = sim_csv(sim, batch, 250, d, wide=wide)
        assert check_channels(out, lens, err, want, out.shape[1], d) == (250, 0)


def test_kernel_source_renders_the_chains_of_the_fixture(sim, fx):
    """the text of `encode aggregate # encode csv` (sums restated in numpy) and of `encode csv` alone; -0.0f pinned both ways"""
    v = fx.meter()
    texts, _, _ = fx.chain("meter.plain")
    assert texts[0].startswith(b"-0.00\n")
    out, lens, err = sim_csv(sim, v.view(np.uint32), v.shape[1], 2)
    assert check_channels(out, lens, err, texts, out.shape[1], "plain") == (v.shape[1], 0)
    for N in (1, 7, 60):
        texts, _, _ = fx.chain("meter.N%d" % N)
        a = sequential(v, N)
        out, lens, err = sim_csv(sim, a.view(np.uint32), a.shape[1], 2, wide=N % 2)
        assert check_channels(out, lens, err, texts, out.shape[1], N) == (v.shape[1], 0)
    assert fx.chain("meter.N1")[0][0].startswith(b"0.00\n")
    # the reference's own series: `decode csv # encode csv` is input.txt again
    s = input_series()
    out, lens, err = sim_csv(sim, s.view(np.uint32), 1, 2, stride=(len(input_txt()) + SLACK + 15) // 16 * 16)
    assert check_channels(out, lens, err, [input_txt()], out.shape[1], "series") == (1, 0)
    texts, _, bits = fx.chain("series.N60")
    a = sequential(s, 60)
    out, lens, err = sim_csv(sim, a.view(np.uint32), 1, 2, wide=1)
    assert check_channels(out, lens, err, texts, out.shape[1], "series N60") == (1, 0) and bits == [54154]


def test_fixture_is_not_blind(fx):
    """what the generator asserted, seen from here: Python's formatting reproduces every stored line (the signed NaNs
    through the patch of py_lines), and ties that go to even are among them"""
    n = nan_signed = 0
    for name in fx.lists():
        column, sep = fx.options(name)
        for d in DECIMALS:
            bits, lines = fx.lines(name, d)
            assert py_lines(bits, d, column, sep) == lines, (name, d)
            n += len(lines)
            nan_signed += sum(1 for s in lines if s.endswith(b"-nan\n"))
    assert n >= 20000 and nan_signed > 0
    for value, d, text in ((0.125, 2, b"0.12\n"), (0.375, 2, b"0.38\n"), (0.5, 0, b"0\n"), (1.5, 0, b"2\n"), (2.5, 0, b"2\n"), (-0.0, 2, b"-0.00\n"),
                           (-0.001, 2, b"-0.00\n"), (7405.3003, 2, b"7405.30\n"), (1e-45, 2, b"0.00\n"), (9.995, 2, b"9.99\n"), (99999.996, 1, b"100000.0\n")):
        b = int(np.array([value], dtype=np.float32).view(np.uint32)[0])
        found = [line for name in ("edge", "ties_d%d" % d) for bb, line in zip(*fx.lines(name, d)) if int(bb) == b]
        assert found and all(line == text for line in found), (value, d, found)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "csv.npz")) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "aggregate_levels.npz"))
