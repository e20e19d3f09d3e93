"""`decode csv` on the device, the part that needs no GPU: the new symbols of the C ABI, the one refusal that needs no
context (the others are checked against the library in tests/test_gpu_csv_read.py), and the kernel's LOGIC -- the shipped kernel source (data-compressor_amd/csrc/csv_read_kernels.hpp) compiled
by g++ under the thread-per-lane emulator of tests/sim/ against tests/golden/csv_read.npz (what the compiled reference
returned) and against libc's strtof on random fields.  Every comparison is exact bit patterns and exact counts, and no
case is left out of one: the only status other than 0 is that of the fields of 48 characters and more, on inputs built to
have it, which are a separate, counted set.  The parity tests proper are tests/test_gpu_csv_read.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from __graft_entry__ import load_package

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import csv_read_common as crc  # noqa: E402
from csv_common import Fixture, input_series  # noqa: E402
from sim_build import sim_library  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dega_hip_csv_read_dev", "dega_hip_csv_read_host", "dega_hip_lzmh_decode_f32_dev")
FILLER = 0x7FC12345  # what the columns beyond C hold: no call may touch it
PER_CLASS = 100000


@pytest.fixture(scope="module")
def dca():
    mod = load_package()
    if not os.path.exists(mod.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return mod


@pytest.fixture(scope="module")
def fx():
    return crc.ReadFixture()


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
    assert "dega_hip_csv_read_" in top and "csv.c:13-44" in top  # the block comment lists what each entry replaces
    assert "There is no `decode csv` here" not in header
    for method in ("csv_read", "csv_read_host", "lzmh_decode_f32"):
        assert hasattr(dca.Context, method), method


def test_null_context_is_rejected(dca):
    L = dca.library()
    buf = (C.c_uint8 * 256)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    E = dca.ERROR_INVALID_VALUE
    assert L.dega_hip_csv_read_dev(None, p, 16, p, 1, 1, ord(","), p, 4, 1, p, p, None) == E
    assert L.dega_hip_csv_read_host(None, p, 16, p, 1, 1, ord(","), p, 4, 1, p, p) == E
    assert L.dega_hip_lzmh_decode_f32_dev(None, p, 16, p, 1, 16, 1, ord(","), p, 4, 1, p, p, p, None) == E


# ---- kernel logic under the emulator ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sim():
    S = sim_library("csv_read")
    S.sim_csv_read.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]
    S.sim_csv_read_field.restype = C.c_int64
    S.sim_csv_read_field.argtypes = [C.c_char_p, C.c_size_t]
    return S


def sim_read(S, texts, max_T, column=1, sep=",", ld=None, stride=None):
    """Returns (values uint32 [max_T][ld], count, err); the columns beyond the channels hold FILLER and must keep it."""
    rows, lens = crc.pack(texts, stride)
    Cn = len(texts)
    ld = Cn if ld is None else ld
    v = np.full((max(max_T, 1), ld), FILLER, dtype=np.uint32)
    count = np.full(Cn, 2 ** 63, dtype=np.uint64)
    err = np.full(Cn, 77, dtype=np.int32)
    sep = ord(sep) if isinstance(sep, str) else int(sep)
    assert S.sim_csv_read(rows.ctypes.data, rows.shape[1], lens.ctypes.data, Cn, column, sep, v.ctypes.data, max_T, ld, count.ctypes.data, err.ctypes.data) == 0
    assert (v[:, Cn:] == FILLER).all(), "a column beyond the channels was written"
    assert (v[max_T:] == FILLER).all()
    return v, count, err


def test_field_conversion_alone_matches_the_reference(sim, fx):
    """the kernel's conversion without the splitting and the emulator (sim_csv_read_field: its parser, its steady and its
    general path on one field): every field of the fixture's own texts, and 48 characters refused"""
    n = 0
    for name in fx.cases():
        if name.startswith("back.") or name == "input":
            continue
        column, sep = fx.options(name)
        fields = crc.split(fx.text(name), column, sep)[0]
        got = [sim.sim_csv_read_field(f, len(f)) for f in fields]
        assert got == fx.bits(name).tolist(), name
        n += len(fields)
    assert n >= 3000
    assert sim.sim_csv_read_field(b"1" * 47, 47) == crc.strtof_bits(b"1" * 47) and sim.sim_csv_read_field(b"1" * 48, 48) == -1


def test_kernel_source_matches_the_reference_on_the_fixture(sim, fx):
    """every case of csv_read.npz: one channel per case, the cases of one (column, separator_char) in one launch -- channels
    of very different lengths side by side, in ragged waves"""
    by_options = {}
    for name in fx.cases():
        by_options.setdefault(fx.options(name), []).append(name)
    assert set(by_options) >= {(1, ord(",")), (2, ord(",")), (3, ord(";"))}
    values = 0
    for (column, sep), names in by_options.items():
        texts = [fx.text(n) for n in names]
        want = [fx.bits(n) for n in names]
        max_T = max(len(w) for w in want)
        v, count, err = sim_read(sim, texts, max_T, column, sep, ld=len(texts) + 3)
        values += crc.check_channels(v, count, err, want, [0] * len(texts), max_T, (column, sep))
    assert values >= 130000
    names = set(fx.cases())
    assert {"grammar", "grammar.col3", "binades", "midpoints", "digits", "exponents", "hex", "input", "crlf", "end.separator", "empty.col2"} <= names
    assert any(n.startswith("back.edge.") for n in names) and any(n.startswith("back.col3.") for n in names) and "back.series.N60.c0" in names
    assert (fx.bits("input") == input_series().view(np.uint32).ravel()).all()


def test_fixture_is_not_blind(fx):
    """what the generator asserted, seen from here: libc's strtof agrees with the reference on every stored field; a
    conversion through double, and one that keeps 19 digits, each disagree on some"""
    n = double_differs = trunc_differs = 0
    for name in fx.cases():
        column, sep = fx.options(name)
        fields, status = crc.split(fx.text(name), column, sep)
        bits = fx.bits(name)
        assert status == 0 and len(fields) == bits.size, name
        if name in ("midpoints", "digits"):
            for f, b in zip(fields, bits.tolist()):
                assert crc.strtof_bits(f) == b, (name, f)
                double_differs += crc.float32_via_double(f.strip()) != b
                trunc_differs += crc.strtof_bits(crc.truncated_19(f)) != b
        elif not name.startswith("back.") and name != "input":
            assert [crc.strtof_bits(f) for f in fields] == bits.tolist(), name
        n += bits.size
    assert n >= 130000 and double_differs > 0 and trunc_differs > 0
    z = dict(zip(*[[f.decode() for f in crc.split(fx.text("grammar"))[0]], fx.bits("grammar").tolist()]))
    for field, b in (("nan(0x123)", 0x7FC00123), ("nan(123)", 0x7FC0007B), ("-nan(0x7fffff)", 0xFFFFFFFF), ("nan(zz)", 0x7FC00000), ("nan(", 0x7FC00000),
                     ("NAN()", 0x7FC00000), ("0x1.000001p0", 0x3F800000), ("0x1.000003p0", 0x3F800002), ("0x", 0), ("1e", 0x3F800000), ("1e+", 0x3F800000),
                     ("5.", 0x40A00000), (".5", 0x3F000000), (".", 0), ("infinit", 0x7F800000), ("abc", 0), ("-", 0), ("-abc", 0), ("-0", 0x80000000),
                     ("3.40282357e38", 0x7F800000), ("3.4028235677973366e38", 0x7F7FFFFF)):
        assert z[field] == b, (field, hex(z[field]))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "csv_read.npz")) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "csv.npz"))


def test_kernel_source_reads_the_writers_texts(sim):
    """csv_read of the texts stored in csv.npz (meter.plain, meter.N*) equals strtof of their lines"""
    w = Fixture()
    for key in ("meter.plain", "meter.N1", "meter.N7", "meter.N60"):
        texts = w.chain(key)[0]
        want = [np.array([crc.strtof_bits(s) for s in t.split(b"\n")[:-1]], dtype=np.uint32) for t in texts]
        v, count, err = sim_read(sim, texts, len(want[0]))
        assert crc.check_channels(v, count, err, want, [0] * len(texts), len(want[0]), key) == sum(len(x) for x in want)
    # channel 0 of the plain text starts with -0.00: the sign of zero comes back
    assert int(sim_read(sim, w.chain("meter.plain")[0], 1)[0][0, 0]) == 0x80000000


@pytest.mark.parametrize("kind", ["printed_d0", "printed_d2", "printed_d6", "digits", "exponents", "hex", "midpoints"])
def test_kernel_source_matches_strtof_on_random_fields(sim, kind):
    """10^5 fields per class through the emulated kernel, 250 channels (ragged waves), every one compared with libc"""
    rng = np.random.default_rng(["printed_d0", "printed_d2", "printed_d6", "digits", "exponents", "hex", "midpoints"].index(kind) + 1)
    if kind.startswith("printed"):
        fields = crc.fields_printed(rng, PER_CLASS, int(kind[-1]))
    else:
        fields = getattr(crc, "fields_" + kind)(rng, PER_CLASS)
    assert len(fields) == PER_CLASS and all(len(f) < crc.FIELD_LIMIT for f in fields)
    if kind in ("digits", "exponents", "hex"):  # the longest field the reference can hold is among them
        assert sum(len(f) == crc.FIELD_LIMIT - 1 for f in fields) >= 100, kind
    texts, want = crc.deal(fields, 250)
    v, count, err = sim_read(sim, texts, PER_CLASS // 250, ld=251)
    assert crc.check_channels(v, count, err, want, [0] * 250, PER_CLASS // 250, kind) == PER_CLASS
    if kind == "midpoints":  # the comparison a plausible wrong implementation fails
        flat = np.concatenate(want)
        dealt = [f for c in range(250) for f in fields[c::250]]
        assert sum(crc.float32_via_double(f) != int(b) for f, b in zip(dealt[:30000], flat[:30000])) > 1000
        assert sum(crc.strtof_bits(crc.truncated_19(f)) != int(b) for f, b in zip(dealt[:30000], flat[:30000])) > 1000


def test_kernel_source_fields_of_48_characters_and_more(sim):
    """the one status that is not 0, on inputs built to have it: a separate, counted set.  The channel stops in front of the
    field, its neighbours do not notice; 47 characters are read; the appended last byte counts."""
    long47 = b"-340282346638528859811704183484516925440.000000"
    assert len(long47) == 47
    cases = [  # (text, column, values in front, too long?)
        (b"1\n2\n" + b"1" * 48 + b"\n3\n", 1, 2, True),
        (b"1" * 48, 1, 0, True),
        (b"1" * 47, 1, 1, False),
        (long47 + b"\n1\n", 1, 2, False),
        (b"5\n" + long47 + b"\n", 1, 1, True),  # the last line: its newline is appended
        (b"5\n" + long47, 1, 2, False),
        (b"1,2\n3," + b"0" * 47 + b"7\n5,6\n", 2, 1, True),
        (b"1,2\n3," + b"0" * 47 + b"7\n5,6\n", 1, 3, False),  # (too long, but in a column that is not read)
        (b" " * 47 + b"1\n", 1, 0, True),
        (b"1.5\n" * 40 + b"9" * 100 + b"\n" + b"2.5\n" * 40, 1, 40, True),
    ]
    flagged = 0
    for column in (1, 2):
        mine = [c for c in cases if c[1] == column]
        texts = [c[0] for c in mine]
        want, status = zip(*[crc.expected(t, column) for t in texts])
        for (t, _, n, long_), w, s in zip(mine, want, status):
            assert len(w) == n and (s == crc.ERROR_INVALID_FORMAT) == long_, t
            flagged += long_
        v, count, err = sim_read(sim, texts, 64, column, ld=len(texts) + 1)
        crc.check_channels(v, count, err, want, status, 64, column)
    assert flagged == 6


def test_kernel_source_batch_shapes(sim):
    """ragged waves, more than one workgroup, channels of very different lengths in one wave, an empty channel, and the text
    lengths around the 16-byte pieces and the batch of the kernel"""
    rng = np.random.default_rng(11)
    fields = crc.fields_printed(rng, 6000, 2)
    for Cn, ld in ((1, 1), (63, 64), (64, 64), (65, 70), (257, 260), (300, 300)):
        texts, want = crc.deal(fields[: 20 * Cn], Cn)
        v, count, err = sim_read(sim, texts, 20, ld=ld)
        assert crc.check_channels(v, count, err, want, [0] * Cn, 20, (Cn, ld)) == 20 * Cn
    # one wave: channel c has c * c values (0 .. 3969), channel 7 none at all, channel 9 a single byte
    texts, want = [], []
    at = 0
    for c in range(64):
        n = 0 if c == 7 else c * c
        mine = [fields[(at + i) % len(fields)] for i in range(n)]
        at += n
        texts.append(crc.lines_text(mine))
        want.append(np.array([crc.strtof_bits(f) for f in mine], dtype=np.uint32))
    texts[9], want[9] = b"4", np.array([0x40800000], dtype=np.uint32)
    v, count, err = sim_read(sim, texts, 63 * 63, ld=66)
    assert crc.check_channels(v, count, err, want, [0] * 64, 63 * 63, "lengths") == sum(len(w) for w in want)
    assert int(count[7]) == 0 and int(err[7]) == 0
    # every text length from 0 to 100 bytes, and a stride with room to spare
    base = crc.lines_text(fields[:30])
    texts = [base[:n] for n in range(101)]
    want, status = zip(*[crc.expected(t) for t in texts])
    assert all(s == 0 for s in status)
    for stride in (None, 256):
        v, count, err = sim_read(sim, texts, 32, stride=stride)
        crc.check_channels(v, count, err, want, status, 32, ("prefixes", stride))
    # empty lines: more values per batch than the ring holds, beside a channel of long lines
    texts = [b"\n" * 500, crc.lines_text([b"0.000000000000000000000000000000000000000001"] * 20), b"1\n" * 300, b"," * 10 + b"\n" + b"\n" * 77]
    want, status = zip(*[crc.expected(t) for t in texts])
    v, count, err = sim_read(sim, texts, 500)
    assert crc.check_channels(v, count, err, want, status, 500, "empty lines") == 500 + 20 + 300 + 78


def test_kernel_source_room_for_fewer_values_than_there_are(sim):
    """max_T too small: ERROR_MEMORY and the room needed in out_count, the rows there are exact, nothing beyond them is
    written; max_T = 0 counts only"""
    rng = np.random.default_rng(12)
    fields = crc.fields_printed(rng, 3000, 2)
    texts, want = [], []
    for c in range(70):
        mine = fields[40 * c: 40 * c + (c % 40) + 1]
        texts.append(crc.lines_text(mine))
        want.append(np.array([crc.strtof_bits(f) for f in mine], dtype=np.uint32))
    for max_T in (0, 1, 7, 16, 17, 39, 40):
        v, count, err = sim_read(sim, texts, max_T, ld=72)
        crc.check_channels(v, count, err, want, [0] * 70, max_T, max_T)
        over = sum(1 for w in want if len(w) > max_T)
        assert int((err == crc.ERROR_MEMORY).sum()) == over and (over > 0 or max_T == 40)
