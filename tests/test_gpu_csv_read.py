"""GPU tests (-m gpu) of `decode csv` on the device, through the C ABI: the reader alone (device and host pointers), behind
the LZMH decoder (dega_hip_lzmh_decode_f32_dev), behind the writer, and in front of the encoders of both of the study's
chains.  Every comparison is exact bit patterns and exact counts.

What is compared against: tests/golden/csv_read.npz (returned by the compiled reference), libc's strtof through ctypes --
what the reference calls; the fixture's generator and tests/test_csv_read_host.py pin the two to each other -- and the
streams of tests/golden/csv.npz and aggregate.npz."""
import os
import sys

import numpy as np
import pytest

from __graft_entry__ import load_package

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import csv_read_common as crc  # noqa: E402
from agg_common import meter  # noqa: E402
from csv_common import GOLDEN, SLACK, Fixture, input_series, input_txt  # noqa: E402

pytestmark = pytest.mark.gpu
FILLER = 0x7FC12345


@pytest.fixture(scope="module")
def dca():
    return load_package()


@pytest.fixture(scope="module")
def ctx(dca):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; the product has no CPU fallback"
    c = dca.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return crc.ReadFixture()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def read(ctx, texts, max_T, column=1, sep=",", ld=None, stride=None):
    """Returns (values uint32 [max_T][ld], count, err); the columns beyond the channels hold FILLER and must keep it."""
    import torch
    rows, lens = crc.pack(texts, stride)
    Cn = len(texts)
    ld = Cn if ld is None else ld
    out = dev(np.full((max_T, ld), FILLER, dtype=np.uint32).view(np.float32))
    v, count, err = ctx.csv_read(dev(rows), dev(lens.astype(np.int64)), max_T, column, chr(sep) if isinstance(sep, int) else sep, ld=ld, out=out)
    torch.cuda.synchronize()
    v = host(v).view(np.uint32)
    assert (v[:, Cn:] == FILLER).all(), "a column beyond the channels was written"
    return v, host(count), host(err)


# ---- the reader alone --------------------------------------------------------------------------------------------------------

def test_csv_read_vs_fixture(ctx, fx):
    """every case of csv_read.npz: one channel per case, the cases of one (column, separator_char) in one launch"""
    by_options = {}
    for name in fx.cases():
        by_options.setdefault(fx.options(name), []).append(name)
    values = 0
    for (column, sep), names in by_options.items():
        texts = [fx.text(n) for n in names]
        want = [fx.bits(n) for n in names]
        max_T = max(len(w) for w in want)
        v, count, err = read(ctx, texts, max_T, column, sep, ld=len(texts) + 3)
        values += crc.check_channels(v, count, err, want, [0] * len(texts), max_T, (column, sep))
    assert values >= 130000
    assert (fx.bits("input") == input_series().view(np.uint32).ravel()).all()


def test_csv_read_vs_strtof_on_a_random_batch(ctx):
    """all classes of random fields mixed, 2 x 10^5 of them over 700 channels, and every class alone over 300"""
    kinds = {"printed0": lambda r, n: crc.fields_printed(r, n, 0), "printed2": lambda r, n: crc.fields_printed(r, n, 2),
             "printed6": lambda r, n: crc.fields_printed(r, n, 6), "digits": crc.fields_digits, "exponents": crc.fields_exponents, "hex": crc.fields_hex,
             "midpoints": crc.fields_midpoints}
    rng = np.random.default_rng(61)
    mixed = []
    for kind, make in kinds.items():
        fields = make(rng, 30000)
        texts, want = crc.deal(fields, 300)
        v, count, err = read(ctx, texts, 100, ld=304)
        assert crc.check_channels(v, count, err, want, [0] * 300, 100, kind) == 30000
        mixed += fields
    order = rng.permutation(len(mixed))
    mixed = [mixed[i] for i in order]
    texts, want = crc.deal(mixed, 700)
    v, count, err = read(ctx, texts, 300)
    assert crc.check_channels(v, count, err, want, [0] * 700, 300, "mixed") == len(mixed)


def test_csv_read_long_fields_and_small_rooms(ctx):
    """fields of 48 characters and more stop their channel with ERROR_INVALID_FORMAT; more values than max_T give ERROR_MEMORY
    and the room needed; max_T = 0 counts only; an empty channel; the neighbours are unaffected"""
    long47 = b"-340282346638528859811704183484516925440.000000"
    texts = [b"1\n2\n" + b"1" * 48 + b"\n3\n", b"1" * 48, b"1" * 47, long47 + b"\n1\n", b"5\n" + long47 + b"\n", b"5\n" + long47, b"",
             b"1.5\n" * 40 + b"9" * 100 + b"\n" + b"2.5\n" * 40, b"7\n" * 90, b" " * 47 + b"1\n"]
    want, status = zip(*[crc.expected(t) for t in texts])
    assert [s != 0 for s in status] == [True, True, False, False, True, False, False, True, False, True]
    assert [len(w) for w in want] == [2, 0, 1, 2, 1, 2, 0, 40, 90, 0]
    for max_T in (90, 41, 40, 2, 1, 0):
        v, count, err = read(ctx, texts, max_T, ld=12)
        crc.check_channels(v, count, err, want, status, max_T, max_T)


def test_csv_read_host(ctx, fx):
    rng = np.random.default_rng(62)
    fields = crc.fields_printed(rng, 4000, 2) + crc.fields_midpoints(rng, 3000) + crc.fields_hex(rng, 1000)
    texts, want = crc.deal(fields, 70)
    rows, lens = crc.pack(texts)
    max_T = max(len(w) for w in want)
    for ld in (70, 75):
        v, count, err = ctx.csv_read_host(rows, lens, max_T, ld=ld)
        assert crc.check_channels(v.view(np.uint32), count, err, want, [0] * 70, max_T, ld) == len(fields)
        assert (v[:, 70:] == 0).all()
    v, count, err = ctx.csv_read_host(rows, lens, 10)
    crc.check_channels(v.view(np.uint32), count, err, want, [0] * 70, 10, "small")
    # the reference's own file
    rows, lens = crc.pack([input_txt()])
    T = input_series().shape[0]
    v, count, err = ctx.csv_read_host(rows, lens, T)
    assert int(count[0]) == T and int(err[0]) == 0 and (v.view(np.uint32) == input_series().view(np.uint32)).all()
    # col3 of the fixture through the host form
    name = "grammar.col3"
    rows, lens = crc.pack([fx.text(name)])
    v, count, err = ctx.csv_read_host(rows, lens, fx.bits(name).size, column=3, separator_char=";")
    assert int(count[0]) == fx.bits(name).size and (v.view(np.uint32)[:, 0] == fx.bits(name)).all()


# ---- behind the writer, behind LZMH, in front of the encoders ----------------------------------------------------------------

def two_decimal_walk(ctx, Cn, T):
    """the benchmark's workload as floats of two-decimal numbers: centi-units / 100, divided in double (a tensor divisor:
    torch multiplies by the reciprocal of a scalar one, which is an ulp off on many readings) and rounded once"""
    import torch
    x = ctx.synth(Cn, T, seed=1234, S=50)
    hundred = torch.full((), 100.0, dtype=torch.float64, device=x.device)
    v = torch.empty((T, Cn), dtype=torch.float32, device=x.device)
    for t0 in range(0, T, 8192):
        v[t0:t0 + 8192] = (x[t0:t0 + 8192].to(torch.float64) / hundred).to(torch.float32)
    return v


def test_csv_write_then_csv_read_is_the_input(ctx):
    """floats of two-decimal numbers come back bit for bit through their two-decimal text"""
    import torch
    v = two_decimal_walk(ctx, 1000, 5000)
    text, lens, err = ctx.csv_write(v, 2, stride=5000 * 10 + 16)
    back, count, rerr = ctx.csv_read(text, lens, 5000)
    torch.cuda.synchronize()
    assert (err == 0).all() and (rerr == 0).all() and (count == 5000).all()
    assert torch.equal(back.view(torch.int32), v.view(torch.int32))
    # and at other places, in another column
    rng = np.random.default_rng(63)
    m = meter(rng, 700, 130, top=70000.0)
    m[::13, ::5] = -0.0
    for d, column, sep in ((2, 1, ","), (6, 3, ";")):
        w = dev(m)
        text, lens, err = ctx.csv_write(w, d, column, sep)
        back, count, rerr = ctx.csv_read(text, lens, 700, column, sep)
        torch.cuda.synchronize()
        assert (rerr == 0).all() and (count == 700).all() and torch.equal(back.view(torch.int32), w.view(torch.int32)), d


def test_lzmh_encode_f32_then_lzmh_decode_f32_is_the_input(ctx):
    import torch
    v = two_decimal_walk(ctx, 600, 3000)
    stride = 3000 * 10 + 16
    out, bits, tlen, err = ctx.lzmh_encode_f32(v, stride)
    back, count, tlen2, derr = ctx.lzmh_decode_f32(out, bits, stride, 3000)
    torch.cuda.synchronize()
    assert (err == 0).all() and (derr == 0).all() and (count == 3000).all() and torch.equal(tlen, tlen2)
    assert torch.equal(back.view(torch.int32), v.view(torch.int32))
    # it is lzmh_decode followed by csv_read
    text, lens, e1 = ctx.lzmh_decode(out, bits, stride)
    v2, count2, e2 = ctx.csv_read(text, lens, 3000)
    torch.cuda.synchronize()
    assert (e1 == 0).all() and (e2 == 0).all() and torch.equal(v2.view(torch.int32), back.view(torch.int32)) and torch.equal(count, count2)


def test_lzmh_decode_f32_reports_a_text_that_outgrows_its_stride(ctx):
    """ERROR_MEMORY and count 0, not a parse of half a text; the neighbours are unaffected"""
    import torch
    rng = np.random.default_rng(64)
    m = meter(rng, 400, 96, top=40.0)
    m[:, 5::7] = meter(rng, 400, len(range(5, 96, 7)), top=5.0e6)  # longer lines: these channels outgrow the stride
    v = dev(m)
    roomy = 400 * 12 + 16
    out, bits, tlen, err = ctx.lzmh_encode_f32(v, roomy)
    torch.cuda.synchronize()
    assert (err == 0).all()
    sizes = sorted(int(n) for n in host(tlen))
    stride = (sizes[40] + 8 + 15) // 16 * 16
    assert sizes[-1] > stride
    back, count, tlen2, derr = ctx.lzmh_decode_f32(out, bits, stride, 400)
    torch.cuda.synchronize()
    over = 0
    for c in range(96):
        if int(tlen[c]) > stride:
            assert int(derr[c]) == crc.ERROR_MEMORY and int(count[c]) == 0, c
            over += 1
        elif int(derr[c]) == 0:
            assert int(count[c]) == 400 and torch.equal(back[:, c].view(torch.int32), v[:, c].view(torch.int32)), c
        else:  # (the LZMH decoder's own margin at the end of a row)
            assert int(derr[c]) == crc.ERROR_MEMORY and int(count[c]) == 0 and int(tlen[c]) + 16 > stride, c
    assert 0 < over < 96 and int((derr == 0).sum()) >= 40


def test_csv_read_of_input_txt_feeds_both_chains(ctx):
    """`decode csv # encode aggregate num_values=60 # ...` on the device from the text on: the DEGA stream of aggregate.npz
    and the LZMH stream of csv.npz"""
    import torch
    rows, lens = crc.pack([input_txt()])
    T = input_series().shape[0]
    v, count, err = ctx.csv_read(dev(rows), dev(lens.astype(np.int64)), T)
    torch.cuda.synchronize()
    assert int(count[0]) == T and int(err[0]) == 0
    (out, bits, eerr), = ctx.encode_f32_levels(v, [60], factor=100.0, adaptive=1)
    golden = np.load(os.path.join(GOLDEN, "aggregate.npz"))
    n = int(golden["series.vs32.ad.bits"][0])
    torch.cuda.synchronize()
    assert int(eerr[0]) == 0 and int(bits[0]) == n
    assert host(out)[0, : (n + 7) // 8].tobytes() == golden["series.vs32.ad.stream"][0, : (n + 7) // 8].tobytes()
    texts, streams, want_bits = Fixture().chain("series.N60")
    (out, bits, tlen, lerr), = ctx.lzmh_encode_levels_f32(v, [60], (len(texts[0]) + SLACK + 15) // 16 * 16)
    torch.cuda.synchronize()
    assert int(lerr[0]) == 0 and int(tlen[0]) == len(texts[0]) and int(bits[0]) == want_bits[0] == 54154
    assert host(out)[0, : len(streams[0])].tobytes() == streams[0]


def test_csv_read_full_length_series(ctx):
    """one batch at T = 86 400 x 256 channels of the benchmark's walk: write, read, the same floats"""
    import torch
    v = two_decimal_walk(ctx, 256, 86400)
    text, lens, err = ctx.csv_write(v, 2, stride=86400 * 9 + 16)
    back, count, rerr = ctx.csv_read(text, lens, 86400)
    torch.cuda.synchronize()
    assert (err == 0).all() and (rerr == 0).all() and (count == 86400).all() and torch.equal(back.view(torch.int32), v.view(torch.int32))


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(dca, ctx):
    import torch
    L = dca.library()
    E = dca.ERROR_INVALID_VALUE
    s = ctx._stream()
    text = torch.full((8, 1024), 0x31, dtype=torch.uint8, device="cuda")
    lens = torch.full((8,), 40, dtype=torch.int64, device="cuda")
    v = torch.full((64, 8), 7.0, dtype=torch.float32, device="cuda")
    count = torch.full((8,), 77, dtype=torch.int64, device="cuda")
    err = torch.full((8,), 77, dtype=torch.int32, device="cuda")
    p = lambda t: t.data_ptr()  # noqa: E731

    def rd(tx=p(text), stride=1024, ln=p(lens), C_=8, column=1, sep=44, vv=p(v), max_T=64, ld=8, cn=p(count), er=p(err)):
        return L.dega_hip_csv_read_dev(ctx._h, tx, stride, ln, C_, column, sep, vv, max_T, ld, cn, er, s)

    assert rd(column=0) == E and rd(sep=256) == E and rd(sep=-1) == E and rd(ld=7) == E
    assert rd(stride=1000) == E and rd(stride=0) == E and rd(stride=2 ** 31) == E and rd(tx=p(text) + 8) == E
    assert rd(tx=None) == E and rd(ln=None) == E and rd(ln=p(lens) + 4) == E and rd(vv=None) == E and rd(vv=p(v) + 2) == E
    assert rd(cn=None) == E and rd(er=None) == E and rd(cn=p(count) + 4) == E and rd(er=p(err) + 2) == E
    assert rd(vv=p(text), max_T=4) == E  # v_tc overlaps text

    def dec(i=p(text), cap=1024, b=p(lens), C_=8, ts=1024, column=1, sep=44, vv=p(v), max_T=64, ld=8, cn=p(count), tl=None, er=p(err)):
        return L.dega_hip_lzmh_decode_f32_dev(ctx._h, i, cap, b, C_, ts, column, sep, vv, max_T, ld, cn, tl, er, s)

    assert dec(column=0) == E and dec(sep=256) == E and dec(ld=7) == E and dec(ts=1000) == E and dec(ts=8) == E and dec(cap=1022) == E and dec(cap=0) == E
    assert dec(i=p(text) + 2) == E and dec(i=None) == E and dec(b=None) == E and dec(vv=None) == E and dec(cn=None) == E and dec(er=None) == E

    hrows, hlens = crc.pack([b"1\n2\n"] * 4, stride=16)
    hv, hcount, herr = np.full((4, 4), 7.0, dtype=np.float32), np.full(4, 77, dtype=np.uint64), np.full(4, 77, dtype=np.int32)

    def hst(tx=hrows.ctypes.data, stride=16, ln=hlens, C_=4, column=1, sep=44, vv=hv.ctypes.data, max_T=4, ld=4):
        return L.dega_hip_csv_read_host(ctx._h, tx, stride, ln.ctypes.data, C_, column, sep, vv, max_T, ld, hcount.ctypes.data, herr.ctypes.data)

    too_long = hlens.copy()
    too_long[2] = 17
    assert hst(column=0) == E and hst(sep=300) == E and hst(ld=3) == E and hst(stride=24) == E and hst(tx=None) == E and hst(vv=None) == E
    assert hst(ln=too_long) == E  # a len[c] above stride, where the host can see it
    torch.cuda.synchronize()
    assert (v == 7.0).all() and (count == 77).all() and (err == 77).all() and (hv == 7.0).all() and (hcount == 77).all() and (herr == 77).all()
    # C = 0: nothing to do.  max_T = 0: counts only, v_tc may be null
    assert rd(C_=0) == 0 and dec(C_=0) == 0 and hst(C_=0) == 0
    torch.cuda.synchronize()
    assert (count == 77).all() and (err == 77).all()
    assert rd(max_T=0, vv=None) == 0
    torch.cuda.synchronize()
    assert (count == 1).all() and (err == crc.ERROR_MEMORY).all() and (v == 7.0).all()  # forty 1s: one field
    # on the device a len[c] above stride cannot be refused: that channel reports it, its neighbours read on
    lens[3] = 1025
    assert rd() == 0
    torch.cuda.synchronize()
    assert int(err[3]) == E and int(count[3]) == 0 and (err[:3] == 0).all() and (count[:3] == 1).all() and (err[4:] == 0).all()
    assert hst() == 0 and (hcount == 2).all() and (herr == 0).all() and (hv[:2].view(np.uint32) == [[0x3F800000] * 4, [0x40000000] * 4]).all()
