"""GPU tests (-m gpu) of `encode csv` on the device, through the C ABI: the renderer alone (both store forms, device and
host pointers), in front of LZMH (dega_hip_lzmh_encode_f32_dev), behind `aggregate` for several granularities
(dega_hip_lzmh_encode_levels_f32_dev), and behind the float-exit decoder.  Every text comparison is exact bytes and
exact lengths; streams are compared byte for byte and bit length for bit length.

What is compared against: tests/golden/csv.npz (written by the compiled reference), Python's "%.*f" with glibc's sign of
NaN (the fixture's generator and tests/test_csv_host.py pin the two to each other), and the library's own earlier entry
points (lzmh_encode / lzmh_decode / lzmh_render / aggregate / decode_f32: their own tests pin them to the reference)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from __graft_entry__ import load_package

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from agg_common import meter  # noqa: E402
from csv_common import DECIMALS, ERROR_MEMORY, GOLDEN, SLACK, Fixture, arrange, check_channels, input_series, input_txt, py_lines  # noqa: E402

pytestmark = pytest.mark.gpu


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
    return Fixture()


@pytest.fixture(params=["store8", "store64"])
def form(request, monkeypatch):
    """both output forms of the kernel, through the knob the header names"""
    monkeypatch.setenv("DEGA_CSV_STORE", "8" if request.param == "store8" else "64")
    return request.param


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_bits(batch):
    """uint32 bit patterns [T][ld] as a float32 CUDA tensor (a byte copy: NaN payloads and signs survive)"""
    return dev(np.ascontiguousarray(batch, dtype=np.uint32).view(np.float32))


def host(t):
    return t.cpu().numpy()


def write(ctx, batch, Cn, d, column=1, sep=",", stride=None):
    import torch
    text, lens, err = ctx.csv_write(dev_bits(batch), d, column, sep, stride=stride, channels=Cn)
    torch.cuda.synchronize()
    return host(text), host(lens), host(err)


def texts_of(text, lens):
    return [text[c, : int(lens[c])].tobytes() for c in range(lens.size)]


def meter_texts(v, d=2):
    """per channel of a float32 [T][C] array: the text, one C-level format call per channel"""
    T, Cn = v.shape
    fmt = ("%%.%df\n" % d) * T
    return [(fmt % tuple(v[:, c].astype(np.float64).tolist())).encode() for c in range(Cn)]


# ---- the renderer alone ------------------------------------------------------------------------------------------------------

def test_csv_write_vs_fixture(ctx, fx, form):
    """every list of the fixture at every num_decimal_places; 37 channels, ld = 41"""
    n = 0
    for name in fx.lists():
        column, sep = fx.options(name)
        for d in DECIMALS:
            bits, lines = fx.lines(name, d)
            batch, want = arrange(bits, lines, 37, 41, py_lines([0], d, column, sep)[0])
            text, lens, err = write(ctx, batch, 37, d, column, sep)
            assert check_channels(text, lens, err, want, text.shape[1], (name, d)) == (37, 0)
            n += len(lines)
    assert n >= 20000


def test_csv_write_vs_python_on_random_bit_patterns(ctx, fx, form):
    rng = np.random.default_rng(51)
    for d in (0, 2, 6):
        bits = rng.integers(0, 2 ** 32, 120000, dtype=np.uint64).astype(np.uint32)
        lines = py_lines(bits, d)
        batch, want = arrange(bits, lines, 300, 304, b"")
        text, lens, err = write(ctx, batch, 300, d)
        assert check_channels(text, lens, err, want, text.shape[1], d) == (300, 0)
    # the lines the reference cannot write (48 characters and more), which the fixture leaves out
    bits = np.concatenate([fx.left_out(name, 6) for name in ("edge", "binades")])
    assert bits.size > 0
    batch, want = arrange(bits, py_lines(bits, 6), 3, 3, b"0.000000\n")
    text, lens, err = write(ctx, batch, 3, 6)
    assert check_channels(text, lens, err, want, text.shape[1], "long") == (3, 0)


def test_csv_write_memory_errors_do_not_disturb_the_neighbours(ctx, fx, form):
    bits, lines = fx.lines("binades", 6)
    batch, want = arrange(bits, lines, 37, 41, b"0.000000\n")
    sizes = sorted(len(w) for w in want)
    stride = (sizes[18] + SLACK + 15) // 16 * 16
    text, lens, err = write(ctx, batch, 37, 6, stride=stride)
    fit, over = check_channels(text, lens, err, want, stride, stride)
    assert fit >= 1 and over >= 1 and fit + over == 37


def test_csv_write_host(ctx, fx):
    rng = np.random.default_rng(52)
    bits = np.concatenate([fx.lines("edge", 2)[0], rng.integers(0, 2 ** 32, 5000, dtype=np.uint64).astype(np.uint32)])
    for d, column, sep in ((2, 1, ","), (6, 3, ";"), (0, 1, ",")):
        lines = py_lines(bits, d, column, sep)
        batch, want = arrange(bits, lines, 70, 72, py_lines([0], d, column, sep)[0])
        text, lens, err = ctx.csv_write_host(batch.view(np.float32), d, column, sep, channels=70)
        assert check_channels(text, lens, err, want, text.shape[1], (d, column)) == (70, 0)
    # the reference's own series: `decode csv # encode csv` is input.txt again
    text, lens, err = ctx.csv_write_host(input_series(), 2)
    assert check_channels(text, lens, err, [input_txt()], text.shape[1], "series") == (1, 0)


def test_decode_f32_then_csv_write_is_input_txt(ctx):
    """the tail of the reference's `make test` chain on the device: decode bac # decode seg # decode diff # decode normalize # encode csv"""
    import torch
    want = input_txt()
    T = input_series().shape[0]
    with open(os.path.join(GOLDEN, "dega_adaptive.bin"), "rb") as f:
        data = f.read()
    cap = (len(data) + 3) & ~3
    st = np.zeros((66, cap), dtype=np.uint8)
    st[:, : len(data)] = np.frombuffer(data, dtype=np.uint8)
    bits = np.full(66, 8 * len(data), dtype=np.int64)  # the file: zero padded to a byte
    v, derr = ctx.decode_f32(dev(st), dev(bits), T, factor=100.0, adaptive=1)
    text, lens, err = ctx.csv_write(v, 2, stride=(len(want) + SLACK + 15) // 16 * 16)
    torch.cuda.synchronize()
    assert (host(derr) == 0).all()
    assert check_channels(host(text), host(lens), host(err), [want] * 66, text.shape[1], "make test") == (66, 0)


def test_the_two_renderers_agree_where_both_are_defined(ctx, form):
    """csv_write of float32(x / 100) = lzmh_render of the int32 centi-units x, for |x| < 10^6"""
    import torch
    rng = np.random.default_rng(53)
    x = rng.integers(-999999, 1000000, (500, 130)).astype(np.int32)
    x[0, :8] = [0, -1, 1, -99, 99, -100, 999999, -999999]
    v = (x.astype(np.float64) / 100.0).astype(np.float32)
    stride = 500 * 16
    t1, l1, e1 = ctx.lzmh_render(dev(x), stride)
    t2, l2, e2 = ctx.csv_write(dev(v), 2, stride=stride)
    torch.cuda.synchronize()
    assert (host(e1) == 0).all() and (host(e2) == 0).all() and (host(l1) == host(l2)).all()
    assert texts_of(host(t1), host(l1)) == texts_of(host(t2), host(l2))


def test_csv_write_full_length_series(ctx):
    """one batch at T = 86 400 x 256 channels of two-decimal readings against Python's formatting"""
    import torch
    rng = np.random.default_rng(54)
    v = meter(rng, 86400, 256)
    stride = 86400 * 9 + 16
    text, lens, err = ctx.csv_write(dev(v), 2, stride=stride)
    torch.cuda.synchronize()
    assert check_channels(host(text), host(lens), host(err), meter_texts(v), stride, "full") == (256, 0)


# ---- in front of LZMH --------------------------------------------------------------------------------------------------------

def check_streams(out, bits, want_streams, want_bits, what):
    for c, (s, b) in enumerate(zip(want_streams, want_bits)):
        assert int(bits[c]) == b, (what, c, int(bits[c]), b)
        assert out[c, : len(s)].tobytes() == s, (what, c)


def test_lzmh_encode_f32_vs_fixture_streams(ctx, fx, form):
    import torch
    v = fx.meter()
    texts, streams, bits = fx.chain("meter.plain")
    out, obits, tlen, err = ctx.lzmh_encode_f32(dev(v), 420 * 16)
    torch.cuda.synchronize()
    assert (host(err) == 0).all() and [int(n) for n in host(tlen)] == [len(t) for t in texts]
    check_streams(host(out), host(obits), streams, bits, "meter.plain")


def test_lzmh_encode_f32_equals_lzmh_encode_over_the_text_and_decodes_to_it(ctx, form):
    import torch
    rng = np.random.default_rng(55)
    for T, Cn, top, d in ((3000, 300, 5000.0, 2), (1000, 70, 40.0, 2), (500, 64, 700000.0, 1)):
        v = meter(rng, T, Cn, top=top)
        want = meter_texts(v, d)
        stride = (max(len(w) for w in want) + SLACK + 15) // 16 * 16
        text = np.zeros((Cn, stride), dtype=np.uint8)
        for c, w in enumerate(want):
            text[c, : len(w)] = np.frombuffer(w, dtype=np.uint8)
        lens = np.array([len(w) for w in want], dtype=np.int64)
        out, bits, tlen, err = ctx.lzmh_encode_f32(dev(v), stride, decimals=d)
        ref_out, ref_bits, ref_err = ctx.lzmh_encode(dev(text), dev(lens), cap=out.shape[1])
        back, blens, berr = ctx.lzmh_decode(out, bits, (stride + 7) // 8 * 8 + 8)
        torch.cuda.synchronize()
        assert (host(err) == 0).all() and (host(ref_err) == 0).all() and (host(berr) == 0).all()
        assert (host(tlen) == lens).all() and torch.equal(bits, ref_bits)
        nbytes = (host(bits) + 7) // 8
        o, r = host(out), host(ref_out)
        for c in range(Cn):
            assert o[c, : nbytes[c]].tobytes() == r[c, : nbytes[c]].tobytes(), (T, c)
        assert texts_of(host(back), host(blens)) == want


def test_lzmh_encode_f32_memory_errors_do_not_disturb_the_neighbours(dca, ctx):
    import torch
    rng = np.random.default_rng(56)
    v = meter(rng, 400, 96, top=40.0)
    v[:, 5::7] = meter(rng, 400, len(range(5, 96, 7)), top=5.0e6)  # longer lines: these channels outgrow the stride
    want = meter_texts(v)
    sizes = sorted(len(w) for w in want)
    stride = (sizes[40] + SLACK + 15) // 16 * 16
    assert sizes[-1] + SLACK > stride
    roomy = (sizes[-1] + SLACK + 15) // 16 * 16
    out, bits, tlen, err = ctx.lzmh_encode_f32(dev(v), stride, cap=dca.lzmh_worst_case_bytes(roomy))
    full, fbits, ftlen, ferr = ctx.lzmh_encode_f32(dev(v), roomy, cap=dca.lzmh_worst_case_bytes(roomy))
    torch.cuda.synchronize()
    assert (host(ferr) == 0).all()
    over = 0
    for c, w in enumerate(want):
        if len(w) + SLACK <= stride:
            assert int(err[c]) == 0 and int(tlen[c]) == len(w) and int(bits[c]) == int(fbits[c])
            n = (int(bits[c]) + 7) // 8
            assert torch.equal(out[c, :n], full[c, :n]), c
        else:
            assert int(err[c]) == ERROR_MEMORY and int(bits[c]) == 0 and int(tlen[c]) == 0, c
            over += 1
    assert 0 < over < 96


def test_lzmh_encode_f32_calls_on_two_streams_share_the_scratch_safely(ctx):
    """two calls on one context, back to back on different streams without a synchronisation in between; both results equal
    those of the same calls made alone"""
    import torch
    rng = np.random.default_rng(57)
    va, vb = dev(meter(rng, 2000, 1024, top=30.0)), dev(meter(rng, 2000, 1024, top=3000.0))
    stride = 2000 * 9 + 16
    alone = []
    for v in (va, vb):
        res = ctx.lzmh_encode_f32(v, stride)
        torch.cuda.synchronize()
        alone.append([t.clone() for t in res])
    assert not torch.equal(alone[0][1], alone[1][1])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for first, second in ((va, vb), (vb, va)):
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            r1 = ctx.lzmh_encode_f32(first, stride)
        with torch.cuda.stream(s2):
            r2 = ctx.lzmh_encode_f32(second, stride)
        torch.cuda.synchronize()
        w1, w2 = (alone[0], alone[1]) if first is va else (alone[1], alone[0])
        for got, want in ((r1, w1), (r2, w2)):
            assert (got[3] == 0).all() and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
            nbytes = int((int(want[1].max()) + 7) // 8)
            assert torch.equal(got[0][:, :nbytes], want[0][:, :nbytes])


# ---- behind aggregate, several granularities ------------------------------------------------------------------------------------

@pytest.fixture(params=["planned", "shared"])
def sharing(request, monkeypatch):
    """narrow batches get a pass per level; "shared" lowers the planner's workgroup floor so that the levels share passes"""
    if request.param == "shared":
        monkeypatch.setenv("DEGA_AGG_LEVELS_MIN_WORKGROUPS", "1")
    return request.param


def test_lzmh_encode_levels_f32_vs_fixture_chains(ctx, fx, sharing):
    import torch
    v = fx.meter()
    levels = [60, 1, 7]
    res = ctx.lzmh_encode_levels_f32(dev(v), levels, [16 * 16, 420 * 16, 64 * 16])
    torch.cuda.synchronize()
    for N, (out, bits, tlen, err) in zip(levels, res):
        texts, streams, want_bits = fx.chain("meter.N%d" % N)
        assert (host(err) == 0).all() and [int(n) for n in host(tlen)] == [len(t) for t in texts], N
        check_streams(host(out), host(bits), streams, want_bits, N)
    assert fx.chain("meter.N1")[0][0].startswith(b"0.00\n") and fx.chain("meter.plain")[0][0].startswith(b"-0.00\n")
    # the reference's own series, N = 60
    texts, streams, want_bits = fx.chain("series.N60")
    (out, bits, tlen, err), = ctx.lzmh_encode_levels_f32(dev(input_series()), [60], (len(texts[0]) + SLACK + 15) // 16 * 16)
    torch.cuda.synchronize()
    assert int(err[0]) == 0 and int(tlen[0]) == len(texts[0]) and want_bits == [54154]
    check_streams(host(out), host(bits), streams, want_bits, "series")


@pytest.mark.parametrize("levels", [[60, 300], [7, 1, 60], [899, 900, 2], [1]])
def test_lzmh_encode_levels_f32_equals_the_single_calls(dca, ctx, sharing, levels):
    """level by level = aggregate, then lzmh_encode_f32 over the sums; sets that share a pass and sets that do not, N = 1 included"""
    import torch
    rng = np.random.default_rng(58)
    T, Cn = 3601, 520
    v = meter(rng, T, Cn, top=50.0)
    v[::11, ::3] = -0.0
    vd = dev(v)
    if sharing == "shared":
        assert len(dca.aggregate_levels_plan(Cn, T, levels)[1]) == 1
    strides = [(-(-T // N) * 12 + SLACK + 15) // 16 * 16 for N in levels]
    res = ctx.lzmh_encode_levels_f32(vd, levels, strides)
    torch.cuda.synchronize()
    for N, stride, (out, bits, tlen, err) in zip(levels, strides, res):
        sums = ctx.aggregate(vd, N)
        w_out, w_bits, w_tlen, w_err = ctx.lzmh_encode_f32(sums, stride)
        torch.cuda.synchronize()
        assert (host(err) == 0).all() and (host(w_err) == 0).all()
        assert torch.equal(bits, w_bits) and torch.equal(tlen, w_tlen), N
        nbytes = int((int(w_bits.max()) + 7) // 8)
        assert torch.equal(out[:, :nbytes], w_out[:, :nbytes]), N
        if N == 1:  # +0.0f + v: no "-0.00" anywhere, although the readings hold -0.0f
            text, lens, _ = ctx.csv_write(sums, 2)
            torch.cuda.synchronize()
            assert not any(b"-" in t for t in texts_of(host(text), host(lens)))


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(dca, ctx):
    import torch
    L = dca.library()
    E = dca.ERROR_INVALID_VALUE
    s = ctx._stream()
    v = dev(meter(np.random.default_rng(1), 64, 8))
    text = torch.full((8, 1024), 0xEE, dtype=torch.uint8, device="cuda")
    lens = torch.full((8,), 77, dtype=torch.int64, device="cuda")
    err = torch.full((8,), 77, dtype=torch.int32, device="cuda")
    out = torch.full((8, 2048), 0xEE, dtype=torch.uint8, device="cuda")
    bits = torch.full((8,), 77, dtype=torch.int64, device="cuda")
    p = lambda t: t.data_ptr()  # noqa: E731

    def csv(C_=8, T=64, ld=8, d=2, column=1, sep=44, o=p(text), stride=1024, ln=p(lens), er=p(err), vv=p(v)):
        return L.dega_hip_csv_write_dev(ctx._h, vv, C_, T, ld, d, column, sep, o, stride, ln, er, s)

    assert csv(d=7) == E and csv(column=0) == E and csv(sep=256) == E and csv(sep=-1) == E
    assert csv(o=p(text) + 8) == E and csv(stride=1000) == E and csv(stride=0) == E and csv(stride=2 ** 31) == E
    assert csv(ld=7) == E and csv(o=None) == E and csv(ln=None) == E and csv(er=None) == E and csv(vv=None) == E
    assert csv(column=1025) == E  # more empty columns than a row holds
    assert csv(o=p(v), stride=16) == E  # out overlaps v_tc

    def enc(C_=8, T=64, ld=8, d=2, column=1, sep=44, ts=1024, o=p(out), cap=2048, b=p(bits), tl=p(lens), er=p(err), vv=p(v)):
        return L.dega_hip_lzmh_encode_f32_dev(ctx._h, vv, C_, T, ld, d, column, sep, ts, o, cap, b, tl, er, s)

    assert enc(d=7) == E and enc(column=0) == E and enc(ts=1000) == E and enc(ld=7) == E and enc(cap=2040) == E and enc(cap=32) == E
    assert enc(o=p(out) + 4) == E and enc(o=None) == E and enc(b=None) == E and enc(er=None) == E and enc(vv=None) == E

    def lev(nv=(2, 4), K=2, d=2, column=1, ts=(1024, 1024), outs=None, caps=(1024, 1024), C_=8, ld=8):
        outs = (p(out), p(out) + 8 * 1024) if outs is None else outs
        arr = lambda xs, t: (t * max(1, len(xs)))(*xs)  # noqa: E731
        two = arr((p(bits), p(bits)), C.c_void_p)
        return L.dega_hip_lzmh_encode_levels_f32_dev(ctx._h, p(v), C_, 64, ld, arr(nv, C.c_size_t), K, d, column, 44, arr(ts, C.c_size_t),
                                                     arr(outs, C.c_void_p), arr(caps, C.c_size_t), two, None, arr((p(err), p(err)), C.c_void_p), s)

    assert lev(nv=(2, 0)) == E and lev(nv=(4, 4)) == E and lev(nv=tuple(range(1, 10)), K=9) == E
    assert lev(d=7) == E and lev(column=0) == E and lev(ts=(1024, 1000)) == E and lev(ld=7) == E and lev(caps=(1024, 1000)) == E
    assert lev(outs=(p(out), p(out) + 512)) == E  # two levels' outputs overlap
    assert L.dega_hip_lzmh_encode_levels_f32_dev(ctx._h, p(v), 8, 64, 8, (C.c_size_t * 2)(2, 4), 2, 2, 1, 44, None, None, None, None, None, None, s) == E
    torch.cuda.synchronize()
    for t, fill in ((text, 0xEE), (out, 0xEE), (lens, 77), (err, 77), (bits, 77)):
        assert (t == fill).all()  # nothing was launched
    # K = 0 and C = 0: nothing to do; T = 0: lengths 0
    assert L.dega_hip_lzmh_encode_levels_f32_dev(ctx._h, p(v), 8, 64, 8, None, 0, 2, 1, 44, None, None, None, None, None, None, s) == 0
    assert csv(C_=0) == 0 and enc(C_=0) == 0 and lev(C_=0) == 0
    torch.cuda.synchronize()
    assert (lens == 77).all() and (err == 77).all()
    assert csv(T=0) == 0
    torch.cuda.synchronize()
    assert (lens == 0).all() and (err == 0).all() and (text == 0xEE).all()
    lens.fill_(77)
    err.fill_(77)
    assert enc(T=0) == 0
    torch.cuda.synchronize()
    assert (lens == 0).all() and (err == 0).all() and (bits == 0).all() and (out == 0xEE).all()
