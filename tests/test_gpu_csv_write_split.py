"""GPU tests (-m gpu) of `encode csv` with one channel's rows split over lanes (dega_hip_csv_write_split_dev), through the C
ABI and Context.csv_write(split=): the fixture, the edge ladder, the digit-count ladder, the counts and the rooms of
tests/test_csv_write_split_host.py on the device; equality with the unsplit calls, result for result; the refusals; the
scratch between the launches on two streams and growing; and the writer in the study's chains.  Every comparison is exact
bytes, exact lengths and exact status; every row is pre-filled with a canary, and every test asserts that the bytes at or
beyond out_len[c], and the whole rows of channels with an error, still hold it.

What is compared against: tests/golden/csv.npz (written by the compiled reference), Python's "%.*f" with glibc's sign of
NaN (csv_common.py_lines, pinned to the reference by tests/test_csv_host.py), dega_hip_csv_write_dev / _var_dev, and the
streams of `meter.plain` in the fixture."""
import os
import sys

import numpy as np
import pytest

from __graft_entry__ import load_package

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import csv_write_split_common as wc  # noqa: E402
from csv_common import DECIMALS, SLACK, Fixture, arrange, py_lines  # noqa: E402

pytestmark = pytest.mark.gpu
SPLITS = (1, 5, "auto")


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


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def launch(ctx, batch, Cn, d, column=1, sep=",", stride=None, split=1, count=None):
    """the call on the current stream, not waited for: (rows [Cn + 1][stride] pre-filled with the canary, lens, err) on the device"""
    import torch
    batch = np.ascontiguousarray(batch, dtype=np.uint32)
    v = dev(batch.view(np.float32))  # (a byte copy: NaN payloads and signs survive)
    out = torch.full((Cn + 1, stride), wc.CANARY, dtype=torch.uint8, device="cuda")
    cnt = None if count is None else dev(np.asarray(count).astype(np.int64))
    text, lens, err = ctx.csv_write(v, d, column, sep, stride=stride, channels=Cn, out=out, count=cnt, split=split)
    return out, lens, err


def fetch(result, Cn):
    out, lens, err = (host(t) for t in result)
    assert (out[Cn:] == wc.CANARY).all(), "a row beyond the channels was written"
    return out[:Cn], lens, err


def runner(ctx, split_of=lambda block_rows: block_rows):
    def run(batch, Cn, d, column, sep, stride, block_rows, count):
        import torch
        result = launch(ctx, batch, Cn, d, column, sep, stride, split_of(block_rows), count)
        torch.cuda.synchronize()
        return fetch(result, Cn)
    return run


# ---- the cases of the host tests on the device -------------------------------------------------------------------------------

@pytest.mark.parametrize("split", SPLITS)
def test_split_vs_fixture(ctx, fx, split):
    """every list of csv.npz at every num_decimal_places; 37 channels, ld = 41; and the lines of 48 characters and more that
    the reference cannot write, against Python"""
    run = runner(ctx)
    n = 0
    for name in fx.lists():
        column, sep = fx.options(name)
        for d in DECIMALS:
            bits, lines = fx.lines(name, d)
            batch, want = arrange(bits, lines, 37, 41, py_lines([0], d, column, sep)[0])
            stride = wc.stride_for(want)
            rows, lens, err = run(batch, 37, d, column, sep, stride, split, None)
            assert wc.check(rows, lens, err, want, stride, (name, d, split)) == (37, 0)
            n += len(lines)
    assert n >= 20000
    bits = np.concatenate([fx.left_out(name, 6) for name in ("edge", "binades")])
    assert bits.size > 0 and all(len(s) >= 48 for s in py_lines(bits, 6))
    batch, want = arrange(bits, py_lines(bits, 6), 3, 4, b"0.000000\n")
    stride = wc.stride_for(want)
    rows, lens, err = run(batch, 3, 6, 1, ",", stride, split, None)
    assert wc.check(rows, lens, err, want, stride, ("long lines", split)) == (3, 0)


@pytest.mark.parametrize("split", SPLITS + (2, 3, 7))
def test_split_edge_ladder(ctx, split):
    assert wc.check_ladder(runner(ctx), split) > 400


@pytest.mark.parametrize("split", SPLITS)
def test_split_digit_count_ladder(ctx, split):
    assert wc.check_digit_ladder(runner(ctx), split) > 3 * 500


def test_split_counts_separators_and_room(ctx, fx):
    run = runner(ctx)
    for block_rows in (wc.COUNT_BLOCK_ROWS, 1, 100, "auto"):
        wc.check_counts(run, block_rows)
    bits, _ = fx.lines("binades", 2)
    for column, sep in ((12, ";"), (3, ",")):
        lines = py_lines(bits[:600], 2, column, sep)
        batch, want = arrange(bits[:600], lines, 5, 7, py_lines([0], 2, column, sep)[0])
        stride = wc.stride_for(want)
        for split in (1, 7, "auto"):
            rows, lens, err = run(batch, 5, 2, column, sep, stride, split, None)
            assert wc.check(rows, lens, err, want, stride, (column, split)) == (5, 0)
    bits, lines = fx.lines("binades", 6)
    batch, want = arrange(bits, lines, 37, 41, b"0.000000\n")
    sizes = sorted(len(w) for w in want)
    for stride in ((sizes[18] + SLACK + 15) // 16 * 16, 16, (sizes[-1] + SLACK - 1) // 16 * 16):
        for split in (1, 6, "auto"):
            rows, lens, err = run(batch, 37, 6, 1, ",", stride, split, None)
            fit, over = wc.check(rows, lens, err, want, stride, (stride, split))
            assert over >= 1 and (fit >= 1 or stride == 16)
    T, total = wc.room_boundary(bits, lines)
    text = b"".join(lines[:T])
    for split in (1, 3, "auto"):
        rows, lens, err = run(bits[:T].reshape(T, 1), 1, 6, 1, ",", total + SLACK, split, None)
        assert wc.check(rows, lens, err, [text], total + SLACK, T) == (1, 0)
        rows, lens, err = run(bits[:T].reshape(T, 1), 1, 6, 1, ",", total, split, None)
        assert wc.check(rows, lens, err, [text], total, T) == (0, 1)


def test_split_batch_shapes(ctx, fx):
    run = runner(ctx)
    bits, lines = fx.lines("binades", 2)
    bits, lines = np.resize(bits, 300 * 17), (lines * (300 * 17 // len(lines) + 1))[: 300 * 17]  # (the list once and again)
    for Cn in (1, 5, 37, 64, 257, 300):
        batch, want = arrange(bits[: Cn * 17], lines[: Cn * 17], Cn, Cn + 3, b"0.00\n")
        stride = wc.stride_for(want)
        for split in (1, 5, 40, "auto"):
            rows, lens, err = run(batch, Cn, 2, 1, ",", stride, split, None)
            assert wc.check(rows, lens, err, want, stride, (Cn, split)) == (Cn, 0)
    for T in (1, 15, 16, 17, 33):
        batch, want = arrange(bits[: 5 * T], lines[: 5 * T], 5, 8, b"0.00\n")
        stride = wc.stride_for(want)
        for split in (1, 2, 4, 16, T + 3):
            rows, lens, err = run(batch, 5, 2, 1, ",", stride, split, None)
            assert wc.check(rows, lens, err, want, stride, (T, split)) == (5, 0)


# ---- equality with the unsplit calls -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("counted", [False, True])
def test_split_equals_the_unsplit_call(dca, ctx, counted):
    """a mixed batch of 5 channels x 5 000 rows -- two-decimal readings, random bit patterns, large integers, small values and
    one channel that outgrows the stride -- through split=None, "auto", 1, 16, 4096 and a value above T: the same err and
    len everywhere and the same bytes below len; with and without count (one count above T)"""
    import torch
    rng = np.random.default_rng(81)
    T = 5000
    batch = np.full((T, 6), 0x7FC12345, dtype=np.uint32)
    batch[:, 0] = wc.f32_bits(np.round(rng.uniform(0.0, 70000.0, T) * 100.0) / 100.0)
    batch[:, 1] = rng.integers(0, 2 ** 32, T, dtype=np.uint64).astype(np.uint32)
    batch[:, 2] = wc.f32_bits(rng.uniform(-1.0e12, 1.0e12, T))
    batch[:, 3] = wc.f32_bits(rng.uniform(-1.0, 1.0, T))
    batch[:, 4] = wc.f32_bits(-3.0e38 * rng.uniform(0.5, 1.0, T))  # 42 bytes a line: this one outgrows the stride
    count = [T, 4999, 0, 2500, T + 1] if counted else None
    stride = (T * 30 + 16 + 15) // 16 * 16
    assert 1 <= dca.csv_write_split_block_rows(5, T) <= T
    got = {}
    for split in (None, "auto", 1, 16, 4096, T + 7):
        result = launch(ctx, batch, 5, 2, stride=stride, split=split, count=count)
        torch.cuda.synchronize()
        got[split] = fetch(result, 5)
    rows0, lens0, err0 = got[None]
    assert err0.tolist() == ([0, 0, 0, 0, wc.ERROR_INVALID_VALUE] if counted else [0, 0, 0, 0, wc.ERROR_MEMORY]) and int(lens0[4]) == 0
    for c in range(4):
        n = T if count is None else count[c]
        assert rows0[c, : int(lens0[c])].tobytes() == b"".join(py_lines(batch[:n, c], 2)), c
    for split, (rows, lens, err) in got.items():
        assert (err == err0).all() and (lens == lens0).all(), split
        for c in range(5):
            n = int(lens0[c])
            assert (rows[c, :n] == rows0[c, :n]).all(), (split, c)
            if split is not None:
                assert (rows[c, n:] == wc.CANARY).all(), (split, c)


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def test_split_refusals_launch_nothing(dca, ctx):
    import torch
    L = dca.library()
    E = dca.ERROR_INVALID_VALUE
    s = ctx._stream()
    v = torch.full((64, 8), 1.5, dtype=torch.float32, device="cuda")
    text = torch.full((8, 1024), wc.CANARY, dtype=torch.uint8, device="cuda")
    lens = torch.full((8,), 77, dtype=torch.int64, device="cuda")
    err = torch.full((8,), 77, dtype=torch.int32, device="cuda")
    count = torch.full((8,), 64, dtype=torch.int64, device="cuda")
    p = lambda t: t.data_ptr()  # noqa: E731

    def wr(vv=p(v), C_=8, T=64, ld=8, cn=None, d=2, column=1, sep=44, tx=p(text), stride=1024, ln=p(lens), er=p(err), R=4):
        return L.dega_hip_csv_write_split_dev(ctx._h, vv, C_, T, ld, cn, d, column, sep, tx, stride, ln, er, R, s)

    assert wr(d=7) == E and wr(column=0) == E and wr(sep=256) == E and wr(sep=-1) == E and wr(ld=7) == E
    assert wr(stride=1000) == E and wr(stride=0) == E and wr(stride=2 ** 31) == E and wr(column=1025) == E
    assert wr(tx=p(text) + 8) == E and wr(tx=None) == E and wr(ln=None) == E and wr(er=None) == E and wr(er=p(err) + 2) == E and wr(ln=p(lens) + 4) == E
    assert wr(vv=None) == E and wr(vv=p(text), T=4) == E  # (out overlaps v_tc)
    assert wr(cn=p(count) + 4) == E and wr(cn=p(count), T=2 ** 32) == E
    assert wr(T=2 ** 33, R=1) == E and wr(T=2 ** 32, R=0) == E  # (more than 2^32 - 1 blocks; no rule for such a T)
    torch.cuda.synchronize()
    assert (text == wc.CANARY).all() and (lens == 77).all() and (err == 77).all()
    assert wr(C_=0) == 0 and wr(C_=0, R=0) == 0
    torch.cuda.synchronize()
    assert (text == wc.CANARY).all() and (lens == 77).all() and (err == 77).all()
    # T = 0: lengths 0, no text; with counts, count[c] > 0 is INVALID_VALUE
    assert wr(T=0, vv=None) == 0
    torch.cuda.synchronize()
    assert (text == wc.CANARY).all() and (lens == 0).all() and (err == 0).all()
    lens.fill_(77)
    count[3] = 0
    assert wr(T=0, vv=None, cn=p(count)) == 0
    torch.cuda.synchronize()
    assert (text == wc.CANARY).all() and (lens == 0).all() and err.tolist() == [E, E, E, 0, E, E, E, E]
    count.fill_(64)
    # any block_rows from 1 on is legal, one at or above T is one block per channel, 0 is the library's choice
    for R in (1, 3, 64, 65, 2 ** 40, 0):
        text.fill_(wc.CANARY)
        lens.fill_(77)
        assert wr(R=R) == 0 and wr(R=R, cn=p(count)) == 0
        torch.cuda.synchronize()
        assert (lens == 64 * 5).all() and (err == 0).all(), R
        assert bytes(host(text[3, :320])) == b"1.50\n" * 64 and (text[:, 320:] == wc.CANARY).all(), R


# ---- the scratch between the launches ------------------------------------------------------------------------------------------

def test_split_two_streams_and_a_growing_scratch(ctx, fx):
    """two calls of different shapes on two streams with no synchronisation between them (the scratch's event orders them on
    the device), then on one stream a small batch followed by a larger one (the scratch grows)"""
    import torch
    bits, lines = fx.lines("binades", 2)
    bits, lines = np.resize(bits, 9000), (lines * (9000 // len(lines) + 1))[:9000]  # (the list once and again)
    small = arrange(bits[:600], lines[:600], 3, 4, b"0.00\n")
    large = arrange(bits[600:9000], lines[600:9000], 7, 8, b"0.00\n")
    huge = arrange(bits[:9000], lines[:9000], 9, 9, b"0.00\n")
    strides = [wc.stride_for(x[1]) for x in (small, large, huge)]
    fresh = type(ctx)(0)  # its scratch starts empty
    try:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            r1 = launch(fresh, large[0], 7, 2, stride=strides[1], split=2)
        with torch.cuda.stream(s2):
            r2 = launch(fresh, small[0], 3, 2, stride=strides[0], split=3)
        torch.cuda.synchronize()
        assert wc.check(*fetch(r1, 7), large[1], strides[1], "stream 1") == (7, 0)
        assert wc.check(*fetch(r2, 3), small[1], strides[0], "stream 2") == (3, 0)
        with torch.cuda.stream(s1):
            r3 = launch(fresh, small[0], 3, 2, stride=strides[0], split=5)
            r4 = launch(fresh, huge[0], 9, 2, stride=strides[2], split=1)  # more blocks than any call before
        torch.cuda.synchronize()
        assert wc.check(*fetch(r3, 3), small[1], strides[0], "small first") == (3, 0)
        assert wc.check(*fetch(r4, 9), huge[1], strides[2], "then larger") == (9, 0)
    finally:
        fresh.close()


# ---- in the chains ---------------------------------------------------------------------------------------------------------------

def test_split_write_then_split_read_is_the_input(ctx):
    """floats of two-decimal numbers come back bit for bit through their two-decimal text, few long channels, both halves split"""
    import torch
    Cn, T = 3, 20000
    x = ctx.synth(Cn, T, seed=1234, S=50)
    hundred = torch.full((), 100.0, dtype=torch.float64, device=x.device)
    v = (x.to(torch.float64) / hundred).to(torch.float32)
    stride = T * 10 + 16
    out = torch.full((Cn, stride), wc.CANARY, dtype=torch.uint8, device="cuda")
    text, lens, err = ctx.csv_write(v, 2, stride=stride, out=out, split="auto")
    text0, lens0, err0 = ctx.csv_write(v, 2, stride=stride)
    back, count, rerr = ctx.csv_read(text, lens, T, split="auto")
    torch.cuda.synchronize()
    assert (err == 0).all() and (rerr == 0).all() and (count == T).all() and torch.equal(lens, lens0)
    assert torch.equal(back.view(torch.int32), v.view(torch.int32))
    for c in range(Cn):
        n = int(lens[c])
        assert torch.equal(text[c, :n], text0[c, :n]) and (text[c, n:] == wc.CANARY).all()


@pytest.mark.parametrize("split", ["auto", 7])
def test_split_text_of_the_meter_feeds_lzmh(ctx, fx, split):
    """`encode csv # encode lzmh`: the split writer's text of meter.v through lzmh_encode gives the streams of meter.plain"""
    import torch
    v = fx.meter()
    texts, streams, bits = fx.chain("meter.plain")
    Cn = v.shape[1]
    stride = 420 * 16
    rows, lens, err = fetch(launch(ctx, v.view(np.uint32), Cn, 2, stride=stride, split=split), Cn)
    assert wc.check(rows, lens, err, texts, stride, "meter.plain") == (Cn, 0)
    out, obits, oerr = ctx.lzmh_encode(dev(rows), dev(lens.astype(np.int64)))
    torch.cuda.synchronize()
    out, obits = host(out), host(obits)
    assert (host(oerr) == 0).all()
    for c, (s, b) in enumerate(zip(streams, bits)):
        assert int(obits[c]) == b, (c, int(obits[c]), b)
        assert out[c, : len(s)].tobytes() == s, c
