"""GPU tests (-m gpu) of `decode csv` with one channel's text split over lanes (dega_hip_csv_read_split_dev), through the C
ABI and Context.csv_read(split=): the fixture, the block-edge ladder, the fields of 48 characters and more and the rooms too
small of tests/test_csv_read_split_host.py on the device; equality with the unsplit call, result for result; the refusals;
the scratch between the launches on two streams and growing; and the reader in both of the study's chains.  Every
comparison is exact bit patterns, exact counts and exact status.

What is compared against: tests/golden/csv_read.npz (returned by the compiled reference), csv.c:20-42 restated with libc's
strtof (csv_read_common.expected), dega_hip_csv_read_dev, and the sums of tests/golden/aggregate.npz."""
import os
import sys

import numpy as np
import pytest

from __graft_entry__ import load_package

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import csv_read_common as crc  # noqa: E402
import csv_read_split_common as sc  # noqa: E402
from csv_common import GOLDEN, input_series, input_txt  # noqa: E402

pytestmark = pytest.mark.gpu
FILLER = sc.FILLER


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


def launch(ctx, texts, max_T, column=1, sep=",", ld=None, stride=None, split=48, lens=None):
    """the call on the current stream, not waited for: (out [max_T + 2][ld] prefilled with FILLER, count, err) on the device"""
    rows, own = crc.pack(texts, stride)
    lens = own if lens is None else lens
    Cn = len(texts)
    ld = Cn if ld is None else ld
    out = dev(np.full((max_T + 2, ld), FILLER, dtype=np.uint32).view(np.float32))
    return ctx.csv_read(dev(rows), dev(np.asarray(lens).astype(np.int64)), max_T, column, chr(sep) if isinstance(sep, int) else sep, ld=ld, out=out, split=split)


def fetch(result, Cn, max_T):
    """Returns (values uint32 [max_T][ld], count, err); rows at or beyond max_T and the columns beyond the channels hold FILLER
    and must keep it."""
    v = host(result[0]).view(np.uint32)
    assert (v[:, Cn:] == FILLER).all(), "a column beyond the channels was written"
    assert (v[max_T:] == FILLER).all(), "a row at or beyond max_T was written"
    return v[:max_T], host(result[1]), host(result[2])


def read(ctx, texts, max_T, column=1, sep=",", ld=None, stride=None, split=48, lens=None):
    import torch
    result = launch(ctx, texts, max_T, column, sep, ld, stride, split, lens)
    torch.cuda.synchronize()
    return fetch(result, len(texts), max_T)


# ---- the cases of the host tests on the device -------------------------------------------------------------------------------

def test_split_vs_fixture(ctx, fx):
    """every case of csv_read.npz at blocks of 48 bytes: one channel per case, the cases of one (column, separator_char) in one
    call"""
    by_options = {}
    for name in fx.cases():
        by_options.setdefault(fx.options(name), []).append(name)
    values = 0
    for (column, sep), names in by_options.items():
        texts = [fx.text(n) for n in names]
        want = [fx.bits(n) for n in names]
        max_T = max(len(w) for w in want)
        v, count, err = read(ctx, texts, max_T, column, sep, ld=len(texts) + 3, split=48)
        values += crc.check_channels(v, count, err, want, [0] * len(texts), max_T, (column, sep))
        assert (err == 0).all()
    assert values >= 130000


@pytest.mark.parametrize("B", [16, 64])
def test_split_block_edge_ladder_and_long_fields(ctx, B):
    def run(texts, max_T, column, sep, block):
        return read(ctx, texts, max_T, column, sep, ld=len(texts) + 2, split=block)
    assert sc.check_ladder(run, B) > 2500
    assert sc.check_long_fields(run, B) == sc.LONG_FLAGGED


def test_split_room_for_fewer_values_than_there_are(dca, ctx):
    """ERROR_MEMORY with the room needed, exact rows below max_T, nothing beyond them; max_T = 0 counts only, without a v"""
    import torch
    texts, want = sc.room_set()
    for max_T in sc.ROOMS:
        if max_T == 0:
            rows, lens = crc.pack(texts)
            text, ln = dev(rows), dev(lens.astype(np.int64))
            count, err = dev(np.full(70, 77, dtype=np.int64)), dev(np.full(70, 77, dtype=np.int32))
            assert dca.library().dega_hip_csv_read_split_dev(ctx._h, text.data_ptr(), rows.shape[1], ln.data_ptr(), 70, 1, 44, None, 0, 72, count.data_ptr(),
                                                             err.data_ptr(), 32, ctx._stream()) == 0
            torch.cuda.synchronize()
            v, count, err = np.zeros((0, 72), dtype=np.uint32), host(count), host(err)
        else:
            v, count, err = read(ctx, texts, max_T, ld=72, split=32)
        crc.check_channels(v, count, err, want, [0] * 70, max_T, max_T)
        over = sum(1 for w in want if len(w) > max_T)
        assert int((err == crc.ERROR_MEMORY).sum()) == over and int((err != 0).sum()) == over and (over > 0 or max_T == 40)


# ---- equality with the unsplit call ------------------------------------------------------------------------------------------

def test_split_equals_the_unsplit_call(dca, ctx):
    """a mixed batch of 5 channels of up to 5 000 lines -- three classes of fields, an empty channel and one whose len[c]
    exceeds the stride -- through split=None, "auto", 16, 4096 and a block above the stride: the same err and count, and
    the same rows below each channel's count"""
    rng = np.random.default_rng(71)
    fields = [crc.short_one_last(crc.fields_printed(rng, 5000, 2)), crc.short_one_last(crc.fields_digits(rng, 3000)),
              crc.short_one_last(crc.fields_exponents(rng, 4000))]
    texts = [crc.lines_text(fields[0]), crc.lines_text(fields[1]), b"", crc.lines_text(fields[2]), b"1.5\n" * 100]
    rows, lens = crc.pack(texts)
    stride = rows.shape[1]
    lens = lens.copy()
    lens[4] = stride + 1  # built by hand: no text can be that long
    assert dca.csv_read_split_block_bytes(5, stride) % 16 == 0
    got = {}
    for split in (None, "auto", 16, 4096, stride + 160):
        v, count, err = read(ctx, texts, 5000, ld=6, split=split, lens=lens)
        got[split] = (v, count, err)
    v0, count0, err0 = got[None]
    assert err0.tolist() == [0, 0, 0, 0, crc.ERROR_INVALID_VALUE] and count0.tolist() == [5000, 3000, 0, 4000, 0]
    for c, f in ((0, fields[0]), (1, fields[1]), (3, fields[2])):
        assert (v0[: len(f), c] == np.array([crc.strtof_bits(x) for x in f], dtype=np.uint32)).all(), c
    for split, (v, count, err) in got.items():
        assert (err == err0).all() and (count == count0).all(), split
        for c in range(5):
            k = int(count0[c])
            assert (v[:k, c] == v0[:k, c]).all(), (split, c)


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def test_split_refusals_launch_nothing(dca, ctx):
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

    def rd(tx=p(text), stride=1024, ln=p(lens), C_=8, column=1, sep=44, vv=p(v), max_T=64, ld=8, cn=p(count), er=p(err), B=64):
        return L.dega_hip_csv_read_split_dev(ctx._h, tx, stride, ln, C_, column, sep, vv, max_T, ld, cn, er, B, s)

    assert rd(B=8) == E and rd(B=24) == E and rd(B=1) == E and rd(B=1000) == E
    assert rd(ld=7) == E and rd(column=0) == E and rd(tx=p(text) + 8) == E and rd(vv=p(text), max_T=4) == E  # (v_tc overlaps text)
    assert rd(sep=256) == E and rd(stride=1000) == E and rd(stride=2 ** 31) == E and rd(tx=None) == E and rd(ln=None) == E and rd(vv=None) == E
    assert rd(cn=None) == E and rd(er=None) == E and rd(er=p(err) + 2) == E
    torch.cuda.synchronize()
    assert (v == 7.0).all() and (count == 77).all() and (err == 77).all()
    assert rd(C_=0) == 0 and rd(C_=0, B=0) == 0
    torch.cuda.synchronize()
    assert (v == 7.0).all() and (count == 77).all() and (err == 77).all()
    # a block above the stride is one block per channel, and the library's choice is taken for 0: forty 1s are one field
    for B in (1024 + 16, 2 ** 40, 0):
        count.fill_(77)
        assert rd(B=B) == 0
        torch.cuda.synchronize()
        assert (count == 1).all() and (err == 0).all() and (v[0].view(torch.int32) == crc.strtof_bits(b"1" * 40)).all() and (v[1:] == 7.0).all(), B


# ---- the scratch between the launches ------------------------------------------------------------------------------------------

def test_split_two_streams_and_a_growing_scratch(ctx):
    """two calls of different shapes on two streams with no synchronisation between them (the scratch's event orders them on
    the device), then on one stream a small batch followed by a larger one (the scratch grows)"""
    import torch
    rng = np.random.default_rng(72)
    fields = crc.fields_printed(rng, 9000, 2)
    small = crc.deal(fields[:600], 3)
    large = crc.deal(fields[600:], 7)
    fresh = type(ctx)(0)  # its scratch starts empty
    try:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            r1 = launch(fresh, large[0], 1200, ld=8, split=32)
        with torch.cuda.stream(s2):
            r2 = launch(fresh, small[0], 200, ld=4, split=48)
        torch.cuda.synchronize()
        assert crc.check_channels(*fetch(r1, 7, 1200), large[1], [0] * 7, 1200, "stream 1") == 8400
        assert crc.check_channels(*fetch(r2, 3, 200), small[1], [0] * 3, 200, "stream 2") == 600
        with torch.cuda.stream(s1):
            r3 = launch(fresh, small[0], 200, ld=4, split=64)
            huge = crc.deal(fields, 9)
            r4 = launch(fresh, huge[0], 1000, ld=9, split=16)  # more blocks than any call before
        torch.cuda.synchronize()
        assert crc.check_channels(*fetch(r3, 3, 200), small[1], [0] * 3, 200, "small first") == 600
        assert crc.check_channels(*fetch(r4, 9, 1000), huge[1], [0] * 9, 1000, "then larger") == 9000
    finally:
        fresh.close()


# ---- in the chains ---------------------------------------------------------------------------------------------------------------

def test_csv_write_then_split_read_is_the_input(ctx):
    """floats of two-decimal numbers come back bit for bit through their two-decimal text, few long channels"""
    import torch
    Cn, T = 3, 20000
    x = ctx.synth(Cn, T, seed=1234, S=50)
    hundred = torch.full((), 100.0, dtype=torch.float64, device=x.device)
    v = (x.to(torch.float64) / hundred).to(torch.float32)
    text, lens, err = ctx.csv_write(v, 2, stride=T * 10 + 16)
    back, count, rerr = ctx.csv_read(text, lens, T, split="auto")
    torch.cuda.synchronize()
    assert (err == 0).all() and (rerr == 0).all() and (count == T).all()
    assert torch.equal(back.view(torch.int32), v.view(torch.int32))


@pytest.mark.parametrize("split", ["auto", 48])
def test_split_read_of_input_txt_feeds_aggregate(ctx, split):
    """`decode csv # encode aggregate num_values=60`: the split reader's floats and count into aggregate_levels(count=), the
    sums of aggregate.npz that the unsplit chain is held to"""
    import torch
    rows, lens = crc.pack([input_txt()])
    T = input_series().shape[0]
    v, count, err = ctx.csv_read(dev(rows), dev(lens.astype(np.int64)), T, split=split)
    torch.cuda.synchronize()
    assert int(count[0]) == T and int(err[0]) == 0
    assert (host(v).view(np.uint32) == input_series().view(np.uint32)).all()
    (sums,), (n,), aerr = ctx.aggregate_levels(v, [60], count=count)
    torch.cuda.synchronize()
    golden = np.load(os.path.join(GOLDEN, "aggregate.npz"))
    want = golden["series.a"][:, 0]  # the reference's `encode aggregate num_values=60` over its own series
    assert int(aerr[0]) == 0 and int(n[0]) == (T + 59) // 60 == want.size
    assert (host(sums).view(np.uint32)[: want.size, 0] == want.view(np.uint32)).all()
