"""GPU tests (-m gpu) of ragged batches of integer samples and of counts through the host jobs: the counted device entries
(Context.encode(count=), dega_hip_encode64_var_dev, encode_segments(count=)) on the steered input of
tests/ragged_int_common.py, and encode_job(count=) on a Context and on a Group -- one chunk, every sample type and both
layouts, pageable and pinned; then chunks and bands together at shape A of tests/bands_chunks_common.py.

Expected streams: the oracle's chain on each channel's own first count[c] samples (ragged_int_common.expected), for float32
jobs tests/golden/ragged.npz, the compiled reference.  Every channel is compared; there is no tolerance anywhere."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from __graft_entry__ import load_package

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bands_chunks_common as bc  # noqa: E402
import ragged_int_common as ri  # noqa: E402
from ragged_common import CASES, FACTOR, SETS, Fixture, poisoned, same_streams  # noqa: E402

pytestmark = pytest.mark.gpu

T, CN = ri.T, ri.C
CUTS = [0, 1, 8, 9, 64, 200, T]
SENTINEL = 0x5C


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


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.dtype(">i4"):
        a = a.view(np.int32)  # the bytes as they lie
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


def host(*tensors):
    import torch
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in tensors)


def padded(x, ld):
    """the rows of x in an array of pitch ld, the columns behind them holding all ones"""
    wide = np.full((x.shape[0], ld), -1, dtype=x.dtype)
    wide[:, : x.shape[1]] = x
    return wide


def encode64_var(dca, ctx, xd, Cn, count_d, ad, vs):
    import torch
    rows, ld = xd.shape
    cap = dca.library().dega_hip_worst_case_bytes64(rows)
    out = torch.zeros((Cn, cap), dtype=torch.uint8, device=xd.device)
    bits = torch.zeros(Cn, dtype=torch.int64, device=xd.device)
    err = torch.zeros(Cn, dtype=torch.int32, device=xd.device)
    ret = dca.library().dega_hip_encode64_var_dev(ctx._h, xd.data_ptr(), Cn, rows, ld, count_d.data_ptr(), ad, vs, out.data_ptr(), cap, bits.data_ptr(),
                                                  err.data_ptr(), ctx._stream())
    ctx._check(ret, "dega_hip_encode64_var_dev")
    return out, bits, err


def encode_device(dca, ctx, kind, x, count, ld):
    vs, ad, be, wide = ri.KINDS[kind]
    xd, cd = dev(padded(x, ld)), dev(count)
    if wide:
        return encode64_var(dca, ctx, xd, CN, cd, ad, vs)
    return ctx.encode(xd, adaptive=ad, valuesize=vs, count=cd, channels=CN, samples=dca.SAMPLES_BE32 if be else dca.SAMPLES_I32)[:3]


def decode_var(dca, ctx, kind, out, bits, err):
    """(samples [T, C], counts, err) of the library's variable-count decoder on the channels the encoder accepted"""
    import torch
    vs, ad, _, wide = ri.KINDS[kind]
    Cn, cap = out.shape
    x = torch.zeros((T, Cn), dtype=torch.int64 if wide else torch.int32, device=out.device)
    counts = torch.zeros(Cn, dtype=torch.int64, device=out.device)
    derr = torch.zeros(Cn, dtype=torch.int32, device=out.device)
    b = torch.where(err == 0, bits, torch.zeros_like(bits))
    fn = dca.library().dega_hip_decode64_var_dev if wide else dca.library().dega_hip_decode_var_dev
    ret = fn(ctx._h, out.data_ptr(), cap, b.data_ptr(), Cn, T, Cn, ad, vs, x.data_ptr(), counts.data_ptr(), derr.data_ptr(), ctx._stream())
    ctx._check(ret, "decode var")
    return x, counts, derr


# ---- 1. the device entries --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", list(ri.KINDS))
@pytest.mark.parametrize("arrangement", ["full", "short"])
def test_device_entries_on_the_steered_input(dca, ctx, kind, arrangement):
    vs, ad, be, wide = ri.KINDS[kind]
    count = ri.counts(arrangement)
    vals, x = ri.steered(kind, count)
    want = ri.expected(kind, vals, count, arrangement)
    for ld in (136, 135) if kind in ("i32", "be32", "i64") else (136,):  # rows of 16-byte pieces, and rows fetched dword by dword
        out, bits, err = encode_device(dca, ctx, kind, x, count, ld)
        got = host(out, bits, err)
        assert ri.mismatch(want, *got) == "", (kind, ld)
    # and back: the counts and each channel's first count[c] samples
    y, counts, derr = host(*decode_var(dca, ctx, kind, out, bits, err))
    ok = got[2] == 0
    assert ok.sum() == CN - 1 and (derr[ok] == 0).all() and (counts[ok] == count.astype(np.int64)[ok]).all(), kind
    mask = np.uint64((1 << vs) - 1)
    live = (np.arange(T)[:, None] < count.astype(np.int64)[None, :]) & ok[None, :]
    seen = y.astype(np.int64).view(np.uint64) & mask
    assert (seen[live] == vals[live]).all(), kind


# ---- 2. counts above T, and what is refused ---------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["i32", "vs16", "i64"])
def test_counts_above_T(dca, ctx, kind):
    count = ri.counts("full")
    vals, x = ri.steered(kind, count)
    count[5], count[70], count[130] = T + 1, 1 << 40, T + 1
    want = ri.expected(kind, vals, count)
    got = host(*encode_device(dca, ctx, kind, x, count, 136))
    assert ri.mismatch(want, *got, count, T) == "", kind
    assert all(int(got[2][c]) == dca.ERROR_INVALID_VALUE and int(got[1][c]) == 0 for c in (5, 70, 130))


def test_refusals_launch_nothing(dca, ctx):
    import torch
    L, E = dca.library(), dca.ERROR_INVALID_VALUE
    count = ri.counts("full")
    _, x = ri.steered("i32", count)
    _, x64 = ri.steered("i64", count)
    xd, x64d = dev(x), dev(x64)
    cd = dev(np.concatenate([count, count[:1]]))
    cap = dca.worst_case_bytes(T)
    out = torch.full((CN, cap), SENTINEL, dtype=torch.uint8, device=xd.device)
    bits = torch.full((CN,), -7, dtype=torch.int64, device=xd.device)
    err = torch.full((CN,), 77, dtype=torch.int32, device=xd.device)
    state = torch.zeros(L.dega_hip_encode_state_bytes(CN), dtype=torch.uint8, device=xd.device)
    o, b, e, s = out.data_ptr(), bits.data_ptr(), err.data_ptr(), ctx._stream()
    I32 = dca.SAMPLES_I32
    for bad_count in (None, cd.data_ptr() + 4):
        assert L.dega_hip_encode_var_dev(ctx._h, xd.data_ptr(), CN, T, CN, bad_count, 1, 32, I32, o, cap, b, e, s) == E
        assert L.dega_hip_encode64_var_dev(ctx._h, x64d.data_ptr(), CN, T, CN, bad_count, 1, 40, o, cap, b, e, s) == E
        assert L.dega_hip_encode_segment_var_dev(ctx._h, xd.data_ptr(), CN, T, CN, bad_count, 0, T, 1, 32, o, cap, b, e, state.data_ptr(), 0, s) == E
    big = (1 << 25) + 1
    assert L.dega_hip_encode_var_dev(ctx._h, xd.data_ptr(), CN, big, CN, cd.data_ptr(), 1, 32, I32, o, cap, b, e, s) == E
    assert L.dega_hip_encode64_var_dev(ctx._h, x64d.data_ptr(), CN, big, CN, cd.data_ptr(), 1, 40, o, cap, b, e, s) == E
    assert L.dega_hip_encode_var_dev(ctx._h, xd.data_ptr(), CN, T, CN, cd.data_ptr(), 1, 32, dca.SAMPLES_F32, o, cap, b, e, s) == E
    assert L.dega_hip_encode_var_dev(ctx._h, xd.data_ptr(), CN, T, CN, cd.data_ptr(), 1, 33, I32, o, cap, b, e, s) == E
    assert L.dega_hip_encode64_var_dev(ctx._h, x64d.data_ptr(), CN, T, CN, cd.data_ptr(), 1, 32, o, cap, b, e, s) == E
    # the counted segment launch: row0 + T_seg <= T_total <= 2^25
    for row0, T_seg, T_total in ((T - 7, 8, T), (T + 1, 0, T), (0, 8, 7), (0, 8, big)):
        assert L.dega_hip_encode_segment_var_dev(ctx._h, xd.data_ptr(), CN, T_seg, CN, cd.data_ptr(), row0, T_total, 1, 32, o, cap, b, e, state.data_ptr(), 2,
                                                 s) == E, (row0, T_seg, T_total)
    got = host(out, bits, err, state)
    assert (got[0] == SENTINEL).all() and (got[1] == -7).all() and (got[2] == 77).all() and (got[3] == 0).all()
    # C = 0 is nothing to do, whatever the count; C != 0 with T = 0 still launches: the counts decide
    assert L.dega_hip_encode_var_dev(ctx._h, xd.data_ptr(), 0, T, CN, None, 1, 32, I32, o, cap, b, e, s) == 0
    zero = torch.zeros(CN, dtype=torch.int64, device=xd.device)
    zero[3] = 1
    assert L.dega_hip_encode_var_dev(ctx._h, xd.data_ptr(), CN, 0, CN, zero.data_ptr(), 1, 32, I32, o, cap, b, e, s) == 0
    got = host(bits, err)
    empty = ri.oracle_channel(np.zeros(0, dtype=np.uint64), 32, 1)
    assert empty[0] == 0 and int(got[1][3]) == E and int(got[0][3]) == 0
    assert all(int(got[0][c]) == empty[2] and int(got[1][c]) == 0 for c in range(CN) if c != 3)


# ---- 3. segments on the device ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["i32", "i32_static", "vs16", "vs7"])
def test_counted_segments_equal_the_single_call(dca, ctx, kind):
    vs, ad, _, _ = ri.KINDS[kind]
    count = ri.counts("short")
    for c, n in ((1, 8), (2, 9), (6, 64), (7, 63), (8, 65), (66, 200), (67, 1), (129, 9), (131, 201)):
        count[c] = n
    count[133] = T + 1
    vals, x = ri.steered(kind, count)
    want = ri.expected(kind, vals, count)
    xd, cd = dev(x), dev(count)
    single = host(*ctx.encode(xd, adaptive=ad, valuesize=vs, count=cd)[:3])
    assert ri.mismatch(want, *single, count, T) == "", kind
    for cuts in (CUTS, CUTS + [T]):
        got = host(*ctx.encode_segments(xd, cuts, adaptive=ad, valuesize=vs, count=cd))
        assert ri.mismatch(want, *got, count, T) == "", (kind, cuts)
        assert (got[1] == single[1]).all() and (got[2] == single[2]).all(), (kind, cuts)


# ---- 4. host jobs, one chunk ------------------------------------------------------------------------------------------------

def channel_major(x, stride, fill):
    """[C, stride]: one series per row, `fill` behind its T values"""
    a = np.full((x.shape[1], stride), fill, dtype=x.dtype)
    a[:, : x.shape[0]] = x.T
    return a


def job_kwargs(dca, kind):
    vs, ad, be, wide = ri.KINDS[kind]
    return dict(adaptive=ad, valuesize=vs, samples=dca.SAMPLES_I64 if wide else (dca.SAMPLES_BE32 if be else dca.SAMPLES_I32))


@pytest.mark.parametrize("kind", ["i32", "be32", "i64", "vs7"])
def test_host_job_one_chunk_integer_samples(dca, ctx, kind):
    count = ri.counts("short")
    vals, x = ri.steered(kind, count)
    want = ri.expected(kind, vals, count, "short")
    kw = job_kwargs(dca, kind)
    first = None
    pinned = dca.PinnedArray(x.shape, x.dtype)
    try:
        pinned.array[...] = x
        arrays = (("pageable", x, {}), ("pinned", pinned.array, {}),
                  ("channel", channel_major(x, T + 5, -1), dict(layout="channel", T=T)))
        for tag, a, more in arrays:
            packed, offsets, bits, err = ctx.encode_job(a, count=count, **kw, **more)
            assert ri.mismatch(want, (packed, offsets), bits, err) == "", (kind, tag)
            assert int(offsets[0]) == 0 and int(offsets[CN]) == packed.size, (kind, tag)
            if first is None:
                first = (packed.copy(), offsets.copy(), bits.copy(), err.copy())
            assert packed.tobytes() == first[0].tobytes() and (offsets == first[1]).all() and (bits == first[2]).all() and (err == first[3]).all(), (kind, tag)
    finally:
        pinned.free()
    # decode_job(var=True) -> encode_job(count=counts): the packed bytes and offsets again, exactly.  (The broken row of the
    # honest channel lies beyond a count of 50, so every channel has a stream.)
    count = np.array(count)
    count[ri.HONEST] = 50
    packed, offsets, bits, err = ctx.encode_job(x, count=count, **kw)
    assert (err == 0).all(), kind
    back, counts, derr = ctx.decode_job(packed, offsets, bits, T, var=True, **kw)
    assert counts.dtype == np.uint64 and (derr == 0).all() and (counts == count).all(), kind
    again = ctx.encode_job(back, count=counts, **kw)
    back_ct, counts_ct, _ = ctx.decode_job(packed, offsets, bits, T, var=True, layout="channel", **kw)
    again_ct = ctx.encode_job(back_ct, count=counts_ct, layout="channel", **kw)
    for got in (again, again_ct):
        for g, w in zip(got, (packed, offsets, bits, err)):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), kind


@pytest.mark.parametrize("case", CASES)
def test_host_job_one_chunk_float_samples_against_the_compiled_reference(dca, ctx, case):
    fx = Fixture()
    count = fx.count(case).astype(np.uint64)
    v = poisoned(fx.v(case), count)
    rows, Cn = v.shape
    pinned = dca.PinnedArray(v.shape, v.dtype)
    try:
        pinned.array[...] = v
        for vs, ad in SETS:
            want = fx.dega(case, 1, vs, ad)
            kw = dict(adaptive=ad, valuesize=vs, samples=dca.SAMPLES_F32, factor=FACTOR)
            for tag, a, more in (("pageable", v, {}), ("pinned", pinned.array, {}),
                                 ("channel", channel_major(v, rows + 3, np.float32(np.nan)), dict(layout="channel", T=rows))):
                packed, offsets, bits, err = ctx.encode_job(a, count=count, **kw, **more)
                slabs = np.zeros((Cn, want[0].shape[1]), dtype=np.uint8)
                for c in range(Cn):
                    n = int(offsets[c + 1] - offsets[c])
                    assert n == (int(bits[c]) + 7) // 8 or int(err[c]) != 0, (case, vs, ad, tag, c)
                    slabs[c, : min(n, slabs.shape[1])] = packed[int(offsets[c]):int(offsets[c]) + min(n, slabs.shape[1])]
                assert same_streams(slabs, bits, err, *want) == "", (case, vs, ad, tag)
    finally:
        pinned.free()


# ---- 5. host jobs, chunks and bands together --------------------------------------------------------------------------------

CA, TA = bc.CA, bc.TA
EDGE_COUNTS = (0, 1, 31, 32, 33, 150, TA)
INSIDE, BEYOND = bc.BROKEN[0], bc.BROKEN[1]  # broken from row 150 on: inside a count of 180, beyond one of 150


def counts_a():
    rng = np.random.default_rng(1760)
    count = rng.integers(0, TA + 1, CA).astype(np.uint64)
    for c0 in range(0, CA, bc.CHUNK):
        c1 = min(CA, c0 + bc.CHUNK)
        count[c0:c0 + len(EDGE_COUNTS)] = EDGE_COUNTS
        count[c1 - len(EDGE_COUNTS):c1] = EDGE_COUNTS
    count[list(bc.NOISY)] = TA
    count[INSIDE], count[BEYOND], count[bc.BROKEN[2]] = 180, bc.BROKEN_FROM, 100
    return count


@pytest.fixture(scope="module")
def shape_a(dca):
    """shape A's steered batch with counts, rows at or beyond a count holding -1, and the oracle on every channel; computed once"""
    out = {}
    count = counts_a()
    dead = np.arange(TA)[:, None] >= count.astype(np.int64)[None, :]
    for kind, rkind in (("i32", "i32"), ("i64", "i64")):
        x, kw = bc.input_a(kind, dca)
        vs = kw["valuesize"]
        full = np.array(x)
        x = np.array(x)
        x[dead] = -1
        vals = full.astype(np.int64).view(np.uint64) & np.uint64((1 << vs) - 1)
        want = ri.expected(rkind, vals, count)
        bad = [c for c, w in enumerate(want) if w[0] != 0]
        assert bad == [INSIDE], (kind, bad[:8])
        for a in (x, full, count):
            a.flags.writeable = False
        out[kind] = (x, full, kw, count, want)
    return out


def set_knobs(monkeypatch):
    for k, v in bc.knobs(bc.CHUNKS_A).items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("kind", ["i32", "i64"])
def test_host_job_chunks_and_bands_on_a_context(dca, ctx, shape_a, monkeypatch, kind):
    x, _, kw, count, want = shape_a[kind]
    set_knobs(monkeypatch)
    packed, offsets, bits, err = ctx.encode_job(x, count=np.array(count), **kw)
    assert ri.mismatch(want, (packed, offsets), bits, err) == "", kind
    assert int(offsets[CA]) == packed.size
    for c in bc.NOISY:  # the stream outgrew the usual slab: the chunk was redone, with its counts
        assert int(offsets[c + 1] - offsets[c]) > 4 * TA + 64, (kind, c)


@pytest.mark.parametrize("kind", ["i32", "i64"])
def test_host_job_chunks_and_bands_on_a_group(dca, shape_a, monkeypatch, kind):
    import torch
    x, _, kw, count, want = shape_a[kind]
    set_knobs(monkeypatch)
    members = [[0, 0]] + ([[0, 1]] if torch.cuda.device_count() >= 2 else [])
    for devices in members:
        grp = dca.Group(devices)
        try:
            packed, offsets, bits, err = grp.encode_job(x, count=np.array(count), **kw)
        finally:
            grp.close()
        assert ri.mismatch(want, (packed, offsets), bits, err) == "", (kind, devices)
        assert int(offsets[CA]) == packed.size


# ---- 6. the uniform paths are untouched -------------------------------------------------------------------------------------

def test_full_counts_are_the_uniform_job(dca, ctx, shape_a, monkeypatch):
    _, full, kw, _, _ = shape_a["i32"]
    every = np.full(CA, TA, dtype=np.uint64)
    for knobs in (False, True):
        if knobs:
            set_knobs(monkeypatch)
        uniform = ctx.encode_job(full, **kw)
        counted = ctx.encode_job(full, count=every, **kw)
        for g, w in zip(counted, uniform):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), knobs
    count = ri.counts("full")
    for kind in ("i32", "be32", "i64"):
        vals, x = ri.steered(kind, count)
        kwk = job_kwargs(dca, kind)
        uniform = ctx.encode_job(x, **kwk)
        counted = ctx.encode_job(x, count=np.full(CN, T, dtype=np.uint64), **kwk)
        for g, w in zip(counted, uniform):
            assert g.tobytes() == w.tobytes(), kind
