"""GPU tests (-m gpu) of A-XDR through the C ABI: the cases of tests/axdr_common.py over the whole product of value sizes,
rows and channels, the chains around them (levels, compaction, the host forms) and index width.  Everything is compared
exactly -- the float entry and exit with the oracle's `normalize` stage, the integer entries with the plain numpy pack that
tests/test_axdr_host.py holds to the oracle and the fixture -- and no channel is excused.  The emulator runs a selection of
the same cases first (tests/test_axdr_host.py), where a wrong offset is harmless."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from __graft_entry__ import load_package

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import axdr_common as ax  # noqa: E402
import float_edges_common as fe  # noqa: E402
from agg_common import meter  # noqa: E402
from oracle import orc  # noqa: E402

pytestmark = pytest.mark.gpu

LEVELS = (1, 4, 15, 96)


class Handle:
    def __init__(self, raw, view, initial):
        self.raw, self.view, self.initial = raw, view, initial


class Device:
    """the backend of axdr_common over the library: torch tensors on the GPU, the device-resident entry points"""

    def __init__(self, dca, ctx):
        import torch
        self.torch, self.dca, self.ctx, self.L = torch, dca, ctx, dca.library()

    def buf(self, array, offset=0):
        data = np.ascontiguousarray(array).reshape(-1).view(np.uint8)
        raw = self.torch.zeros(data.size + offset + 16, dtype=self.torch.uint8, device="cuda")  # (the allocator's bases are 16-byte aligned, and more)
        assert raw.data_ptr() % 16 == 0
        view = raw[offset:offset + data.size]
        view.copy_(self.torch.from_numpy(data.copy()))
        return Handle(raw, view, data.tobytes())

    @staticmethod
    def ptr(h):
        return h.view.data_ptr()

    def get(self, h):
        self.torch.cuda.synchronize()
        return h.view.cpu().numpy()

    @staticmethod
    def initial(h):
        return h.initial

    def pack(self, x, kind, Cn, T, ld, count, factor, vs, out, cap, bits, err, wide, gx_max):
        return self.L.dega_hip_axdr_encode_dev(self.ctx._h, x, ax.SAMPLES[kind], Cn, T, ld, count or None, factor, vs, out, cap, bits, err, self.ctx._stream())

    def unpack(self, s, cap, bits, Cn, max_T, ld, factor, vs, kind, x, count, err, wide, gx_max):
        return self.L.dega_hip_axdr_decode_dev(self.ctx._h, s, cap, bits, Cn, max_T, ld, factor, vs, ax.SAMPLES[kind], x, count, err, self.ctx._stream())


@pytest.fixture(scope="module")
def dca():
    return load_package()


@pytest.fixture(scope="module")
def ctx(dca):
    c = dca.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def B(dca, ctx):
    return Device(dca, ctx)


SHAPES = [(T, Cn) for T in ax.ROWS for Cn in ax.CHANNELS]


# ---- the whole product -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("vs", ax.SIZES)
def test_pack_integers(B, vs):
    """every T and every C at every value size: fields over the full range, junk above them; ld = C and C + 7, the rows' base one
    element off, cap no multiple of 16 with the slabs 4 bytes off"""
    for k, (T, Cn) in enumerate(SHAPES):
        ax.case_pack_int(B, vs, Cn, T, pitch_case=k % 2)
    ax.case_pack_int(B, vs, 132, 300)  # (rows on the 16-byte path with tiles inside the region)
    ax.case_pack_int(B, vs, 64, 128, pitch_case=1)


@pytest.mark.parametrize("vs", ax.SIZES)
def test_unpack_integers(B, vs):
    for k, (T, Cn) in enumerate(SHAPES):
        ax.case_unpack(B, vs, Cn, T, ax.kind_of(vs), pitch_case=k % 2)
    ax.case_unpack(B, vs, 132, 300, ax.kind_of(vs))
    for how in ("file", "zero", "short"):
        ax.case_unpack(B, vs, 65, 131, ax.kind_of(vs), how=how)
        ax.case_unpack(B, vs, 64, 33, ax.kind_of(vs), how=how, pitch_case=1)


FLOAT_SIZES = tuple(vs for vs in ax.SIZES if vs >= 7)  # (float_edges_common.channels needs four bits; 1, 2 and 3: the integer entries)


@pytest.mark.parametrize("vs", FLOAT_SIZES)
def test_pack_floats(B, vs):
    """the float entry against the oracle's stage: every T and every C at factor 100, a selection at 1, 3.3 and -100"""
    for k, (T, Cn) in enumerate(SHAPES):
        if T:
            ax.case_pack_float(B, vs, 100.0, Cn, T, pitch_case=k % 2)
    for i, factor in enumerate(ax.FACTORS[1:]):
        for k, (T, Cn) in enumerate(SHAPES[1 + i::7]):
            if T:
                ax.case_pack_float(B, vs, factor, Cn, T, pitch_case=k % 2)


@pytest.mark.parametrize("vs", FLOAT_SIZES)
def test_unpack_floats(B, vs):
    for k, (T, Cn) in enumerate(SHAPES):
        ax.case_unpack(B, vs, Cn, T, ax.F32, 100.0, pitch_case=k % 2)
    for i, factor in enumerate(ax.FACTORS[1:]):
        for k, (T, Cn) in enumerate(SHAPES[1 + i::7]):
            ax.case_unpack(B, vs, Cn, T, ax.F32, factor, pitch_case=k % 2)
        for how in ("file", "zero", "short"):
            ax.case_unpack(B, vs, 65, 70, ax.F32, factor, how=how)


@pytest.mark.parametrize("vs", (1, 2, 3))
def test_unpack_floats_at_the_smallest_sizes(B, vs):
    """the float exit on integer streams: every field of one, two and three bits through the oracle's `decode normalize`"""
    for factor in ax.FACTORS:
        ax.case_unpack(B, vs, 65, 129, ax.F32, factor)
        ax.case_unpack(B, vs, 65, 131, ax.F32, factor, how="file")


# ---- refusals, counts, cuts ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("factor", ax.FACTORS)
@pytest.mark.parametrize("vs", (8, 12, 17, 32, 33, 64))
def test_refusals(B, vs, factor):
    ax.case_refusals(B, vs, factor)


@pytest.mark.parametrize("floats", (False, True))
@pytest.mark.parametrize("vs", (3, 8, 12, 17, 24, 32, 33, 47, 64))
def test_counts(B, vs, floats):
    if floats and vs < 4:
        vs = 7
    for T in ax.ROWS:
        for Cn, short in ((65, False), (64, True), (130, False)):
            if T or not short:
                ax.case_counts(B, vs, Cn, T, floats, short_cap=short)


@pytest.mark.parametrize("vs", ax.SIZES)
def test_unpack_cuts(B, vs):
    ax.case_unpack_cuts(B, vs, ax.kind_of(vs))
    for factor in ax.FACTORS:
        ax.case_unpack_cuts(B, vs, ax.F32, factor)


@pytest.mark.parametrize("factor", ax.FACTORS)
@pytest.mark.parametrize("vs", (8, 16, 24, 32, 47, 64))
def test_round_trip(B, vs, factor):
    for T, Cn in ((1, 1), (129, 65), (300, 130)):
        ax.case_round_trip(B, vs, factor, Cn, T)


# ---- the Python surface: compaction, levels, the host forms ------------------------------------------------------------------------

def readings(T, Cn, seed):
    return meter(np.random.default_rng([2040, T, Cn, seed]), T, Cn, top=3000.0)


@pytest.mark.parametrize("vs", (12, 24, 32, 40))
def test_binding_and_compaction(dca, ctx, vs):
    """Context.axdr_encode / axdr_decode on tensors, and compact() of the slabs: orc.file_bytes of every channel, back to back"""
    import torch
    T, Cn = 131, 67
    v = readings(T, Cn, vs) if vs >= 24 else readings(T, Cn, vs) / np.float32(200.0)  # (12 bits at factor 100: readings below 20)
    slabs, bits, err = ctx.axdr_encode(torch.from_numpy(v).cuda(), vs)
    torch.cuda.synchronize()
    want = ax.want_float(v.view(np.uint32), vs, 100.0)
    assert all(w[0] == 0 for w in want)
    got = slabs.cpu().numpy()
    for c, (_, data, n) in enumerate(want):
        assert int(err[c]) == 0 and int(bits[c]) == n and got[c, : len(data)].tobytes() == data, (vs, c)
    packed, offsets = ctx.compact(slabs, bits)
    torch.cuda.synchronize()
    assert packed.cpu().numpy().tobytes() == b"".join(orc.file_bytes(data, n) for _, data, n in want)
    assert int(offsets[-1]) == sum((n + 7) // 8 for _, _, n in want)
    back, count, derr = ctx.axdr_decode(slabs, bits, T, vs)
    torch.cuda.synchronize()
    assert (derr.cpu().numpy() == 0).all() and (count.cpu().numpy() == T).all()
    for c, (_, data, n) in enumerate(want):
        r, vals = ax.oracle_unpack(data, n, vs, 100.0)
        assert r == 0 and fe.same_float_bits(back[:, c].cpu().numpy().view(np.uint32), vals).all(), (vs, c)
    # the integer surface: fields in, the same fields out
    f = ax.fields(vs, T, Cn, 5)
    x = torch.from_numpy(ax.containers(f, vs).view(np.int64 if vs > 32 else np.int32)).cuda()
    samples = dca.SAMPLES_I64 if vs > 32 else dca.SAMPLES_I32
    slabs, bits, err = ctx.axdr_encode(x, vs, samples=samples)
    y, count, derr = ctx.axdr_decode(slabs, bits, T, vs, samples=samples)
    torch.cuda.synchronize()
    assert (err.cpu().numpy() == 0).all() and (derr.cpu().numpy() == 0).all() and (count.cpu().numpy() == T).all()
    assert (y.cpu().numpy().view(np.uint64 if vs > 32 else np.uint32) == f.astype(np.uint64 if vs > 32 else np.uint32)).all()


@pytest.mark.parametrize("counted", (False, True))
@pytest.mark.parametrize("vs", (24, 32, 47))
def test_levels(dca, ctx, vs, counted):
    """every level's streams, bits, counts and statuses: aggregate_levels followed by axdr_encode on each level"""
    import torch
    T, Cn = 300, 68
    v = readings(T, Cn, 7)
    v[17, 5] = np.float32(3e38)  # one channel that Normalize refuses at every level
    count = None
    if counted:
        count = torch.from_numpy(ax.counts_for(Cn, T).astype(np.int64)).cuda()
        for c in range(Cn):
            n = min(int(ax.counts_for(Cn, T)[c]), T)
            v[n:, c] = ax.POISON.view(np.float32)[(c + np.arange(T - n)) % ax.POISON.size]
    vt = torch.from_numpy(v).cuda()
    got = ctx.axdr_encode_levels_f32(vt, LEVELS, vs, count=count)
    if counted:
        sums, counts, aerr = ctx.aggregate_levels(vt, LEVELS, count=count)
    else:
        sums, counts, aerr = ctx.aggregate_levels(vt, LEVELS), [None] * len(LEVELS), None
    torch.cuda.synchronize()
    refused = 0
    for k, n in enumerate(LEVELS):
        slabs, bits, err = ctx.axdr_encode(sums[k].contiguous(), vs, count=counts[k], cap=got[k][0].shape[1])
        torch.cuda.synchronize()
        want_err = err.cpu().numpy().copy()
        want_bits = bits.cpu().numpy().copy()
        if counted:
            a = aerr.cpu().numpy()
            want_err[a != 0], want_bits[a != 0] = a[a != 0], 0
            assert (got[k][3].cpu().numpy() == counts[k].cpu().numpy()).all(), ("counts", vs, n)
            assert (a != 0).sum() == (ax.counts_for(Cn, T) > T).sum() > 0
        assert (got[k][2].cpu().numpy() == want_err).all(), ("status", vs, n, got[k][2].cpu().numpy(), want_err)
        ok = want_err == 0
        assert (got[k][1].cpu().numpy()[ok] == want_bits[ok]).all(), ("bits", vs, n)
        assert (got[k][0].cpu().numpy()[ok] == slabs.cpu().numpy()[ok]).all(), ("streams", vs, n)
        refused += int((want_err == -1).sum())
        # and one channel of the level against the oracle itself
        c = 9
        m = sums[k].shape[0] if not counted else int(counts[k][c])
        r, data, nb = ax.oracle_pack(sums[k][:m, c].cpu().numpy().view(np.uint32), vs, 100.0)
        assert r == int(got[k][2][c]), ("oracle", vs, n, r)
        assert r != 0 or (int(got[k][1][c]) == nb and got[k][0][c, : len(data)].cpu().numpy().tobytes() == data), ("oracle", vs, n)
    assert refused >= len(LEVELS)


@pytest.mark.parametrize("pinned", (False, True))
@pytest.mark.parametrize("Cn", (70, 37))
def test_host_forms(dca, ctx, Cn, pinned, monkeypatch):
    """DEGA_HOST_CHUNK_BYTES set so that the call runs as 1, 5 and C chunks; pinned and pageable memory; the one-chunk result and
    the oracle; sentinels around the outputs"""
    T, vs, ld = 131, 24, Cn + 3
    rows = np.full((T, ld), np.float32("nan"), dtype=np.float32)
    rows[:, :Cn] = readings(T, Cn, 11)
    rows[40, 4] = np.float32(1e9)  # refused
    count = ax.counts_for(Cn, T)
    count[4] = T
    cap = ax.axdr_bytes(T, vs) + 8
    per_channel = T * 4 + cap + 16
    want = ax.want_float(rows[:, :Cn].view(np.uint32), vs, 100.0, count, cap)
    keep = []

    def array(shape, dtype, fill):
        if pinned:
            keep.append(dca.PinnedArray(shape, dtype))
            a = keep[-1].array
        else:
            a = np.empty(shape, dtype=dtype)
        a[...] = fill
        return a

    x = array(rows.shape, np.float32, 0)
    x[...] = rows
    results = {}
    try:
        for chunks, step in ((1, Cn + 3), (5, 16 if Cn == 70 else 8), (Cn, 1)):  # (a step of four or more is rounded down to a multiple of four)
            monkeypatch.setenv("DEGA_HOST_CHUNK_BYTES", str(per_channel * step))
            out = array((Cn + 2, cap), np.uint8, ax.CANARY)  # a sentinel slab on either side
            slabs, bits, err = ctx.axdr_encode_host(x, vs, count=count, channels=Cn, out=out[1:])
            assert (out[0] == ax.CANARY).all() and (out[-1] == ax.CANARY).all(), chunks
            ax.check_packed(ax.Packed(out[1:Cn + 1], bits, err), want, ("host encode", Cn, pinned, chunks))
            healthy = err == 0
            results[chunks] = (out[1:Cn + 1].copy(), bits.copy(), err.copy())
            assert (results[chunks][1][healthy] == results[1][1][healthy]).all() and (results[chunks][2] == results[1][2]).all()
            assert (results[chunks][0][healthy] == results[1][0][healthy]).all()
            # and back: the streams of the healthy channels, one too many bits on one of them
            in_bits = np.where(healthy, bits, 0).astype(np.uint64)
            in_bits[7] += 1
            back = array((T + 2, ld), np.float32, np.float32(-7.5))
            v, n, derr = ctx.axdr_decode_host(out[1:Cn + 1], in_bits, T, vs, out=back[1:T + 1])
            assert (back[0] == -7.5).all() and (back[-1] == -7.5).all() and (back[:, Cn:] == -7.5).all(), chunks
            dwant = ax.want_unpack([out[1 + c].tobytes() for c in range(Cn)], in_bits, vs, ax.F32, T, 100.0)
            assert dwant[7][0] == ax.LIBRARY_CALL
            ax.check_unpacked(ax.Unpacked(v.view(np.uint32), n, derr), dwant, ax.F32, ("host decode", Cn, pinned, chunks))
    finally:
        for p in keep:
            p.free()


# ---- refusals of the entry points, with a live context -----------------------------------------------------------------------------

def test_refusals_of_the_entry_points(dca, ctx, B):
    L = dca.library()
    x = B.buf(np.zeros((3, 4), dtype=np.float32))
    out, bits, err, cnt = B.buf(np.full(64, 0xC5, np.uint8)), B.buf(np.zeros(4, np.uint64)), B.buf(np.full(4, 77, np.int32)), B.buf(np.zeros(4, np.uint64))
    S = dca

    def enc(vs=8, samples=S.SAMPLES_F32, ld=4, cap=8, xx=B.ptr(x), oo=B.ptr(out), bb=B.ptr(bits), ee=B.ptr(err), T=3):
        return L.dega_hip_axdr_encode_dev(ctx._h, xx, samples, 4, T, ld, None, 100.0, vs, oo, cap, bb, ee, ctx._stream())

    def dec(vs=8, samples=S.SAMPLES_F32, ld=4, cap=8, xx=B.ptr(x), oo=B.ptr(out), bb=B.ptr(bits), ee=B.ptr(err), T=3, cc=B.ptr(cnt)):
        return L.dega_hip_axdr_decode_dev(ctx._h, oo, cap, bb, 4, T, ld, 100.0, vs, samples, xx, cc, ee, ctx._stream())

    bad = (dict(vs=0), dict(vs=65), dict(vs=33, samples=S.SAMPLES_I32), dict(vs=32, samples=S.SAMPLES_I64), dict(samples=S.SAMPLES_BE32),
           dict(samples=S.SAMPLES_F32 | S.SAMPLES_CHANNEL_MAJOR), dict(samples=7), dict(ld=3), dict(cap=6), dict(xx=None), dict(oo=None), dict(bb=None),
           dict(ee=None), dict(T=1 << 32), dict(xx=B.ptr(x) + 2), dict(bb=B.ptr(bits) + 4))
    for call in (enc, dec):
        for kw in bad:
            assert call(**kw) == dca.ERROR_INVALID_VALUE, (call.__name__, kw)
            assert "axdr" in ctx.last_error()
    assert dec(cc=None) == dca.ERROR_INVALID_VALUE
    assert (B.get(out) == 0xC5).all() and (B.get(err).view(np.int32) == 77).all()
    assert enc() == 0 and dec() == 0
    assert L.dega_hip_axdr_encode_dev(ctx._h, None, S.SAMPLES_F32, 0, 3, 0, None, 100.0, 8, None, 8, None, None, ctx._stream()) == 0  # C = 0
    B.get(out)


# ---- index width ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def V(dca, ctx):
    import torch
    import index_width_common as iw
    from test_gpu_index_width import Device as Images

    class Sparse(Images):
        def __init__(self):  # (the three images these cases use, never written as a whole)
            self.torch, self.dca, self.ctx, self.L = torch, dca, ctx, dca.library()
            self.images = {name: torch.empty(size, dtype=torch.uint8, device="cuda") for name, size in iw.IMAGES.items() if name in ("BIG", "MID", "TEXT")}
            self.kept = []
            self.kinds = {"int32": torch.int32, "int64": torch.int64, "uint8": torch.uint8}

    v = Sparse()
    yield v
    v.close()


@pytest.mark.parametrize("what", ("ld", "cap"))
def test_offsets_are_64_bit_on_the_device(B, V, what):
    """ld = 2^26 at T = 70 and cap = 2^29 at C = 12: sparse images, only the logical regions touched; the emulator has run the
    same cases (tests/test_axdr_host.py)"""
    try:
        ax.case_index_width(B, V, what)
    finally:
        V.forget()
