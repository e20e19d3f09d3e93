"""GPU tests (-m gpu) of the host pipeline over a batch that really is cut into several chunks.  plan_chunks never makes a
chunk narrower than min(C, 8192) channels, so DEGA_PIPELINE_CHUNKS only cuts a batch of more than 8 192 channels:
C = 2 * 8192 + 1100 = 17 484 under DEGA_PIPELINE_CHUNKS=3 is chunks of 8 192, 8 192 and 1 100 channels on a context, and on
Group([0, 0]) a cut at 8 704 with two chunks per member (8 192 + 512 and 8 192 + 588).  The smallest shape at which the
running base of the packed streams across chunks, the reuse of a slot's buffers, a redone middle chunk and the host-side
concatenate of the members can all go wrong -- for the plain coder, for K > 1 levels and for LZMH.

What is compared against: the same call without the knob -- one chunk, which the other files hold to the oracle -- byte
for byte; for LZMH the single-context slab calls, and the oracle itself on the first 64 channels."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from __graft_entry__ import load_package
from oracle import orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from agg_common import meter  # noqa: E402

pytestmark = pytest.mark.gpu

CN = 2 * 8192 + 1100
CUT = 8704  # where Group([0, 0]) cuts CN channels: whole 512-channel (LZMH: 256-channel) workgroups


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
def groups(dca, ctx):
    gs = {"one": dca.Group([0]), "two": dca.Group([0, 0])}
    yield gs
    for g in gs.values():
        g.close()


def test_the_shape_is_what_it_claims(dca):
    cuts = (C.c_size_t * 3)()
    assert dca.library().dega_hip_split_channels(CN, 2, cuts) == 0 and list(cuts) == [0, CUT, CN]


# ---- the plain coder ---------------------------------------------------------------------------------------------------------

T_PLAIN = 64
NOISY = (9000, 17000)  # one in the second chunk, one in the last (of the second member: one in each of its chunks)


@pytest.fixture(scope="module")
def plain(dca, ctx):
    """int32 walks with two channels of noise, and their one-chunk encode and decode (computed once, never changed)"""
    assert "DEGA_PIPELINE_CHUNKS" not in os.environ
    rng = np.random.default_rng(1748)
    x = np.cumsum(rng.integers(-50, 51, (T_PLAIN, CN)), axis=0) + rng.integers(20000, 60000, CN)[None, :]
    x = np.clip(x, 0, 2 ** 31 - 1).astype(np.int32)
    for c in NOISY:
        x[:, c] = rng.integers(0, 1 << 30, T_PLAIN)
    want = ctx.encode_job(x, adaptive=1)
    back = ctx.decode_job(want[0], want[1], want[2], T_PLAIN, adaptive=1, var=True)
    for a in (x,) + tuple(want) + tuple(back):
        a.flags.writeable = False
    return x, want, back


def test_plain_encode_across_chunks_with_redone_chunks(dca, ctx, groups, plain, monkeypatch):
    x, want, _ = plain
    packed, offsets, bits, err = want
    for c in NOISY:  # the case is what it claims to be: longer than the usual slab, so the chunk is redone
        assert int(err[c]) == 0 and int(offsets[c + 1] - offsets[c]) > 4 * T_PLAIN + 64, c
    assert int(offsets[0]) == 0 and int(offsets[CN]) == packed.size
    pin = dca.PinnedArray((T_PLAIN, CN), np.int32)
    try:
        pin.array[:] = x
        monkeypatch.setenv("DEGA_PIPELINE_CHUNKS", "3")
        for ahead in ("1", "2", "16"):
            monkeypatch.setenv("DEGA_PIPELINE_AHEAD", ahead)
            for who, src in ((ctx, x), (ctx, pin.array), (groups["one"], x), (groups["two"], x)):
                got = who.encode_job(src, adaptive=1)
                for g, w, name in zip(got, want, ("packed", "offsets", "bits", "err")):
                    assert g.shape == w.shape and g.tobytes() == w.tobytes(), (type(who).__name__, src is x, ahead, name)
    finally:
        pin.free()


@pytest.mark.parametrize("uploads_first", ("0", "1"))
def test_plain_decode_across_chunks(dca, ctx, plain, monkeypatch, uploads_first):
    x, (packed, offsets, bits, err), (want_x, want_counts, want_derr) = plain
    monkeypatch.setenv("DEGA_PIPELINE_CHUNKS", "3")
    monkeypatch.setenv("DEGA_PIPELINE_UPLOADS_FIRST", uploads_first)
    back, counts, derr = ctx.decode_job(packed, offsets, bits, T_PLAIN, adaptive=1, var=True)
    ok = err == 0
    assert ok[list(NOISY)].all() and (back[:, ok] == x[:, ok]).all()
    assert (counts == want_counts).all() and (derr == want_derr).all()


@pytest.mark.parametrize("who", ("ctx", "two"))
def test_plain_packed_buffer_too_small(dca, ctx, groups, plain, monkeypatch, who):
    """through the C ABI: ERROR_MEMORY, and offsets (offsets[C] included), bits and err are complete all the same -- when
    the last byte is missing, and when the first chunk just fits and everything behind it does not"""
    x, (packed, offsets, bits, err), _ = plain
    L = dca.library()
    fn, h = (L.dega_hip_encode_job_host, ctx._h) if who == "ctx" else (L.dega_hip_group_encode, groups[who]._h)
    job = dca.Job(CN, T_PLAIN, CN, 1, 32, dca.SAMPLES_I32, 0.0)
    monkeypatch.setenv("DEGA_PIPELINE_CHUNKS", "3")
    for cap in (packed.size - 1, int(offsets[8192]) + 1):
        buf = np.zeros(cap, dtype=np.uint8)
        o, b, e = np.full(CN + 1, 7, dtype=np.uint64), np.full(CN, 7, dtype=np.uint64), np.full(CN, 7, dtype=np.int32)
        ret = fn(h, C.byref(job), x.ctypes.data, buf.ctypes.data, cap, o.ctypes.data, b.ctypes.data, e.ctypes.data)
        assert ret == dca.ERROR_MEMORY, cap
        assert (o == offsets).all() and (b == bits).all() and (e == err).all(), cap


# ---- several granularities -----------------------------------------------------------------------------------------------------

T_LEVELS, LEVELS = 96, [1, 4, 12]


@pytest.fixture(scope="module")
def levels(dca, ctx):
    """float32 meter series with one channel of noise in the second chunk, and every level's one-chunk job"""
    assert "DEGA_PIPELINE_CHUNKS" not in os.environ
    rng = np.random.default_rng(1749)
    v = meter(rng, T_LEVELS, CN)
    v[:, 9000] = rng.integers(0, 2 ** 26, T_LEVELS).astype(np.float32)  # (the sums of twelve such values stay inside 32 bits)
    want = [ctx.encode_job(v, adaptive=1, samples=dca.SAMPLES_F32, factor=1.0, num_values=N) for N in LEVELS]
    for a in [v] + [a for w in want for a in w]:
        a.flags.writeable = False
    return v, want


def assert_same_job(got, want, tag):
    for x, y in zip(got, want):
        assert x.shape == y.shape and (x == y).all(), tag


def test_levels_across_chunks(dca, ctx, groups, levels, monkeypatch):
    v, want = levels
    for w in want:
        assert (w[3] == 0).all()
    # at N = 1 the noise outgrows the usual slab, so that level of the second chunk is redone and the others are not
    assert int(want[0][1][9001] - want[0][1][9000]) > 4 * T_LEVELS + 64
    monkeypatch.setenv("DEGA_PIPELINE_CHUNKS", "3")
    for who in (ctx, groups["two"]):
        got = who.encode_job_levels(v, LEVELS, adaptive=1, factor=1.0)
        for k, N in enumerate(LEVELS):
            assert_same_job(got[k], want[k], (type(who).__name__, N))


@pytest.mark.parametrize("who", ("ctx", "two"))
def test_levels_one_packed_cap_too_small(dca, ctx, groups, levels, monkeypatch, who):
    """through the C ABI: the level whose buffer is one byte short reports its size, every level's offsets / bits / err are
    complete, and the other two levels' bytes are delivered"""
    v, want = levels
    L = dca.library()
    fn, h = (L.dega_hip_encode_levels_job_host, ctx._h) if who == "ctx" else (L.dega_hip_group_encode_levels, groups[who]._h)
    K = len(LEVELS)
    caps = [want[0][0].size, want[1][0].size - 1, want[2][0].size]
    packed = [np.zeros(c, dtype=np.uint8) for c in caps]
    offsets = [np.full(CN + 1, 7, dtype=np.uint64) for _ in range(K)]
    bits = [np.full(CN, 7, dtype=np.uint64) for _ in range(K)]
    err = [np.full(CN, 7, dtype=np.int32) for _ in range(K)]
    hp = lambda arrs: (C.c_void_p * K)(*[a.ctypes.data for a in arrs])  # noqa: E731
    job = dca.Job(CN, T_LEVELS, CN, 1, 32, dca.SAMPLES_F32, 1.0)
    monkeypatch.setenv("DEGA_PIPELINE_CHUNKS", "3")
    ret = fn(h, C.byref(job), (C.c_size_t * K)(*LEVELS), K, v.ctypes.data, hp(packed), (C.c_size_t * K)(*caps), hp(offsets), hp(bits), hp(err))
    assert ret == dca.ERROR_MEMORY
    for k in range(K):
        assert (offsets[k] == want[k][1]).all() and (bits[k] == want[k][2]).all() and (err[k] == want[k][3]).all(), k
    for k in (0, 2):
        assert (packed[k] == want[k][0]).all(), k


# ---- LZMH ----------------------------------------------------------------------------------------------------------------------

STRIDE = 48


@pytest.fixture(scope="module")
def lzmh(dca, ctx):
    """17 484 strings of 0 ... 40 bytes (the kinds of test_gpu_lzmh.make_strings), and the single-context slab calls on them"""
    from test_gpu_lzmh import make_strings
    assert "DEGA_PIPELINE_CHUNKS" not in os.environ
    strings = [s[:40] for s in make_strings(np.random.default_rng(1750), CN, 41)]
    text = np.zeros((CN, STRIDE), dtype=np.uint8)
    lens = np.array([len(s) for s in strings], dtype=np.uint64)
    for i, s in enumerate(strings):
        text[i, : len(s)] = np.frombuffer(s, dtype=np.uint8)
    want_out, want_bits, want_err = ctx.lzmh_encode_host(strings)
    assert (want_err == 0).all()
    for c in range(64):
        r, b, n = orc.stage("lzmh", True, strings[c], 8 * len(strings[c]))
        assert r == 0 and int(want_bits[c]) == n and want_out[c, : (n + 7) // 8].tobytes() == b[: (n + 7) // 8], c
    want_back, want_lens, want_derr = ctx.lzmh_decode_host(want_out, want_bits, STRIDE)
    assert (want_derr == 0).all()
    # the codec's quirks: an empty stream decodes to one byte, and some short strings lose a last zero byte (the oracle does
    # the same).  Every other string has to come back as it went in.
    quirk = {c for c, s in enumerate(strings) if int(want_lens[c]) != len(s)}
    assert all(strings[c] == b"" or strings[c][-1] == 0 for c in quirk) and len(quirk) < CN // 20
    for c in sorted(quirk)[:16]:
        r, b, n = orc.stage("lzmh", False, want_out[c, : (int(want_bits[c]) + 7) // 8].tobytes(), int(want_bits[c]))
        assert r == 0 and n // 8 == int(want_lens[c]), c
    return strings, text, lens, want_out, want_bits, want_back, want_lens, quirk


@pytest.mark.parametrize("who", ("one", "two"))
def test_lzmh_across_chunks(dca, ctx, groups, lzmh, monkeypatch, who):
    strings, text, lens, want_out, want_bits, want_back, want_lens, quirk = lzmh
    g = groups[who]
    pinned = dca.PinnedArray((CN, STRIDE), np.uint8)
    try:
        pinned.array[:] = text
        monkeypatch.setenv("DEGA_PIPELINE_CHUNKS", "3")
        for src in (text, pinned.array):
            packed, offsets, bits, err = g.lzmh_encode_job(src, lens)
            assert (err == 0).all() and (bits == want_bits).all()
            assert int(offsets[0]) == 0 and (np.diff(offsets.astype(np.int64)) == (bits.astype(np.int64) + 7) // 8).all()
            for c in range(CN):
                nb = (int(bits[c]) + 7) // 8
                assert packed[int(offsets[c]): int(offsets[c]) + nb].tobytes() == want_out[c, :nb].tobytes(), (who, c)
            for c in range(64):
                r, b, n = orc.stage("lzmh", True, strings[c], 8 * len(strings[c]))
                assert r == 0 and int(bits[c]) == n and packed[int(offsets[c]): int(offsets[c + 1])].tobytes() == b[: (n + 7) // 8], (who, c)
            back, blens, berr = g.lzmh_decode_job(packed, offsets, bits, STRIDE)
            assert (berr == 0).all() and (blens == want_lens).all()  # (the codec's quirks included: an empty stream decodes to one byte)
            for c in range(CN):
                assert back[c, : int(want_lens[c])].tobytes() == want_back[c, : int(want_lens[c])].tobytes(), (who, c)
                assert c in quirk or back[c, : len(strings[c])].tobytes() == strings[c], (who, c)
        # one byte short, through the C ABI: the call says how much it needs
        size = int(offsets[CN])
        small = np.zeros(size - 1, dtype=np.uint8)
        o, b, e = np.zeros(CN + 1, dtype=np.uint64), np.zeros(CN, dtype=np.uint64), np.zeros(CN, dtype=np.int32)
        ret = dca.library().dega_hip_group_lzmh_encode(g._h, text.ctypes.data, STRIDE, lens.ctypes.data, CN, small.ctypes.data, small.size, o.ctypes.data,
                                                       b.ctypes.data, e.ctypes.data)
        assert ret == dca.ERROR_MEMORY and int(o[CN]) == size
    finally:
        pinned.free()
