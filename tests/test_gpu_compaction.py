"""GPU tests (-m gpu) of the kernels that carry every packed stream, on their own: dega_offsets_kernel (bit lengths -> byte
offsets), dega_gather_kernel (slabs -> streams back to back) and dega_scatter_kernel (the inverse), and the wave_copy_bytes
under the last two -- a head up to the destination's 16-byte boundary, rounds of 16 bytes per lane shifted into place at the
source's own alignment (v_alignbyte), a tail of fewer than 20 bytes.

Through the C ABI (dega_hip_compact_offsets_dev / dega_hip_compact_gather_dev) on torch buffers; what is expected comes from
numpy.  The pipeline tests cannot see these kernels go wrong: they compare the gather with the gather."""
import numpy as np
import pytest

from __graft_entry__ import load_package
from oracle import orc

pytestmark = pytest.mark.gpu

POISON = 0xA5


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


def to_dev(a):
    """a numpy array of uint8 / uint64 / int64 as a device tensor of the same bytes (torch has no uint64 arithmetic: int64)"""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def source_bytes(rng, n):
    """random bytes, none of them the poison: a byte that was not copied can never look as if it had been"""
    b = rng.integers(0, 256, n, dtype=np.uint8)
    b[b == POISON] = POISON ^ 0xFF
    return b


# ---- dega_offsets_kernel ---------------------------------------------------------------------------------------------------------

def bit_lengths(kind, Cn):
    rng = np.random.default_rng([3, Cn, ("edges", "random", "near 2^35").index(kind)])
    if kind == "edges":  # no bytes, one bit, the last bit of a byte, a whole byte, one bit more
        return np.array([0, 1, 7, 8, 9], dtype=np.uint64)[np.arange(Cn) % 5]
    if kind == "random":
        b = rng.integers(0, 1 << 20, Cn).astype(np.uint64)
        b[rng.random(Cn) < 0.1] = 0
        return b
    return ((1 << 35) + rng.integers(-9, 10, Cn)).astype(np.uint64)  # 2^32 bytes each: the second sum is beyond 32 bits


@pytest.mark.parametrize("kind", ("edges", "random", "near 2^35"))
def test_offsets_are_the_running_sum_of_the_streams_bytes(dca, ctx, kind):
    """offsets = [0] + cumsum(ceil(bits / 8)) in 64 bits, for channel counts around the block's 1 024 entries (the carry from
    one trip of the scan to the next, a ragged last trip, none at all) and sums that pass 2^32; the element behind
    offsets[C] is not written.  Catches: a scan that drops or doubles the carry between trips, 32-bit sums, the rounding
    of a bit length to bytes, a store beyond C + 1 entries."""
    import torch
    L = dca.library()
    behind = 4
    cases = []
    for Cn in (0, 1, 2, 1023, 1024, 1025, 2048, 3000):
        bits = bit_lengths(kind, Cn)
        d_bits = to_dev(bits if Cn else np.zeros(1, dtype=np.uint64))
        d_off = torch.full((Cn + 1 + behind,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda")
        assert L.dega_hip_compact_offsets_dev(ctx._h, d_bits.data_ptr(), Cn, d_off.data_ptr(), ctx._stream()) == 0
        cases.append((Cn, bits, d_bits, d_off))
    torch.cuda.synchronize()
    for Cn, bits, _, d_off in cases:
        got = d_off.cpu().numpy().view(np.uint64)
        want = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum((bits + np.uint64(7)) // np.uint64(8), dtype=np.uint64)])
        assert want.dtype == np.uint64 and (got[: Cn + 1] == want).all(), (kind, Cn, int(np.nonzero(got[: Cn + 1] != want)[0][0]))
        assert (got[Cn + 1:] == np.uint64(0xA5A5A5A5A5A5A5A5)).all(), (kind, Cn, "written behind offsets[C]")
        if kind == "near 2^35" and Cn >= 2:
            assert int(want[Cn]) > 1 << 32


# ---- wave_copy_bytes, one channel at a time --------------------------------------------------------------------------------------

LENGTHS = (0, 1, 3, 15, 16, 17, 19, 20, 21, 35, 36, 37, 1043, 1044, 1045, 2100)
REGION, SLAB = 2560, 2304  # bytes of the packed buffer / of the source per case: multiples of 256 / of 4, room for every case


@pytest.mark.parametrize("src_align", (0, 1, 2, 3))
def test_one_wave_copies_any_length_at_any_alignment(dca, ctx, src_align):
    """Single-channel gathers: the destination 0 ... 15 bytes behind a 16-byte boundary (offsets[0] is not 0), the slab 0 ... 3
    bytes behind a dword, and lengths that take no round (n - head < 20), the first round, the second, and a lane's second
    trip through the loop (beyond 64 lanes x 16 bytes) -- each with a length on either side of the step.  The packed buffer
    is poisoned: the stream's bytes are the source's, and every other byte still holds the poison.  Catches: the gather's
    head (bytes up to the boundary), the number of rounds, the shift of the five source dwords at each of the four source
    alignments (the head moves it), the tail's start and length, any store outside [o0, o0 + n)."""
    import torch
    L = dca.library()
    rng = np.random.default_rng([5, src_align])
    cases = [(d, n) for d in range(16) for n in LENGTHS]
    K = len(cases)
    src = source_bytes(rng, K * SLAB + 256)
    o0 = np.array([d + 16 * (k % 5) for k, (d, n) in enumerate(cases)], dtype=np.uint64)  # (a few boundaries into the region)
    offsets = np.stack([o0, o0 + np.array([n for _, n in cases], dtype=np.uint64)], axis=1)
    assert int(offsets.max()) <= REGION - 256 and max(LENGTHS) + 3 + 20 <= SLAB
    d_src, d_off = to_dev(src), to_dev(offsets)
    d_packed = torch.full((K * REGION + 256,), POISON, dtype=torch.uint8, device="cuda")
    assert d_packed.data_ptr() % 256 == 0 and d_src.data_ptr() % 256 == 0
    for k in range(K):
        ret = L.dega_hip_compact_gather_dev(ctx._h, d_src.data_ptr() + k * SLAB + src_align, SLAB, d_off.data_ptr() + 16 * k, 1,
                                            d_packed.data_ptr() + k * REGION, ctx._stream())
        assert ret == 0
    torch.cuda.synchronize()  # (one wait for all of them)
    got = d_packed.cpu().numpy()
    want = np.full(K * REGION + 256, POISON, dtype=np.uint8)
    for k, (d, n) in enumerate(cases):
        at = k * REGION + int(o0[k])
        assert at % 16 == d
        want[at: at + n] = src[k * SLAB + src_align: k * SLAB + src_align + n]
    if not (got == want).all():
        bad = int(np.nonzero(got != want)[0][0])
        k = min(bad // REGION, K - 1)
        d, n = cases[k]
        raise AssertionError("source alignment %d, destination alignment %d, %d bytes at %d: byte %d of the case's region is 0x%02X, not 0x%02X"
                             % (src_align, d, n, int(o0[k]), bad - k * REGION, int(got[bad]), int(want[bad])))


# ---- many channels at once -------------------------------------------------------------------------------------------------------

def test_gather_of_many_channels_is_the_concatenation(dca, ctx):
    """1 500 slabs of an odd pitch (so the slabs start at every alignment) with 0 ... 300 bytes each, a tenth of them empty,
    gathered behind offsets[0] = 5: the packed range is the streams back to back, and the bytes before offsets[0] and
    behind offsets[C] keep their poison.  Catches: the slab's address (c * cap), a wave taking the wrong channel in its
    workgroup or the ragged last workgroup, empty streams, a copy that spills into its neighbour."""
    import torch
    L = dca.library()
    rng = np.random.default_rng(6)
    Cn, cap, first = 1500, 301, 5
    n = rng.integers(1, 301, Cn)
    n[rng.random(Cn) < 0.1] = 0
    n[[0, 1, Cn - 1]] = (300, 0, 299)
    assert 100 < int((n == 0).sum()) < 220 and cap % 2 == 1
    offsets = (first + np.concatenate([[0], np.cumsum(n)])).astype(np.uint64)
    slabs = source_bytes(rng, Cn * cap).reshape(Cn, cap)
    total = int(offsets[Cn])
    d_slabs, d_off = to_dev(slabs), to_dev(offsets)
    d_packed = torch.full((total + 64,), POISON, dtype=torch.uint8, device="cuda")
    assert L.dega_hip_compact_gather_dev(ctx._h, d_slabs.data_ptr(), cap, d_off.data_ptr(), Cn, d_packed.data_ptr(), ctx._stream()) == 0
    torch.cuda.synchronize()
    got = d_packed.cpu().numpy()
    want = np.concatenate([np.full(first, POISON, dtype=np.uint8)] + [slabs[c, : n[c]] for c in range(Cn)] + [np.full(64, POISON, dtype=np.uint8)])
    assert got.size == want.size
    if not (got == want).all():
        bad = int(np.nonzero(got != want)[0][0])
        raise AssertionError("byte %d differs (channel %d)" % (bad, int(np.searchsorted(offsets, bad, side="right")) - 1))


# ---- the scatter side ------------------------------------------------------------------------------------------------------------

def test_scatter_spreads_short_streams_into_slabs(dca, ctx):
    """decode_job(var=True) on 700 streams the oracle made from 0 ... 12 samples each: a few bytes per stream, so the packed
    offsets take every residue mod 4 (the scatter's source alignments; its slabs start on dwords) and the lengths lie on
    either side of 20 (with and without a round).  Counts, status and samples are the oracle's.  Catches: the scatter's
    rounds and tail by source alignment, a stream's last bytes dropped or its neighbour's first bytes taken."""
    rng = np.random.default_rng(7)
    Cn, room = 700, 16
    counts = np.arange(Cn) % 13
    rng.shuffle(counts)
    x = (np.cumsum(rng.integers(-3000, 3001, (12, Cn)), axis=0) + rng.integers(20000, 60000, Cn)[None, :]).astype(np.int32)
    streams = []
    for c in range(Cn):
        ret, b, nb = orc.encode_i32(np.ascontiguousarray(x[: counts[c], c]), 1)
        assert ret == 0 and len(b) == (nb + 7) // 8, c
        streams.append((b, nb))
    lens = np.array([len(b) for b, _ in streams])
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    bits = np.array([nb for _, nb in streams], dtype=np.uint64)
    packed = np.frombuffer(b"".join(b for b, _ in streams), dtype=np.uint8)
    assert set((offsets[:-1] % np.uint64(4)).tolist()) == {0, 1, 2, 3}
    assert all((lens == n).any() for n in (1, 19, 20, 21, 35))  # no bytes but the end mark's, either side of the first round, past the second
    y, got_counts, err = ctx.decode_job(packed, offsets, bits, room, adaptive=1, var=True)
    for c in range(Cn):
        ret, want = orc.decode_i32(streams[c][0], streams[c][1], room, 1)
        assert int(err[c]) == ret, (c, int(err[c]), ret)
        if ret == 0:
            assert int(got_counts[c]) == len(want) and (y[: len(want), c] == want).all(), (c, int(counts[c]))
            assert len(want) == counts[c] and (want == x[: counts[c], c]).all(), c
