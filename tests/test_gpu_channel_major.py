"""GPU tests (-m gpu) of channel-major batches: dega_hip_to_time_major_dev / dega_hip_to_channel_major_dev against torch.t(),
and the host jobs with DEGA_SAMPLES_CHANNEL_MAJOR (layout="channel") against the same jobs on the contiguous transpose.

A transposition moves bits, so every comparison is exact (integer dtypes; float32 samples are compared as their bytes).

Not expressible, so not tested: "the flag on a slab-style *_host call".  The slab forms (dega_hip_encode_host,
dega_hip_decode_var_host, dega_hip_encode_f32_host, dega_hip_encode64_host, the *_packed_host pair, ...) take their sample
type from their name, not from a `samples` argument or a dega_hip_job, so no caller can hand them the flag; inside they
build their shape with the flag clear.  What can carry a wrong flag is a job: test_refusals_of_the_host_jobs covers a job
with ld < T, a job whose `samples` has an unknown bit or an unknown type beside the flag, and a channel-major levels job of
another type than float32."""
import ctypes as C
import itertools

import numpy as np
import pytest

from __graft_entry__ import load_package
from oracle import orc

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (63, 65), (64, 64), (65, 63), (130, 257), (1024, 96), (257, 130))  # (C, T)
POISON = 0x5A5A5A5A


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


def dev_image(rows, used, pitch, dtype, offset_elems=0, fill=POISON):
    """CUDA tensor [rows, pitch] (contiguous, its first element offset_elems elements behind the allocation's 256-byte
    aligned base) filled with `fill`, and the view of its logical [rows, used] part"""
    import torch
    flat = torch.full((rows * pitch + offset_elems,), fill, dtype=dtype, device="cuda")
    full = flat[offset_elems:].view(rows, pitch)
    return full, full[:, :used]


def pitch_cases(used, esz):
    """(pitch, base offset in elements): tight; a multiple of 4 elements on a 16-byte base; an odd pitch; a base one element off"""
    odd = used + 1 if used % 2 == 0 else used + 2
    return ((used, 0), ((used + 3) // 4 * 4 + 4, 0), (odd, 0), (used, 1))


# ---- 1. exact transposition ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("esz", (4, 8))
def test_transposition_is_exact_and_padding_survives(ctx, esz):
    import torch
    dt = torch.int32 if esz == 4 else torch.int64
    g = torch.Generator(device="cuda").manual_seed(7)
    for Cn, T in SHAPES:
        x_ct = torch.randint(-2 ** 31, 2 ** 31 - 1, (Cn, T), dtype=dt, device="cuda", generator=g)
        if esz == 8:
            x_ct = x_ct * 4294967311 + 12345  # all eight bytes in use
        want_tc = x_ct.t().contiguous()
        # every source case with every destination case: tight x tight and multiple-of-4 x multiple-of-4 on aligned bases are
        # the kernel with 16-byte accesses on BOTH sides (where C and T allow: (64, 64), (1024, 96), every padded case), the
        # mixed pairs its two one-sided forms, odd pitches and offset bases the element form
        for (ps, offs), (pd, offd) in itertools.product(pitch_cases(T, esz), pitch_cases(Cn, esz)):
            src_full, src = dev_image(Cn, T, ps, dt, offs, fill=-7)
            src.copy_(x_ct)
            tc_full, _ = dev_image(T, Cn, pd, dt, offd)
            got = ctx.to_time_major(src_full, T=T, out=tc_full)
            assert torch.equal(got, want_tc), (Cn, T, ps, offs, pd, offd)
            assert bool((tc_full[:, Cn:] == POISON).all()), (Cn, T, pd)
            # and back: the identity, into a poisoned image of the source's own pitch
            ct_full, _ = dev_image(Cn, T, ps, dt, offs)
            back = ctx.to_channel_major(tc_full, channels=Cn, out=ct_full)
            assert torch.equal(back, x_ct), (Cn, T, ps, offs, pd, offd)
            assert bool((ct_full[:, T:] == POISON).all()), (Cn, T, ps)
    # float32 is the same four bytes
    v = torch.randn((65, 63), device="cuda", generator=g)
    assert torch.equal(ctx.to_time_major(v), v.t()) and torch.equal(ctx.to_channel_major(v.t().contiguous()), v)


# ---- 2. counts ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("esz", (4, 8))
def test_counts_zero_the_tail_whatever_the_source_holds(ctx, esz):
    import torch
    Cn, T = 200, 150
    g = torch.Generator(device="cuda").manual_seed(11)
    count = torch.randint(0, T + 6, (Cn,), dtype=torch.int64, device="cuda", generator=g)
    count[:5] = torch.tensor([0, T, T + 5, 1, T - 1], device="cuda")
    live = torch.arange(T, device="cuda")[None, :] < count[:, None]  # [C, T]
    if esz == 4:
        x_ct = torch.rand((Cn, T), device="cuda", generator=g) + 1.0
        given = torch.where(live, x_ct, torch.tensor(float("nan"), device="cuda"))
    else:
        x_ct = torch.randint(1, 2 ** 62, (Cn, T), dtype=torch.int64, device="cuda", generator=g)
        given = torch.where(live, x_ct, torch.tensor(0x7FF8000000000001, dtype=torch.int64, device="cuda"))
    want = torch.where(live, x_ct, torch.zeros((), dtype=x_ct.dtype, device="cuda"))
    # channel pitch, row pitch: tight (150 is a 16-byte pitch for 8-byte elements only); 16-byte accesses on both sides (152
    # and 200 are multiples of the vector for 4 and 8 bytes), on the channel-major side only (203 is odd), on the time-major
    # side only (151 is odd), on neither
    for pitch_src, pitch_dst in ((T, Cn), (T + 2, Cn), (T + 2, Cn + 3), (T + 1, Cn), (T + 1, Cn + 3)):
        src_full, src = dev_image(Cn, T, pitch_src, x_ct.dtype, fill=0)
        src.copy_(given)
        dst_full, _ = dev_image(T, Cn, pitch_dst, x_ct.dtype, fill=3)
        got = ctx.to_time_major(src_full, T=T, count=count, out=dst_full)
        assert got.contiguous().view(torch.uint8).equal(want.t().contiguous().view(torch.uint8)), (pitch_src, pitch_dst)
        assert bool((dst_full[:, Cn:] == 3).all())
        # the other direction reads the poisoned time-major image
        tc_full, tc = dev_image(T, Cn, pitch_dst, x_ct.dtype, fill=0)
        tc.copy_(given.t())
        ct_full, _ = dev_image(Cn, T, pitch_src, x_ct.dtype, fill=3)
        got = ctx.to_channel_major(tc_full, channels=Cn, count=count, out=ct_full)
        assert got.contiguous().view(torch.uint8).equal(want.view(torch.uint8)), (pitch_src, pitch_dst)
        assert bool((ct_full[:, T:] == 3).all())


# ---- 3. index width ---------------------------------------------------------------------------------------------------------

def test_offsets_are_64_bit(ctx):
    """a pitch of 2^26 elements: c * stride (and t * ld) pass 2^32 elements from row 64 on.  The sparse image is allocated but
    only its logical region is ever written or read."""
    import torch
    big = 2 ** 26
    need = 70 * big * 4
    if torch.cuda.mem_get_info()[0] < need + (1 << 30):
        pytest.skip("needs %.1f GB of free device memory for the sparse image" % (need / 1e9))
    g = torch.Generator(device="cuda").manual_seed(3)
    sparse = torch.empty((70, big), dtype=torch.int32, device="cuda")
    small = torch.randint(-2 ** 31, 2 ** 31 - 1, (70, 64), dtype=torch.int32, device="cuda", generator=g)
    # channel-major with stride 2^26, C = 70, T = 64
    sparse[:, :64] = small
    assert torch.equal(ctx.to_time_major(sparse, T=64), small.t())
    sparse[:, :64] = 0
    got = ctx.to_channel_major(small.t().contiguous(), out=sparse)
    assert torch.equal(got, small) and torch.equal(sparse[:, :64], small)
    # time-major with ld 2^26, T = 70, C = 64: the same image read as [T][ld]
    assert torch.equal(ctx.to_channel_major(sparse, channels=64), small.t())
    sparse[:, :64] = 0
    got = ctx.to_time_major(small.t().contiguous(), out=sparse)
    assert torch.equal(got, small) and torch.equal(sparse[:, :64], small)
    del sparse


# ---- 4. grid limits -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ((3, 4194400), (4194400, 3)))
def test_more_than_65535_tiles_along_either_axis(ctx, shape):
    import torch
    Cn, T = shape
    x_ct = torch.arange(Cn * T, dtype=torch.int32, device="cuda").view(Cn, T)
    x_tc = ctx.to_time_major(x_ct)
    assert torch.equal(x_tc, x_ct.t())
    assert torch.equal(ctx.to_channel_major(x_tc.contiguous()), x_ct)


# ---- 5. host jobs ---------------------------------------------------------------------------------------------------------------

def walk(rng, Cn, T, S=50, base=20000):
    x = np.cumsum(rng.integers(-S, S + 1, (Cn, T)), axis=1) + rng.integers(base, 3 * base, Cn)[:, None]
    return np.clip(x, 0, 2 ** 31 - 1).astype(np.int32)  # [C][T]


def meter(rng, Cn, T):
    return np.round(np.abs(np.cumsum(rng.normal(0, 0.4, (Cn, T)), axis=1) + 40.0), 2).astype(np.float32)


def same_job(got, want, what):
    for g, w, name in zip(got, want, ("packed", "offsets", "bits", "err")):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name)


def sample_sets(dca, rng, Cn, T):
    x = walk(rng, Cn, T)
    return ((dca.SAMPLES_I32, 32, x), (dca.SAMPLES_BE32, 32, x.astype(">i4")), (dca.SAMPLES_I64, 40, x.astype(np.int64) * 131),
            (dca.SAMPLES_F32, 32, meter(rng, Cn, T)))


def test_encode_job_channel_major_equals_the_transposed_job(dca, ctx):
    """every sample type, tight and with a padded channel pitch ld = T + 3 (padding poisoned); decode returns [C][T]"""
    rng = np.random.default_rng(21)
    Cn, T = 37, 700
    for samples, vs, x_ct in sample_sets(dca, rng, Cn, T):
        want = ctx.encode_job(np.ascontiguousarray(x_ct.T), adaptive=1, valuesize=vs, samples=samples)
        assert (want[3] == 0).all()
        same_job(ctx.encode_job(x_ct, adaptive=1, valuesize=vs, samples=samples, layout="channel"), want, (samples, "tight"))
        padded = np.full((Cn, T + 3), 0x7F, dtype=x_ct.dtype)
        padded[:, :T] = x_ct
        same_job(ctx.encode_job(padded, adaptive=1, valuesize=vs, samples=samples, layout="channel", T=T), want, (samples, "padded"))
        # decode: what the time-major decode returns, transposed -- for the integer types the original series (a float
        # comes back as Denormalize gives it, which need not be the bits that went in)
        back_tc, derr = ctx.decode_job(want[0], want[1], want[2], T, adaptive=1, valuesize=vs, samples=samples)
        original = np.ascontiguousarray(back_tc.T)
        assert (derr == 0).all() and (samples == dca.SAMPLES_F32 or original.tobytes() == x_ct.tobytes()), samples
        back, derr = ctx.decode_job(want[0], want[1], want[2], T, adaptive=1, valuesize=vs, samples=samples, layout="channel")
        assert (derr == 0).all() and back.shape == (Cn, T) and back.tobytes() == original.tobytes(), samples
        out = np.full((Cn, T + 3), 0x7F, dtype=x_ct.dtype)
        back, derr = ctx.decode_job(want[0], want[1], want[2], T, adaptive=1, valuesize=vs, samples=samples, layout="channel", out=out)
        assert back is out and np.ascontiguousarray(out[:, :T]).tobytes() == original.tobytes() and (out[:, T:] == padded[:, T:]).all(), samples


def test_host_jobs_through_the_sixteen_byte_kernel(dca, ctx):
    """C = 1 024, T = 128: the chunk's images have 16-byte pitches on both sides, so encode and decode (with and without
    counts) take the pipeline through the kernel with 16-byte loads AND stores -- every other job shape here has an odd
    or 2-mod-4 extent on one side."""
    rng = np.random.default_rng(27)
    Cn, T = 1024, 128
    for samples, vs, x_ct in sample_sets(dca, rng, Cn, T):
        x_tc = np.ascontiguousarray(x_ct.T)
        want = ctx.encode_job(x_tc, adaptive=1, valuesize=vs, samples=samples)
        assert (want[3] == 0).all()
        back_tc, counts_tc, _ = ctx.decode_job(want[0], want[1], want[2], T + 4, adaptive=1, valuesize=vs, samples=samples, var=True)
        original = np.ascontiguousarray(back_tc[:T].T)
        assert samples == dca.SAMPLES_F32 or original.tobytes() == x_ct.tobytes()
        same_job(ctx.encode_job(x_ct, adaptive=1, valuesize=vs, samples=samples, layout="channel"), want, samples)
        back, derr = ctx.decode_job(want[0], want[1], want[2], T, adaptive=1, valuesize=vs, samples=samples, layout="channel")
        assert (derr == 0).all() and back.tobytes() == original.tobytes(), samples
        # room for T + 4 values: every channel reports T, and the four behind them come home as zero bits
        out = np.full((Cn, T + 4), 0x7F, dtype=x_ct.dtype)
        back, counts, derr = ctx.decode_job(want[0], want[1], want[2], T + 4, adaptive=1, valuesize=vs, samples=samples, var=True, layout="channel", out=out)
        assert (derr == 0).all() and (counts == T).all() and (counts == counts_tc).all(), samples
        assert np.ascontiguousarray(out[:, :T]).tobytes() == original.tobytes(), samples
        assert not np.ascontiguousarray(out[:, T:]).view(np.uint8).any(), samples


def test_every_channels_stream_is_the_oracles(dca, ctx):
    rng = np.random.default_rng(22)
    x_ct = walk(rng, 41, 300)
    packed, offsets, bits, err = ctx.encode_job(x_ct, adaptive=1, layout="channel")
    for c in range(41):
        ret, b, n = orc.encode_i32(x_ct[c], 1)
        assert ret == 0 and int(err[c]) == 0 and int(bits[c]) == n and packed[int(offsets[c]): int(offsets[c + 1])].tobytes() == b, c


def test_two_chunks_agree_with_one(dca, ctx, monkeypatch):
    """C = 8 741, T = 130 under DEGA_PIPELINE_CHUNKS=2: chunks of 8 192 and 549 channels, both layouts, against one chunk"""
    rng = np.random.default_rng(23)
    Cn, T = 8741, 130
    x_ct = walk(rng, Cn, T)
    x_tc = np.ascontiguousarray(x_ct.T)
    whole = ctx.encode_job(x_tc, adaptive=1)
    monkeypatch.setenv("DEGA_PIPELINE_CHUNKS", "2")
    try:
        same_job(ctx.encode_job(x_tc, adaptive=1), whole, "time-major, two chunks")
        same_job(ctx.encode_job(x_ct, adaptive=1, layout="channel"), whole, "channel-major, two chunks")
        back, derr = ctx.decode_job(whole[0], whole[1], whole[2], T, adaptive=1, layout="channel")
        assert (derr == 0).all() and (back == x_ct).all()
    finally:
        monkeypatch.delenv("DEGA_PIPELINE_CHUNKS")
    same_job(ctx.encode_job(x_ct, adaptive=1, layout="channel"), whole, "channel-major, one chunk")


def test_decode_var_zeroes_behind_every_count(dca, ctx):
    """streams of different lengths (every channel coded alone, by the oracle): the first count[c] values are the time-major
    decode's, the rest zero, the counts equal; the caller's pitch padding keeps its poison"""
    rng = np.random.default_rng(24)
    Cn, T = 50, 90
    lens = rng.integers(0, T + 1, Cn)
    lens[:3] = (0, T, 1)
    x = walk(rng, Cn, T)
    streams = [orc.encode_i32(x[c, : int(lens[c])], 1) for c in range(Cn)]
    assert all(s[0] == 0 for s in streams)
    bits = np.array([s[2] for s in streams], dtype=np.uint64)
    offsets = np.concatenate(([0], np.cumsum([len(s[1]) for s in streams]))).astype(np.uint64)
    packed = np.frombuffer(b"".join(s[1] for s in streams) + b"\0", dtype=np.uint8)
    t_back, t_counts, t_err = ctx.decode_job(packed, offsets, bits, T, adaptive=1, var=True)
    assert (t_counts == lens).all() and (t_err == 0).all()
    out = np.full((Cn, T + 5), 0x7B7B7B7B, dtype=np.int32)
    back, counts, err = ctx.decode_job(packed, offsets, bits, T, adaptive=1, var=True, layout="channel", out=out)
    assert (counts == t_counts).all() and (err == t_err).all()
    for c in range(Cn):
        n = int(lens[c])
        assert (out[c, :n] == t_back[:n, c]).all() and (out[c, :n] == x[c, :n]).all() and (out[c, n:T] == 0).all(), c
    assert (out[:, T:] == 0x7B7B7B7B).all()


def test_levels_channel_major_equal_time_major(dca, ctx):
    rng = np.random.default_rng(25)
    v_ct = meter(rng, 300, 130)
    levels = [1, 4, 60]
    want = ctx.encode_job_levels(np.ascontiguousarray(v_ct.T), levels, adaptive=1, factor=100.0)
    got = ctx.encode_job_levels(v_ct, levels, adaptive=1, factor=100.0, layout="channel")
    for k, N in enumerate(levels):
        same_job(got[k], want[k], N)
    # a single coarser level takes the same path (dega_hip_encode_agg_job_host)
    same_job(ctx.encode_job(v_ct, samples=dca.SAMPLES_F32, num_values=4, layout="channel"), want[1], "num_values=4")


def test_group_of_two_members(dca, ctx):
    """Group([0, 0]) really splits 1 100 channels: a member's share starts cut * ld elements into the array"""
    rng = np.random.default_rng(26)
    Cn, T = 1100, 130
    x_ct = walk(rng, Cn, T)
    v_ct = meter(rng, Cn, T)
    padded = np.full((Cn, T + 3), -1, dtype=np.int32)
    padded[:, :T] = x_ct
    want = ctx.encode_job(np.ascontiguousarray(x_ct.T), adaptive=1)
    want_levels = ctx.encode_job_levels(np.ascontiguousarray(v_ct.T), [1, 4, 60], adaptive=1)
    grp = dca.Group([0, 0])
    try:
        same_job(grp.encode_job(x_ct, adaptive=1, layout="channel"), want, "group encode")
        same_job(grp.encode_job(padded, adaptive=1, layout="channel", T=T), want, "group encode, padded")
        out = np.full((Cn, T + 3), -1, dtype=np.int32)
        back, derr = grp.decode_job(want[0], want[1], want[2], T, adaptive=1, layout="channel", out=out)
        assert (derr == 0).all() and (out == padded).all()
        got = grp.encode_job_levels(v_ct, [1, 4, 60], adaptive=1, layout="channel")
        for k in range(3):
            same_job(got[k], want_levels[k], ("group levels", k))
    finally:
        grp.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals_of_the_device_entry_points(dca, ctx):
    import torch
    L, E = dca.library(), dca.ERROR_INVALID_VALUE
    src = torch.arange(64, dtype=torch.int32, device="cuda")
    dst = torch.full((64,), POISON, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(9, dtype=torch.int64, device="cuda")
    s, d, n = src.data_ptr(), dst.data_ptr(), cnt.data_ptr()
    st = ctx._stream()
    to_time = lambda *a: L.dega_hip_to_time_major_dev(ctx._h, *a, st)  # noqa: E731  (x_ct, C, T, stride, esz, count, x_tc, ld)
    to_chan = lambda *a: L.dega_hip_to_channel_major_dev(ctx._h, *a, st)  # noqa: E731  (x_tc, C, T, ld, esz, count, x_ct, stride)
    for esz in (0, 1, 2, 3, 5, 16):
        assert to_time(s, 4, 4, 4, esz, None, d, 4) == E and to_chan(s, 4, 4, 4, esz, None, d, 4) == E
    assert to_time(s, 4, 4, 3, 4, None, d, 4) == E  # stride < T
    assert to_time(s, 4, 4, 4, 4, None, d, 3) == E  # ld < C
    assert to_chan(s, 4, 4, 3, 4, None, d, 4) == E  # ld < C
    assert to_chan(s, 4, 4, 4, 4, None, d, 3) == E  # stride < T
    assert to_time(s + 2, 4, 4, 4, 4, None, d, 4) == E and to_time(s, 4, 4, 4, 4, None, d + 1, 4) == E  # not aligned to the element
    assert to_time(s + 4, 2, 2, 2, 8, None, d, 2) == E and to_chan(s, 2, 2, 2, 8, None, d + 4, 2) == E
    assert to_time(s, 4, 4, 4, 4, n + 4, d, 4) == E and to_chan(s, 4, 4, 4, 4, n + 4, d, 4) == E  # count not aligned to 8
    assert to_time(s, 4, 4, 4, 4, None, s + 60, 4) == E and to_chan(s, 4, 4, 4, 4, None, s, 4) == E  # overlap
    assert to_time(d, 4, 4, 4, 4, None, d + 32, 4) == E  # [d, d + 64) and [d + 32, d + 96)
    assert to_time(s, 2 ** 40, 2 ** 40, 2 ** 40, 4, None, d, 2 ** 40) == E  # an image whose byte range wraps the address space
    torch.cuda.synchronize()
    assert bool((dst == POISON).all()) and torch.equal(src, torch.arange(64, dtype=torch.int32, device="cuda"))
    # nothing to do is not an error, and nothing is launched or written
    assert to_time(s, 0, 4, 4, 4, None, d, 4) == 0 and to_time(s, 4, 0, 4, 4, None, d, 4) == 0 and to_chan(None, 0, 0, 0, 4, None, None, 0) == 0
    torch.cuda.synchronize()
    assert bool((dst == POISON).all())


def test_refusals_of_the_host_jobs(dca, ctx):
    L, E = dca.library(), dca.ERROR_INVALID_VALUE
    Cn, T = 6, 9
    x = np.arange(Cn * T, dtype=np.int32).reshape(Cn, T)
    v = x.astype(np.float32)
    flag = dca.SAMPLES_CHANNEL_MAJOR
    grp = dca.Group([0])

    def outputs():
        return [np.full(4096, 0xEE, dtype=np.uint8), np.full(Cn + 1, 77, dtype=np.uint64), np.full(Cn, 77, dtype=np.uint64), np.full(Cn, 77, dtype=np.int32)]

    def untouched(o):
        return (o[0] == 0xEE).all() and (o[1][1:] == 77).all() and (o[2] == 77).all() and (o[3] == 77).all()

    try:
        for samples, arr, ld in ((dca.SAMPLES_I32 | flag, x, T - 1),           # ld < T
                                 (dca.SAMPLES_I32 | flag | 0x200, x, T),      # an unknown bit beside the flag
                                 (dca.SAMPLES_I32 | flag | 4, x, T)):         # no such sample type
            job = dca.Job(Cn, T, ld, 1, 32, samples, 100.0)
            for fn, h in ((L.dega_hip_encode_job_host, ctx._h), (L.dega_hip_group_encode, grp._h)):
                o = outputs()
                assert fn(h, C.byref(job), arr.ctypes.data, o[0].ctypes.data, o[0].size, o[1].ctypes.data, o[2].ctypes.data, o[3].ctypes.data) == E
                assert untouched(o), (samples, ld)
            for fn, h in ((L.dega_hip_decode_job_host, ctx._h), (L.dega_hip_group_decode, grp._h)):
                back = np.full((Cn, T), 5, dtype=np.int32)
                err = np.full(Cn, 77, dtype=np.int32)
                packed, offsets, bits = np.zeros(8, np.uint8), np.zeros(Cn + 1, np.uint64), np.zeros(Cn, np.uint64)
                assert fn(h, C.byref(job), packed.ctypes.data, offsets.ctypes.data, bits.ctypes.data, back.ctypes.data, None, err.ctypes.data) == E
                assert (back == 5).all() and (err == 77).all(), (samples, ld)
        # the levels forms: ld < T, and a channel-major job of another type than float32
        for samples, arr, ld in ((dca.SAMPLES_F32 | flag, v, T - 1), (dca.SAMPLES_I32 | flag, x, T)):
            job = dca.Job(Cn, T, ld, 1, 32, samples, 100.0)
            nv = (C.c_size_t * 2)(1, 4)
            for fn, h in ((L.dega_hip_encode_levels_job_host, ctx._h), (L.dega_hip_group_encode_levels, grp._h)):
                o = [outputs(), outputs()]
                ptr = lambda k: (C.c_void_p * 2)(o[0][k].ctypes.data, o[1][k].ctypes.data)  # noqa: E731
                assert fn(h, C.byref(job), nv, 2, arr.ctypes.data, ptr(0), (C.c_size_t * 2)(4096, 4096), ptr(1), ptr(2), ptr(3)) == E
                assert (o[0][0] == 0xEE).all() and (o[1][0] == 0xEE).all() and (o[0][2] == 77).all() and (o[0][3] == 77).all() and (o[0][1] == 77).all()
            o = outputs()
            assert L.dega_hip_encode_agg_job_host(ctx._h, C.byref(job), 4, arr.ctypes.data, o[0].ctypes.data, o[0].size, o[1].ctypes.data, o[2].ctypes.data,
                                                  o[3].ctypes.data) == E
            assert untouched(o) and int(o[1][0]) == 77
    finally:
        grp.close()
