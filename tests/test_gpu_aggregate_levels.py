"""GPU tests (-m gpu) of several granularities from one pass over the base series: the multi-level aggregate kernel alone,
in front of the float-entry encoder on the device, and through the host pipeline (context and groups, pageable and pinned
memory).  Everything is bit for bit; a NaN only has to be a NaN.

What is compared against: tests/golden/aggregate_levels.npz (written by the compiled reference, one run of `encode
aggregate num_values=N` per level), the single-level calls of the library (Context.aggregate, encode_f32(num_values=N),
encode_job(num_values=N): their own tests pin them to the reference), and a strict left-to-right float32 loop in numpy."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from __graft_entry__ import load_package

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from agg_common import meter, same_floats, sequential  # noqa: E402
from agg_levels_common import CHAIN_CONFIGS, Fixture  # noqa: E402

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


def dev(v):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v)).cuda()


def rows_of(T, N):
    return (T + N - 1) // N


# ---- the kernel alone -------------------------------------------------------------------------------------------------------

@pytest.fixture(params=["planned", "shared"])
def sharing(request, monkeypatch):
    """the fixture series are narrow, so the planner gives every level a pass of its own (the single-level kernel); "shared"
    lowers the planner's workgroup floor through its test knob so that the same cases run through the multi-level kernel,
    the eight-level set through its K = 8 form"""
    if request.param == "shared":
        monkeypatch.setenv("DEGA_AGG_LEVELS_MIN_WORKGROUPS", "1")
    return request.param


def test_aggregate_levels_vs_fixture_both_load_paths(dca, ctx, fx, sharing):
    import torch
    n = 0
    for name, levels in fx.cases():
        if sharing == "shared":
            assert len(dca.aggregate_levels_plan(fx.series(name).shape[1], fx.series(name).shape[0], levels)[1]) == 1
        v = fx.series(name)
        T, Cn = v.shape
        got = ctx.aggregate_levels(dev(v), levels)  # 16-byte loads when C % 4 == 0 (torch allocations are aligned)
        torch.cuda.synchronize()
        for k, N in enumerate(levels):
            assert same_floats(got[k].cpu().numpy(), fx.sums(name, N)), (name, levels, N)
        # the same rows four bytes further on take the dword path
        flat = torch.zeros(T * Cn + 1, dtype=torch.float32, device="cuda")
        shifted = flat[1:].view(T, Cn)
        shifted.copy_(dev(v))
        assert shifted.data_ptr() % 16 != 0
        got = ctx.aggregate_levels(shifted, levels)
        torch.cuda.synchronize()
        for k, N in enumerate(levels):
            assert same_floats(got[k].cpu().numpy(), fx.sums(name, N)), (name, levels, N, "dword")
        # ld > C and a pitch of its own per level (16-byte stores, dword stores behind 16-byte loads, ...): the padding
        # columns are neither summed into a result nor written
        wide = torch.full((T, Cn + 4), float("nan"), dtype=torch.float32, device="cuda")
        wide[:, :Cn] = dev(v)
        outs = [torch.full((rows_of(T, N), Cn + (8, 1, 4, 3)[k % 4]), -12345.0, dtype=torch.float32, device="cuda") for k, N in enumerate(levels)]
        got = ctx.aggregate_levels(wide, levels, channels=Cn, out=outs)
        torch.cuda.synchronize()
        for k, N in enumerate(levels):
            g = got[k].cpu().numpy()
            assert got[k].data_ptr() == outs[k].data_ptr()
            assert same_floats(g[:, :Cn], fx.sums(name, N)) and (g[:, Cn:] == np.float32(-12345.0)).all(), (name, levels, N, "pitches")
        n += 1
    assert n >= 40


def test_aggregate_levels_equal_the_single_level_calls(dca, ctx):
    """random batches that the plan puts in one pass, in two passes and in K passes"""
    import torch
    rng = np.random.default_rng(2024)
    for (T, Cn), sets in (((3600, 4096), ([2, 4, 7, 14, 28], [28, 2, 900, 4], [899, 900, 901], [60, 300, 900])),
                          ((1801, 300), ([3, 1], [1, 2, 900], [7, 11, 13]))):
        v = meter(rng, T, Cn)
        v[:, 0] *= np.where(np.arange(T) % 2 == 0, np.float32(40000.0), np.float32(-39999.0))  # order-sensitive
        vd = dev(v)
        kinds = set()
        for levels in sets:
            pass_of, step_of = dca.aggregate_levels_plan(Cn, T, levels, True)
            kinds.add("one" if len(step_of) == 1 else ("each alone" if len(step_of) == len(levels) else "two" if len(step_of) == 2 else "more"))
            got = ctx.aggregate_levels(vd, levels)
            torch.cuda.synchronize()
            for k, N in enumerate(levels):
                alone = ctx.aggregate(vd, N)
                torch.cuda.synchronize()
                assert got[k].shape == alone.shape and same_floats(got[k].cpu().numpy(), alone.cpu().numpy()), (T, Cn, levels, N)
            assert same_floats(got[0][:, :3].cpu().numpy(), sequential(v[:, :3], levels[0])), (T, Cn, levels)
        assert kinds == {"one", "two", "each alone"}, kinds


def test_aggregate_levels_headline_length(dca, ctx):
    """2 048 channels x 86 400 one-second readings -> one minute, five minutes, a quarter of an hour, an hour"""
    import torch
    rng = np.random.default_rng(86401)
    levels = [60, 300, 900, 3600]
    v = meter(rng, 86400, 2048)
    vd = dev(v)
    assert len(dca.aggregate_levels_plan(2048, 86400, levels)[1]) < len(levels)  # at least two of them share a pass
    got = ctx.aggregate_levels(vd, levels)
    torch.cuda.synchronize()
    cols = np.sort(rng.choice(2048, size=64, replace=False))
    for k, N in enumerate(levels):
        g = got[k].cpu().numpy()
        assert g.shape == (86400 // N, 2048)
        assert same_floats(g[:, cols], sequential(np.ascontiguousarray(v[:, cols]), N)), N
        alone = ctx.aggregate(vd, N)
        torch.cuda.synchronize()
        assert same_floats(g, alone.cpu().numpy()), N


# ---- in front of the coder, device pointers ------------------------------------------------------------------------------------

def check_streams(out, bits, err, want_stream, want_bits, want_err, tag):
    assert (err == want_err).all(), (tag, err, want_err)
    ok = want_err == 0
    assert (bits[ok].astype(np.uint64) == want_bits[ok]).all(), tag
    for c in np.nonzero(ok)[0]:
        nb = (int(want_bits[c]) + 7) // 8
        assert out[c, :nb].tobytes() == want_stream[c, :nb].tobytes(), (tag, c)


def test_encode_f32_levels_vs_reference_chains(dca, ctx, fx, sharing):
    import torch
    seen = 0
    for name, factor, Ns in fx.chains():
        v = fx.series(name)
        vd = dev(v)
        for vs, ad in CHAIN_CONFIGS:
            res = ctx.encode_f32_levels(vd, Ns, factor=factor, adaptive=ad, valuesize=vs)
            torch.cuda.synchronize()
            for k, N in enumerate(Ns):
                out, bits, err = (t.cpu().numpy() for t in res[k])
                check_streams(out, bits, err, *fx.chain(name, N, vs, ad), (name, N, vs, ad))
                # ... and the single-level call gives the same tensors
                o1, b1, e1 = ctx.encode_f32(vd, factor=factor, adaptive=ad, valuesize=vs, num_values=N)
                torch.cuda.synchronize()
                assert torch.equal(res[k][0], o1) and torch.equal(res[k][1], b1) and torch.equal(res[k][2], e1), (name, N, vs, ad)
                seen += 1
    assert seen >= 32
    e16 = fx.chain("meter3601", 3600, 16, 1)[2]
    assert (e16 == dca.ERROR_INVALID_VALUE).all()  # an hour of these readings leaves 16 bits: the fixture holds failing channels too


def test_encode_f32_levels_round_trip(dca, ctx):
    import torch
    rng = np.random.default_rng(100)
    T, Cn, levels = 3001, 130, [60, 7, 300]
    v = meter(rng, T, Cn, top=30.0)
    res = ctx.encode_f32_levels(dev(v), levels, factor=100.0, adaptive=1)
    torch.cuda.synchronize()
    for k, N in enumerate(levels):
        out, bits, err = res[k]
        T_out = rows_of(T, N)
        assert out.shape[1] == dca.worst_case_bytes(T_out) and (err == 0).all()
        back, derr = ctx.decode_f32(out, bits, T_out, factor=100.0, adaptive=1)
        want, _ = ctx.decode_f32(*ctx.encode_f32(dev(sequential(v, N)), factor=100.0, adaptive=1)[:2], T_out, factor=100.0, adaptive=1)
        torch.cuda.synchronize()
        assert (derr == 0).all() and same_floats(back.cpu().numpy(), want.cpu().numpy()), N


def test_encode_levels_calls_on_two_streams_share_the_scratch_safely(dca, ctx):
    """the pattern of the single-level test: two calls on one context, back to back on different streams without a
    synchronisation in between; both results equal those of the same calls made alone"""
    import torch
    rng = np.random.default_rng(1619)
    T, levels = 21600, [2, 60]
    va, vb = dev(meter(rng, T, 2048, top=30.0)), dev(meter(rng, T, 2048, top=3000.0))
    alone = []
    for v in (va, vb):
        res = ctx.encode_f32_levels(v, levels, factor=100.0, adaptive=1)
        torch.cuda.synchronize()
        alone.append([(o.clone(), b.clone(), e.clone()) for o, b, e in res])
    assert not torch.equal(alone[0][0][0], alone[1][0][0])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for first, second in ((va, vb), (vb, va)):
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            r1 = ctx.encode_f32_levels(first, levels, factor=100.0, adaptive=1)
        with torch.cuda.stream(s2):
            r2 = ctx.encode_f32_levels(second, levels, factor=100.0, adaptive=1)
        torch.cuda.synchronize()
        w1, w2 = (alone[0], alone[1]) if first is va else (alone[1], alone[0])
        for got, want in ((r1, w1), (r2, w2)):
            for k in range(len(levels)):
                assert (got[k][2] == 0).all() and torch.equal(got[k][1], want[k][1]) and torch.equal(got[k][0], want[k][0])


def test_encode_levels_with_a_level_of_one(dca, ctx):
    import torch
    rng = np.random.default_rng(4)
    v = meter(rng, 500, 96, top=50.0)
    v[::7, :] = -0.0
    vd = dev(v)
    res = ctx.encode_f32_levels(vd, [1, 60], factor=100.0, adaptive=1)
    plain = ctx.encode_f32(vd, factor=100.0, adaptive=1)
    coarse = ctx.encode_f32(vd, factor=100.0, adaptive=1, num_values=60)
    torch.cuda.synchronize()
    for got, want in ((res[0], plain), (res[1], coarse)):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])


def test_refusals_launch_nothing(dca, ctx):
    import torch
    L = dca.library()
    E = dca.ERROR_INVALID_VALUE
    s = ctx._stream()
    v = dev(meter(np.random.default_rng(1), 64, 8))
    a = [torch.full((64, 8), -7.0, dtype=torch.float32, device="cuda") for _ in range(9)]
    out = [torch.full((8, 1024), 9, dtype=torch.uint8, device="cuda") for _ in range(2)]
    bits = [torch.full((8,), -5, dtype=torch.int64, device="cuda") for _ in range(2)]
    err = [torch.full((8,), 77, dtype=torch.int32, device="cuda") for _ in range(2)]
    ptrs = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    sizes = lambda *n: (C.c_size_t * len(n))(*n)  # noqa: E731

    def agg(levels, outs, lds, Cn=8, ld=8, vp=None):
        return L.dega_hip_aggregate_levels_dev(ctx._h, vp or v.data_ptr(), Cn, 64, ld, sizes(*levels), len(levels), ptrs(outs), sizes(*lds), s)
    assert agg([2, 0], a[:2], [8, 8]) == E  # a level of 0
    assert agg([4, 4], a[:2], [8, 8]) == E  # the same N twice
    assert agg(list(range(1, 10)), a, [8] * 9) == E  # more than 8 levels
    assert agg([2, 4], a[:2], [8, 7]) == E  # ld_out < C
    assert agg([2, 4], a[:2], [8, 8], ld=7) == E  # ld < C
    assert agg([2, 4], [a[0], a[0]], [8, 8]) == E  # two levels into one array
    assert agg([2, 4], [a[0], v], [8, 8]) == E  # an output over v_tc
    assert agg([2, 4], [a[0], a[1].view(-1)[1:]], [8, 8], vp=v.data_ptr() + 2) == E  # misaligned rows
    assert L.dega_hip_aggregate_levels_dev(ctx._h, v.data_ptr(), 8, 64, 8, sizes(2, 4), 2, None, sizes(8, 8), s) == E
    assert "aggregate levels" in ctx.last_error()

    def enc(levels, caps=(1024, 1024), vs=32):
        return L.dega_hip_encode_levels_f32_dev(ctx._h, v.data_ptr(), 8, 64, 8, sizes(*levels), len(levels), 100.0, 1, vs, ptrs(out), sizes(*caps), ptrs(bits),
                                                ptrs(err), s)
    assert enc([2, 0]) == E and enc([4, 4]) == E
    assert enc([2, 4], caps=(1024, 1022)) == E  # the second level's cap is no multiple of 4: refused before the first level is launched
    assert enc([2, 4], vs=0) == E
    torch.cuda.synchronize()
    assert all((t == -7.0).all() for t in a) and all((t == 9).all() for t in out) and all((t == -5).all() for t in bits) and all((t == 77).all() for t in err)
    # K = 0, C = 0 or T = 0: nothing is launched, DEGA_OK
    assert L.dega_hip_aggregate_levels_dev(ctx._h, v.data_ptr(), 8, 64, 8, None, 0, None, None, s) == 0
    assert agg([2, 4], a[:2], [8, 8], Cn=0) == 0
    assert L.dega_hip_aggregate_levels_dev(ctx._h, v.data_ptr(), 8, 0, 8, sizes(2, 4), 2, ptrs(a[:2]), sizes(8, 8), s) == 0
    torch.cuda.synchronize()
    assert all((t == -7.0).all() for t in a)
    # host forms: samples other than float32, bad level lists
    vh = meter(np.random.default_rng(2), 64, 8)
    packed = [np.full(4096, 9, dtype=np.uint8) for _ in range(2)]
    offsets = [np.full(9, 5, dtype=np.uint64) for _ in range(2)]
    hbits = [np.full(8, 5, dtype=np.uint64) for _ in range(2)]
    herr = [np.full(8, 77, dtype=np.int32) for _ in range(2)]
    hp = lambda arrs: (C.c_void_p * len(arrs))(*[x.ctypes.data for x in arrs])  # noqa: E731
    grp = dca.Group([0])
    try:
        for fn, h in ((L.dega_hip_encode_levels_job_host, ctx._h), (L.dega_hip_group_encode_levels, grp._h)):
            def call(job, levels):
                return fn(h, C.byref(job), sizes(*levels), len(levels), vh.ctypes.data, hp(packed), sizes(4096, 4096), hp(offsets), hp(hbits), hp(herr))
            f32 = dca.Job(8, 64, 8, 1, 32, dca.SAMPLES_F32, 100.0)
            assert call(f32, [2, 0]) == E and call(f32, [4, 4]) == E and call(f32, list(range(1, 10))) == E
            assert call(dca.Job(8, 64, 7, 1, 32, dca.SAMPLES_F32, 100.0), [2, 4]) == E
            for samples in (dca.SAMPLES_I32, dca.SAMPLES_BE32, dca.SAMPLES_I64):
                assert call(dca.Job(8, 64, 8, 1, 32 if samples != dca.SAMPLES_I64 else 64, samples, 100.0), [2, 4]) == E
            assert all((p == 9).all() for p in packed) and all((b == 5).all() for b in hbits) and all((e == 77).all() for e in herr)
    finally:
        grp.close()


# ---- host pointers: the pipeline and the groups ------------------------------------------------------------------------------------

def assert_same_job(got, want, tag):
    for x, y in zip(got, want):
        assert x.shape == y.shape and (x == y).all(), tag


def test_encode_job_levels_equals_the_single_level_jobs(dca, ctx, monkeypatch):
    """pageable and pinned samples, a context and groups of one and two members, a wider batch under the chunk knob"""
    rng = np.random.default_rng(2719)
    T, Cn, levels = 240, 1100, [7, 1, 60, 2]  # 1 100 channels: a group of two members really splits them
    v = meter(rng, T, Cn, top=30.0)
    want = [ctx.encode_job(v, adaptive=1, samples=dca.SAMPLES_F32, factor=100.0, num_values=N) for N in levels]
    pin = dca.PinnedArray((T, Cn), np.float32)
    pin.array[:] = v
    groups = [dca.Group([0]), dca.Group([0, 0])]
    try:
        for who in [ctx] + groups:
            for src in (v, pin.array):
                got = who.encode_job_levels(src, levels, adaptive=1, factor=100.0)
                for k, N in enumerate(levels):
                    assert (got[k][3] == 0).all()
                    assert_same_job(got[k], want[k], (type(who).__name__, N))
            # a wider host array: only the first `channels` columns are coded
            widev = np.full((T, Cn + 5), np.float32(1e30), dtype=np.float32)
            widev[:, :Cn] = v
            got = who.encode_job_levels(widev, levels, adaptive=1, factor=100.0, channels=Cn)
            for k, N in enumerate(levels):
                assert_same_job(got[k], want[k], (type(who).__name__, N, "channels"))
        # the knob the pipeline's own measurements use, on a wider batch and a static model (2 600 channels are still one
        # chunk -- none is narrower than min(C, 8192) channels; several chunks: test_gpu_pipeline_chunks.py)
        monkeypatch.setenv("DEGA_PIPELINE_CHUNKS", "3")
        wide = meter(rng, 96, 2600, top=30.0)
        got = ctx.encode_job_levels(wide, [2, 12, 5], adaptive=0, valuesize=16, factor=10.0)
        monkeypatch.delenv("DEGA_PIPELINE_CHUNKS")
        for k, N in enumerate([2, 12, 5]):
            assert_same_job(got[k], ctx.encode_job(wide, adaptive=0, valuesize=16, samples=dca.SAMPLES_F32, factor=10.0, num_values=N), ("chunks", N))
        # the streams decode with the plain float decoder and each level's row count
        for k, N in enumerate(levels):
            packed, offsets, bits, _ = want[k]
            back, derr = ctx.decode_job(packed, offsets, bits, rows_of(T, N), adaptive=1, samples=dca.SAMPLES_F32, factor=100.0)
            assert (derr == 0).all() and np.abs(back - sequential(v, N)).max() <= 0.02 * N + 0.01, N
    finally:
        for g in groups:
            g.close()
        pin.free()


def test_encode_job_levels_stream_longer_than_the_usual_slab(dca, ctx):
    """one channel of wide noise: its streams are longer than its samples, so they outgrow the slab of the first attempt at
    every level, and that level of the chunk is redone with worst-case slabs; every channel still codes without an error
    (non-negative, and the sums of eight such values stay inside 32 bits), so every byte of the result is defined"""
    rng = np.random.default_rng(5)
    T, Cn, levels = 4000, 1100, [2, 1, 8]  # 1 100 channels: a group of two members really splits them
    v = meter(rng, T, Cn, top=30.0)
    v[:, 77] = rng.integers(0, 2 ** 26, T).astype(np.float32)
    v[:, 900] = rng.integers(0, 2 ** 26, T).astype(np.float32)  # one in each member's range
    grp = dca.Group([0, 0])
    try:
        for ad in (0, 1):
            want = [ctx.encode_job(v, adaptive=ad, samples=dca.SAMPLES_F32, factor=1.0, num_values=N) for N in levels]
            for k, N in enumerate(levels):
                assert (want[k][3] == 0).all(), (ad, N)
                for c in (77, 900):  # the case is what it claims to be: longer than the usual slab
                    assert int(want[k][1][c + 1] - want[k][1][c]) > 4 * rows_of(T, N) + 64, (ad, N, c)
            for who in (ctx, grp):
                got = who.encode_job_levels(v, levels, adaptive=ad, factor=1.0)
                for k, N in enumerate(levels):
                    assert_same_job(got[k], want[k], (type(who).__name__, ad, N))
    finally:
        grp.close()


def test_group_member_whose_share_outgrows_its_own_buffer(dca, ctx):
    """every channel is noise, so each member's share of a level is longer than the host buffer the member starts with (the
    usual slab size per channel) while it fits the caller's: the member runs once more with what it asked for.  Decided level
    by level: when another level's packed_cap really is too small, that one reports its size and this one is still delivered"""
    rng = np.random.default_rng(7)
    T, Cn, levels = 4000, 1100, [2, 8]
    v = rng.integers(0, 2 ** 26, (T, Cn)).astype(np.float32)
    want = [ctx.encode_job(v, adaptive=1, samples=dca.SAMPLES_F32, factor=1.0, num_values=N) for N in levels]
    for k, N in enumerate(levels):
        assert (want[k][3] == 0).all() and want[k][0].size > Cn * (4 * rows_of(T, N) + 64 + 3), N  # longer than every member's first buffer
    grp = dca.Group([0, 0])
    try:
        got = grp.encode_job_levels(v, levels, adaptive=1, factor=1.0, packed_cap=[w[0].size for w in want])
        for k, N in enumerate(levels):
            assert_same_job(got[k], want[k], N)
        L = dca.library()
        K = len(levels)
        caps = [want[0][0].size, want[1][0].size - 1]
        packed = [np.zeros(c, dtype=np.uint8) for c in caps]
        offsets = [np.zeros(Cn + 1, dtype=np.uint64) for _ in range(K)]
        bits = [np.zeros(Cn, dtype=np.uint64) for _ in range(K)]
        err = [np.zeros(Cn, dtype=np.int32) for _ in range(K)]
        hp = lambda arrs: (C.c_void_p * K)(*[x.ctypes.data for x in arrs])  # noqa: E731
        job = dca.Job(Cn, T, Cn, 1, 32, dca.SAMPLES_F32, 1.0)
        ret = L.dega_hip_group_encode_levels(grp._h, C.byref(job), (C.c_size_t * K)(*levels), K, v.ctypes.data, hp(packed), (C.c_size_t * K)(*caps), hp(offsets),
                                             hp(bits), hp(err))
        assert ret == dca.ERROR_MEMORY
        for k in range(K):
            assert (offsets[k] == want[k][1]).all() and (bits[k] == want[k][2]).all() and (err[k] == 0).all(), k
        assert (packed[0] == want[0][0]).all()  # the level that fits is delivered
    finally:
        grp.close()


def test_encode_job_levels_one_packed_cap_too_small(dca, ctx):
    rng = np.random.default_rng(6)
    T, Cn, levels = 240, 1100, [2, 60, 7]
    v = meter(rng, T, Cn, top=30.0)
    want = [ctx.encode_job(v, adaptive=1, samples=dca.SAMPLES_F32, factor=100.0, num_values=N) for N in levels]
    groups = [dca.Group([0, 0])]
    try:
        for who in [ctx] + groups:
            caps = [want[0][0].size, want[1][0].size - 1, want[2][0].size + 100]
            with pytest.raises(dca.DegaError) as e:
                who.encode_job_levels(v, levels, adaptive=1, factor=100.0, packed_cap=caps)
            assert e.value.code == dca.ERROR_MEMORY
            # through the C ABI: the level that does not fit reports its size, the others are delivered
            L = dca.library()
            fn = L.dega_hip_encode_levels_job_host if who is ctx else L.dega_hip_group_encode_levels
            K = len(levels)
            packed = [np.zeros(max(1, c), dtype=np.uint8) for c in caps]
            offsets = [np.zeros(Cn + 1, dtype=np.uint64) for _ in range(K)]
            bits = [np.zeros(Cn, dtype=np.uint64) for _ in range(K)]
            err = [np.zeros(Cn, dtype=np.int32) for _ in range(K)]
            hp = lambda arrs: (C.c_void_p * K)(*[x.ctypes.data for x in arrs])  # noqa: E731
            job = dca.Job(Cn, T, Cn, 1, 32, dca.SAMPLES_F32, 100.0)
            ret = fn(who._handle(), C.byref(job), (C.c_size_t * K)(*levels), K, v.ctypes.data, hp(packed), (C.c_size_t * K)(*caps), hp(offsets), hp(bits), hp(err))
            assert ret == dca.ERROR_MEMORY
            for k in range(K):
                assert int(offsets[k][Cn]) == want[k][0].size and (offsets[k] == want[k][1]).all() and (bits[k] == want[k][2]).all(), k
            for k in (0, 2):
                assert (packed[k][: want[k][0].size] == want[k][0]).all(), k
    finally:
        for g in groups:
            g.close()
