"""GPU tests (-m gpu) of the `aggregate` feature (DCLib/src/aggregate.c:9-26): the aggregate kernel alone, in front of the
float-entry encoder on the device, through the host pipeline (context and groups, pageable and pinned memory) and through
the "gaggregate" row of the mirror DCCLI.  Everything is bit for bit; a NaN only has to be a NaN.

What is compared against: tests/golden/aggregate.npz (written by the compiled reference), and on random batches a strict
left-to-right float32 loop in numpy (test_aggregate_host.py pins it to the fixture and to the compiled reference) with the
oracle's restatement of normalize -> diff -> seg -> bac behind it; where oracle/_ref/libdcref.so is present the compiled
reference's own chain is asked as well."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from __graft_entry__ import load_package
from oracle import orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from agg_common import meter, same_floats, sequential  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HOST = os.path.join(ROOT, "data-compressor_amd", "host")
CLI = os.path.join(HOST, "dccli_amd")
CHAIN_CONFIGS = ((32, 1), (32, 0), (16, 1), (16, 0))


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
def golden():
    return np.load(os.path.join(GOLDEN, "aggregate.npz"))


def ref_aggregate_column(col, N):
    ret, b, n, _ = orc.ref_run_chain(np.ascontiguousarray(col).tobytes(), col.size * 32, ["encode aggregate num_values=%d" % N])
    assert ret == 0
    return np.frombuffer(b, dtype=np.float32)


def dev(v):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v)).cuda()


def float_cases(z):
    return sorted(k[:-2] for k in z.files if k.endswith(".v") and not k.startswith("chain"))


# ---- the kernel alone -------------------------------------------------------------------------------------------------------

def test_aggregate_dev_vs_fixture_both_load_paths(dca, ctx, golden):
    import torch
    for name in float_cases(golden):
        v, N, want = golden[name + ".v"], int(golden[name + ".N"]), golden[name + ".a"]
        T, Cn = v.shape
        got = ctx.aggregate(dev(v), N)  # 16-byte loads when C % 4 == 0 (torch allocations are aligned), dwords otherwise
        torch.cuda.synchronize()
        assert same_floats(got.cpu().numpy(), want), name
        # an offset base pointer: the same rows four bytes further on take the dword path
        flat = torch.zeros(T * Cn + 1, dtype=torch.float32, device="cuda")
        shifted = flat[1:].view(T, Cn)
        shifted.copy_(dev(v))
        assert shifted.data_ptr() % 16 != 0
        got = ctx.aggregate(shifted, N)
        torch.cuda.synchronize()
        assert same_floats(got.cpu().numpy(), want), name
        # ld > C and ld_out != ld: the padding columns are neither summed into a result nor written.  Where C % 4 == 0 the
        # pairs give 16-byte loads with 16-byte stores (4, 8), 16-byte loads with dword stores (4, 1: ld_out % 4 != 0) and
        # dword loads (3, 1)
        for pad, pad_out in ((4, 8), (4, 1), (3, 1)):
            wide = torch.full((T, Cn + pad), float("nan"), dtype=torch.float32, device="cuda")
            wide[:, :Cn] = dev(v)
            out = torch.full(((T + N - 1) // N, Cn + pad_out), -12345.0, dtype=torch.float32, device="cuda")
            got = ctx.aggregate(wide, N, out=out, channels=Cn)
            torch.cuda.synchronize()
            assert got.data_ptr() == out.data_ptr()
            got = got.cpu().numpy()
            assert same_floats(got[:, :Cn], want), (name, pad, pad_out)
            assert (got[:, Cn:] == np.float32(-12345.0)).all(), (name, pad, pad_out)
            ah = np.full(((T + N - 1) // N, Cn + pad_out), np.float32(-12345.0), dtype=np.float32)
            got = ctx.aggregate_host(wide.cpu().numpy(), N, out=ah, channels=Cn)
            assert same_floats(got[:, :Cn], want) and (got[:, Cn:] == np.float32(-12345.0)).all(), (name, pad, pad_out)
        # a misaligned a_tc behind aligned rows: 16-byte loads, dword stores
        if Cn % 4 == 0:
            flat = torch.full((((T + N - 1) // N) * Cn + 1,), -12345.0, dtype=torch.float32, device="cuda")
            out = flat[1:].view(-1, Cn)
            got = ctx.aggregate(dev(v), N, out=out)
            torch.cuda.synchronize()
            assert out.data_ptr() % 16 != 0 and same_floats(got.cpu().numpy(), want) and float(flat[0]) == -12345.0, name


def test_aggregate_dev_random_batches(dca, ctx):
    import torch
    rng = np.random.default_rng(314)
    shapes = [(1000, 100, 60), (1001, 257, 60), (59, 64, 60), (5, 300, 7), (2000, 1028, 2), (1801, 36, 900), (333, 1, 3), (4096, 4100, 7), (40, 2048, 1000)]
    for T, Cn, N in shapes:
        v = meter(rng, T, Cn)
        v[:, 0] *= np.where(np.arange(T) % 2 == 0, np.float32(40000.0), np.float32(-39999.0))  # order-sensitive
        want = sequential(v, N)
        got = ctx.aggregate(dev(v), N)
        torch.cuda.synchronize()
        assert got.shape == want.shape and same_floats(got.cpu().numpy(), want), (T, Cn, N)
        assert same_floats(ctx.aggregate_host(v, N), want), (T, Cn, N)
        if orc.have_ref():
            for c in (0, Cn // 2, Cn - 1):
                assert same_floats(ref_aggregate_column(v[:, c], N), want[:, c]), (T, Cn, N, c)


def test_aggregate_dev_headline_length(dca, ctx):
    """256 channels x 86 400 one-second readings -> one minute and fifteen minutes"""
    import torch
    rng = np.random.default_rng(86400)
    v = meter(rng, 86400, 256)
    vd = dev(v)
    for N in (60, 900):
        want = sequential(v, N)
        got = ctx.aggregate(vd, N)
        torch.cuda.synchronize()
        assert got.shape == (86400 // N, 256) and same_floats(got.cpu().numpy(), want), N
        if orc.have_ref():
            for c in (0, 255):
                assert same_floats(ref_aggregate_column(v[:, c], N), want[:, c]), (N, c)
    # a coarser level comes from the base series: sums of the 60-sums are other floats than the 900-sums
    assert not same_floats(sequential(sequential(v, 60), 15), sequential(v, 900))


def test_aggregate_of_one_is_not_a_copy(dca, ctx, golden):
    import torch
    v = golden["special_n1.v"].copy()
    v[np.isnan(v)] = 1.0
    got = ctx.aggregate(dev(v), 1)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    neg_zero = v.view(np.uint32) == 0x80000000
    assert neg_zero.any()
    assert (got.view(np.uint32)[neg_zero] == 0).all()  # 0.0f + -0.0f = +0.0f (aggregate.c:13,20)
    assert (got.view(np.uint32)[~neg_zero] == v.view(np.uint32)[~neg_zero]).all()  # subnormals and infinities included


# ---- in front of the coder, device pointers ------------------------------------------------------------------------------------

def check_streams(out, bits, err, want_stream, want_bits, want_err, tag):
    assert (err == want_err).all(), (tag, err, want_err)
    ok = want_err == 0
    assert (bits[ok].astype(np.uint64) == want_bits[ok]).all(), tag
    for c in np.nonzero(ok)[0]:
        nb = (int(want_bits[c]) + 7) // 8
        assert out[c, :nb].tobytes() == want_stream[c, :nb].tobytes(), (tag, c)


def test_encode_agg_f32_dev_vs_reference_chain(dca, ctx, golden):
    import torch
    for name in ("chain_meter", "chain_small", "chain_n7"):
        v, N, factor = golden[name + ".v"], int(golden[name + ".N"]), float(golden[name + ".factor"])
        for vs, ad in CHAIN_CONFIGS:
            key = "%s.vs%d.%s." % (name, vs, "ad" if ad else "st")
            out, bits, err = ctx.encode_f32(dev(v), factor=factor, adaptive=ad, valuesize=vs, num_values=N)
            torch.cuda.synchronize()
            check_streams(out.cpu().numpy(), bits.cpu().numpy(), err.cpu().numpy(), golden[key + "stream"], golden[key + "bits"], golden[key + "err"], key)
    e16 = golden["chain_small.vs16.ad.err"]  # one channel's sums leave 16 bits: it alone reports ERROR_INVALID_VALUE
    assert e16[3] == dca.ERROR_INVALID_VALUE and (np.delete(e16, 3) == 0).all()


def test_encode_agg_random_batch_and_round_trip(dca, ctx):
    """streams = the oracle's chain over the sequential sums (and the compiled reference's, where present); decode_f32 of
    them gives Denormalize(Normalize(sums)) as the oracle computes it"""
    import torch
    rng = np.random.default_rng(99)
    T, Cn, N = 3001, 130, 60
    v = meter(rng, T, Cn, top=30.0)
    sums = sequential(v, N)
    T_out = sums.shape[0]
    out, bits, err = ctx.encode_f32(dev(v), factor=100.0, adaptive=1, num_values=N)
    assert out.shape[1] == dca.worst_case_bytes(T_out)  # cap is judged against T_out
    torch.cuda.synchronize()
    o, b, e = out.cpu().numpy(), bits.cpu().numpy(), err.cpu().numpy()
    assert (e == 0).all()
    back, derr = ctx.decode_f32(out, bits, T_out, factor=100.0, adaptive=1)
    torch.cuda.synchronize()
    back = back.cpu().numpy()
    assert (derr.cpu().numpy() == 0).all()
    for c in range(Cn):
        ret, s, n = orc.encode_f32(sums[:, c], 100.0, 1)
        assert ret == 0 and int(b[c]) == n and o[c, : (n + 7) // 8].tobytes() == s, c
        ret, w = orc.decode_f32(s, n, T_out, 100.0, 1)
        assert ret == 0 and same_floats(back[:, c], w), c
    if orc.have_ref():
        for c in (0, 64, Cn - 1):
            ret, s, n, _ = orc.ref_run_chain(np.ascontiguousarray(v[:, c]).tobytes(), T * 32, [
                "encode aggregate num_values=%d" % N, "encode normalize", "encode diff", "encode seg", "encode bac adaptive"])
            assert ret == 0 and int(b[c]) == n and o[c, : (n + 7) // 8].tobytes() == s[: (n + 7) // 8], c


def test_encode_agg_calls_on_two_streams_share_the_scratch_safely(dca, ctx):
    """two calls on one context, enqueued back to back on different streams without a synchronisation in between: the
    second call's aggregate launch must not overwrite the context's scratch while the first call's encode launch reads
    it.  Both results equal those of the same calls made alone."""
    import torch
    rng = np.random.default_rng(1618)
    T, N = 21600, 2  # long channels: the first call's encode kernel runs for milliseconds, the second's aggregate for microseconds
    va, vb = dev(meter(rng, T, 2048, top=30.0)), dev(meter(rng, T, 2048, top=3000.0))
    alone = []
    for v in (va, vb):
        o, b, e = ctx.encode_f32(v, factor=100.0, adaptive=1, num_values=N)
        torch.cuda.synchronize()
        alone.append((o.clone(), b.clone(), e.clone()))
    assert not torch.equal(alone[0][0], alone[1][0])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for first, second in ((va, vb), (vb, va)):
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            r1 = ctx.encode_f32(first, factor=100.0, adaptive=1, num_values=N)
        with torch.cuda.stream(s2):
            r2 = ctx.encode_f32(second, factor=100.0, adaptive=1, num_values=N)
        torch.cuda.synchronize()
        w1, w2 = (alone[0], alone[1]) if first is va else (alone[1], alone[0])
        for got, want in ((r1, w1), (r2, w2)):
            assert (got[2] == 0).all() and torch.equal(got[1], want[1]) and torch.equal(got[0], want[0])


def test_encode_agg_of_one_equals_plain_encode(dca, ctx):
    import torch
    rng = np.random.default_rng(3)
    v = meter(rng, 500, 96, top=50.0)
    v[::7, :] = -0.0
    vd = dev(v)
    plain = ctx.encode_f32(vd, factor=100.0, adaptive=1)
    L = dca.library()
    cap = plain[0].shape[1]
    out = torch.zeros_like(plain[0])
    bits = torch.zeros_like(plain[1])
    err = torch.zeros_like(plain[2])
    ret = L.dega_hip_encode_agg_f32_dev(ctx._h, vd.data_ptr(), 96, 500, 96, 1, 100.0, 1, 32, out.data_ptr(), cap, bits.data_ptr(), err.data_ptr(), ctx._stream())
    assert ret == 0
    torch.cuda.synchronize()
    assert torch.equal(out, plain[0]) and torch.equal(bits, plain[1]) and torch.equal(err, plain[2])
    # and the explicit two-step route gives the same streams: Normalize maps both zeros to 0
    two = ctx.encode_f32(ctx.aggregate(vd, 1), factor=100.0, adaptive=1)
    torch.cuda.synchronize()
    assert torch.equal(two[0], plain[0]) and torch.equal(two[1], plain[1])


def test_refusals_launch_nothing(dca, ctx):
    import torch
    L = dca.library()
    E = dca.ERROR_INVALID_VALUE
    v = dev(meter(np.random.default_rng(1), 64, 8))
    a = torch.full((64, 8), -7.0, dtype=torch.float32, device="cuda")
    out = torch.full((8, 1024), 9, dtype=torch.uint8, device="cuda")
    bits = torch.full((8,), -5, dtype=torch.int64, device="cuda")
    err = torch.full((8,), 77, dtype=torch.int32, device="cuda")
    assert L.dega_hip_aggregate_dev(ctx._h, v.data_ptr(), 8, 64, 8, 0, a.data_ptr(), 8, ctx._stream()) == E
    assert L.dega_hip_encode_agg_f32_dev(ctx._h, v.data_ptr(), 8, 64, 8, 0, 100.0, 1, 32, out.data_ptr(), 1024, bits.data_ptr(), err.data_ptr(), ctx._stream()) == E
    # a_tc may not alias v_tc; ld_out >= C
    assert L.dega_hip_aggregate_dev(ctx._h, v.data_ptr(), 8, 64, 8, 2, v.data_ptr(), 8, ctx._stream()) == E
    assert L.dega_hip_aggregate_dev(ctx._h, v.data_ptr(), 8, 64, 8, 2, a.data_ptr(), 7, ctx._stream()) == E
    torch.cuda.synchronize()
    assert (a == -7.0).all() and (out == 9).all() and (bits == -5).all() and (err == 77).all()
    # T = 0 or C = 0: nothing is launched, DEGA_OK
    assert L.dega_hip_aggregate_dev(ctx._h, v.data_ptr(), 0, 64, 8, 2, a.data_ptr(), 8, ctx._stream()) == 0
    assert L.dega_hip_aggregate_dev(ctx._h, v.data_ptr(), 8, 0, 8, 2, a.data_ptr(), 8, ctx._stream()) == 0
    torch.cuda.synchronize()
    assert (a == -7.0).all()
    # host forms
    vh = meter(np.random.default_rng(2), 64, 8)
    ah = np.full((64, 8), -7.0, dtype=np.float32)
    assert L.dega_hip_aggregate_host(ctx._h, vh.ctypes.data, 8, 64, 8, 0, ah.ctypes.data, 8) == E
    assert (ah == -7.0).all()
    packed = np.full(4096, 9, dtype=np.uint8)
    offsets = np.full(9, 5, dtype=np.uint64)
    hbits = np.full(8, 5, dtype=np.uint64)
    herr = np.full(8, 77, dtype=np.int32)
    grp = dca.Group([0])
    try:
        for fn, h in ((L.dega_hip_encode_agg_job_host, ctx._h), (L.dega_hip_group_encode_agg, grp._h)):
            job = dca.Job(8, 64, 8, 1, 32, dca.SAMPLES_F32, 100.0)
            assert fn(h, C.byref(job), 0, vh.ctypes.data, packed.ctypes.data, packed.size, offsets.ctypes.data, hbits.ctypes.data, herr.ctypes.data) == E
            for samples in (dca.SAMPLES_I32, dca.SAMPLES_BE32, dca.SAMPLES_I64):
                job = dca.Job(8, 64, 8, 1, 32 if samples != dca.SAMPLES_I64 else 64, samples, 100.0)
                assert fn(h, C.byref(job), 2, vh.ctypes.data, packed.ctypes.data, packed.size, offsets.ctypes.data, hbits.ctypes.data, herr.ctypes.data) == E
            assert (packed == 9).all() and (hbits == 5).all() and (herr == 77).all()
    finally:
        grp.close()


# ---- host pointers: the pipeline and the groups ------------------------------------------------------------------------------------

def test_encode_job_with_num_values_equals_the_device_path(dca, ctx, monkeypatch):
    import torch
    rng = np.random.default_rng(2718)
    T, Cn, N = 240, 1100, 7  # 1 100 channels: a group of two members really splits them
    v = meter(rng, T, Cn, top=30.0)
    T_out = (T + N - 1) // N
    out, bits, err = ctx.encode_f32(dev(v), factor=100.0, adaptive=1, num_values=N)
    torch.cuda.synchronize()
    o, b, e = out.cpu().numpy(), bits.cpu().numpy().astype(np.uint64), err.cpu().numpy()
    assert (e == 0).all()
    want = [o[c, : (int(b[c]) + 7) // 8].tobytes() for c in range(Cn)]
    ret, s, n = orc.encode_f32(sequential(v[:, 17:18], N)[:, 0], 100.0, 1)
    assert ret == 0 and want[17] == s and int(b[17]) == n  # (the device path itself is pinned to the oracle above)
    pin = dca.PinnedArray((T, Cn), np.float32)
    pin.array[:] = v
    groups = [dca.Group([0]), dca.Group([0, 0])]
    try:
        for who in [ctx] + groups:
            for src in (v, pin.array):
                packed, offsets, hbits, herr = who.encode_job(src, adaptive=1, samples=dca.SAMPLES_F32, factor=100.0, num_values=N)
                assert (herr == 0).all() and (hbits == b).all()
                assert int(offsets[Cn]) == sum(len(w) for w in want) == packed.size
                for c in range(Cn):
                    assert packed[int(offsets[c]): int(offsets[c + 1])].tobytes() == want[c], c
            # packed_cap too small: ERROR_MEMORY, and offsets[C] says what is needed
            L = dca.library()
            job = dca.Job(Cn, T, Cn, 1, 32, dca.SAMPLES_F32, 100.0)
            small = np.zeros(64, dtype=np.uint8)
            offsets = np.zeros(Cn + 1, dtype=np.uint64)
            hbits = np.zeros(Cn, dtype=np.uint64)
            herr = np.zeros(Cn, dtype=np.int32)
            ret = who._enc_agg_fn()(who._handle(), C.byref(job), N, v.ctypes.data, small.ctypes.data, small.size, offsets.ctypes.data, hbits.ctypes.data, herr.ctypes.data)
            assert ret == dca.ERROR_MEMORY and int(offsets[Cn]) == sum(len(w) for w in want) and (hbits == b).all()
            # a wider host array: only the first `channels` columns are coded
            widev = np.full((T, Cn + 5), np.float32(1e30), dtype=np.float32)
            widev[:, :Cn] = v
            packed, offsets, hbits, herr = who.encode_job(widev, adaptive=1, samples=dca.SAMPLES_F32, factor=100.0, num_values=N, channels=Cn)
            assert (herr == 0).all() and (hbits == b).all() and packed[int(offsets[Cn - 1]): int(offsets[Cn])].tobytes() == want[Cn - 1]
        # the streams decode with the plain float decoder and T_out
        back, derr = ctx.decode_job(packed, offsets, hbits, T_out, adaptive=1, samples=dca.SAMPLES_F32, factor=100.0)
        ret, w = orc.decode_f32(want[17], int(b[17]), T_out, 100.0, 1)
        assert (derr == 0).all() and ret == 0 and same_floats(back[:, 17], w)
        # several chunks on several slots, on a context and on every member (a chunk is never cut below 8 192 channels, so
        # this takes a wider batch: three chunks on the context, two on each member of the pair)
        Cw = 2 * 8192 + 1100
        wv = meter(rng, 48, Cw, top=30.0)
        out, bits, err = ctx.encode_f32(dev(wv), factor=100.0, adaptive=1, num_values=N)
        torch.cuda.synchronize()
        o, wb, e = out.cpu().numpy(), bits.cpu().numpy().astype(np.uint64), err.cpu().numpy()
        assert (e == 0).all()
        nbytes = (wb + np.uint64(7)) // np.uint64(8)
        monkeypatch.setenv("DEGA_PIPELINE_CHUNKS", "3")
        for who in [ctx] + groups:
            packed, offsets, hbits, herr = who.encode_job(wv, adaptive=1, samples=dca.SAMPLES_F32, factor=100.0, num_values=N)
            assert (herr == 0).all() and (hbits == wb).all() and (np.diff(offsets) == nbytes).all() and int(offsets[Cw]) == packed.size
            for c in range(Cw):
                assert packed[int(offsets[c]): int(offsets[c + 1])].tobytes() == o[c, : int(nbytes[c])].tobytes(), c
        monkeypatch.delenv("DEGA_PIPELINE_CHUNKS")
    finally:
        for g in groups:
            g.close()
        pin.free()


# ---- the mirror DCCLI ------------------------------------------------------------------------------------------------------------

def run_cli(args):
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    return subprocess.run([CLI] + args, capture_output=True, text=True)


def test_cli_gaggregate_chain_on_the_reference_test_series(golden, tmp_path):
    with gzip.open(os.path.join(GOLDEN, "input.txt.gz"), "rb") as f:
        v = np.array(f.read().split(), dtype=np.float64).astype(np.float32)
    src = tmp_path / "in.f32"
    src.write_bytes(v.tobytes())
    out = tmp_path / "out.bin"
    p = run_cli([str(src), str(out), "encode", "gaggregate", "num_values=60", "num_channels=1"])
    assert p.returncode == 0, p.stderr
    assert same_floats(np.frombuffer(out.read_bytes(), dtype=np.float32), golden["series.a"][:, 0])
    p = run_cli([str(src), str(out), "encode", "gaggregate", "num_values=60", "num_channels=1", "#", "encode", "fdega", "adaptive"])
    assert p.returncode == 0, p.stderr
    n = int(golden["series.vs32.ad.bits"][0])
    want = golden["series.vs32.ad.stream"][0, : (n + 7) // 8].tobytes()
    assert out.read_bytes() == want  # byte-identical to `encode aggregate num_values=60 # encode normalize # ... # encode bac adaptive`
    assert "Wrote %d bytes and %d bits" % (n // 8, n % 8) in p.stdout
    if orc.have_ref():
        ret, s, nb, _ = orc.ref_run_chain(v.tobytes(), v.size * 32, ["encode aggregate num_values=60", "encode normalize", "encode diff", "encode seg",
                                                                      "encode bac adaptive"])
        assert ret == 0 and nb == n and s[: (n + 7) // 8] == want
    # 64 interleaved channels in one run = 64 single-channel runs
    T = v.size // 64
    v64 = np.ascontiguousarray(v[: T * 64].reshape(T, 64))
    src.write_bytes(v64.tobytes())
    p = run_cli([str(src), str(out), "encode", "gaggregate", "num_values=60", "num_channels=64"])
    assert p.returncode == 0, p.stderr
    sums = sequential(v64, 60)
    assert same_floats(np.frombuffer(out.read_bytes(), dtype=np.float32).reshape(-1, 64), sums)
    p = run_cli([str(src), str(out), "encode", "gaggregate", "num_values=60", "num_channels=64", "#", "encode", "fdega", "adaptive", "num_channels=64"])
    assert p.returncode == 0, p.stderr
    blob = out.read_bytes()
    assert blob[:4] == b"DEGB" and int.from_bytes(blob[8:16], "big") == 64 and int.from_bytes(blob[16:24], "big") == sums.shape[0]
    at = 24 + 8 * 64
    for c in range(64):
        n = int.from_bytes(blob[24 + 8 * c: 32 + 8 * c], "big")
        if orc.have_ref():
            ret, s, nb, _ = orc.ref_run_chain(np.ascontiguousarray(v64[:, c]).tobytes(), T * 32, [
                "encode aggregate num_values=60", "encode normalize", "encode diff", "encode seg", "encode bac adaptive"])
            s = s[: (nb + 7) // 8]
        else:
            ret, s, nb = orc.encode_f32(sums[:, c], 100.0, 1)
        assert ret == 0 and nb == n and blob[at: at + (n + 7) // 8] == s, c
        at += (n + 7) // 8
    assert at == len(blob)
    # a value count that does not divide into the channels, and a trailing partial value: as fdega treats them
    src.write_bytes(v64.tobytes()[:-4])
    assert run_cli([str(src), str(out), "encode", "gaggregate", "num_values=60", "num_channels=64"]).returncode != 0
    src.write_bytes(v.tobytes()[:-1])
    assert run_cli([str(src), str(out), "encode", "gaggregate", "num_values=60"]).returncode != 0
