"""GPU tests (-m gpu) of the float boundary of the DEGA chain across float32, through the C ABI: dega_normalize_kernel and
dega_denormalize_kernel on every value of the corpus of float_edges_common, the fused float entry of the encoder (uniform,
counted, behind the aggregate, from the host-pointer jobs, behind the csv reader) and the fused float exit of the decoder
(four groups and eight pairs) on its channel sets and integer series.  What is compared against: tests/golden/float_edges.npz
(returned by the compiled reference) and the oracle, which tests/test_float_edges_host.py pins to each other.  Integers,
statuses and streams bit for bit; a float that is a NaN only has to be a NaN."""
import os
import sys

import numpy as np
import pytest

from __graft_entry__ import load_package

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import csv_read_common as crc  # noqa: E402
import float_edges_common as fe  # noqa: E402
from agg_common import sequential  # noqa: E402

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
    return fe.EdgeFixture()


def dev_f32(bits):
    """bit patterns uint32 [T, C] as a float32 tensor on the device (no conversion touches a NaN's payload)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint32).view(np.int32)).cuda().view(torch.float32)


def host_bits(t):
    import torch
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def dev_i64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int64)).cuda()


def encoded(result):
    import torch
    torch.cuda.synchronize()
    out, bits, err = result[:3]
    return out.cpu().numpy(), bits.cpu().numpy().astype(np.uint64), err.cpu().numpy()


def decode_slabs(ctx, slabs, sbits, T, factor, ad, vs):
    import torch
    back, derr = ctx.decode_f32(torch.from_numpy(slabs).cuda(), dev_i64(sbits), T, factor, ad, valuesize=vs)
    torch.cuda.synchronize()
    return host_bits(back), derr.cpu().numpy()


@pytest.mark.parametrize("vs", [v for v in fe.VALUE_SIZES if v <= 32])
def test_normalize_and_denormalize_on_every_value(ctx, fx, vs):
    """Context.normalize / denormalize, one value per channel (T = 1) so that every value has a verdict of its own: 4 133
    channels and 4 096 (both load paths), every factor -- 1e38 and 3e38 among them at 17 and 32 bits, where readings and
    quotients are subnormal: IEEE, kept, not flushed"""
    import torch
    for factor in [f for v, f in fe.KEYS if v == vs]:
        bits, cls = fe.values(vs, factor)
        failed, fields = fx.normalized(vs, factor)
        u = fe.integers(vs)
        den = fx.denormalized(vs, factor)
        for Cn in (fe.N_VALUES, fe.N_ALIGNED):
            x, err = ctx.normalize(dev_f32(bits[:Cn].reshape(1, Cn)), factor, valuesize=vs)
            torch.cuda.synchronize()
            x, err = x.cpu().numpy().view(np.uint32)[0], err.cpu().numpy()
            wrong = np.flatnonzero(((err != 0) != failed[:Cn]) | ((err != 0) & (err != fe.INVALID)) | (~failed[:Cn] & (x != fields[:Cn].astype(np.uint32))))
            assert wrong.size == 0, (vs, factor, Cn, [(fe.CLASSES[cls[i]], hex(int(bits[i])), int(err[i]), hex(int(x[i])), bool(failed[i]), hex(int(fields[i]))) for i in wrong[:4]])
            xin = torch.from_numpy(u[:Cn].astype(np.uint32).view(np.int32).reshape(1, Cn)).cuda()
            back = host_bits(ctx.denormalize(xin, factor, valuesize=vs))[0]
            same = fe.same_float_bits(back, den[:Cn])
            assert same.all(), (vs, factor, Cn, [(hex(int(u[i])), hex(int(back[i])), hex(int(den[i]))) for i in np.flatnonzero(~same)[:4]])
    if vs in fe.HUGE_SIZES:
        sub = fe.as_f32(fx.denormalized(vs, 3e38))
        assert np.unique(sub[(sub != 0) & (np.abs(sub) < np.float32(1.17549435e-38))]).size == 6  # (+-1 .. +-3 over 3e38, compared above: all the subnormal quotients there are)


@pytest.mark.parametrize("vs,factor", fe.FUSED)
def test_fused_float_entry_and_exit(ctx, vs, factor):
    """Context.encode_f32 / decode_f32 on the channel sets, both models: status, bits and bytes per channel are the oracle's
    chain's, the floats back its inverse chain's"""
    for ad in (1, 0):
        v, kinds, want = fe.expected_channels(vs, factor, ad)
        want.check_streams(*encoded(ctx.encode_f32(dev_f32(v), factor, ad, cap=want.cap, valuesize=vs)), (vs, factor, ad), kinds)
        back, derr = decode_slabs(ctx, *want.slabs(), want.T, factor, ad, vs)
        want.check_back(back, derr, (vs, factor, ad), kinds)


def test_reference_streams_of_the_fixture(ctx, fx):
    """the thin sample of the channel sets that went through the compiled reference, against the device directly"""
    for vs, factor in fe.FUSED_IN_FIXTURE:
        for ad in (1, 0):
            k = "%s.%s.chain" % (fe.key(vs, factor), "ad" if ad else "st")
            idx, werr, wbits, wstream = (fx.z[k + s] for s in (".idx", ".err", ".bits", ".stream"))
            v, kinds = fe.channels(vs, factor)
            out, bits, err = encoded(ctx.encode_f32(dev_f32(v[:, idx]), factor, ad, cap=fe.stream_cap(v.shape[0], vs), valuesize=vs))
            assert (err == werr).all() and (bits[werr == 0] == wbits[werr == 0]).all(), (vs, factor, ad)
            for j in np.flatnonzero(werr == 0):
                nb = (int(wbits[j]) + 7) // 8
                assert out[j, :nb].tobytes() == wstream[j, :nb].tobytes(), (vs, factor, ad, int(idx[j]), kinds[idx[j]])


@pytest.mark.parametrize("vs", fe.FUSED_SIZES)
def test_float_exit_on_integer_series(ctx, vs):
    """the decoder's row write on integers over the whole range of the value size: sign extension, (float)int64 above 2^24
    (integers exactly between two floats among them), the division -- by 100, by 1, and by 3e38, where the
    quotients of +-1 .. +-3 are subnormal and kept"""
    for factor, ad in ((100.0, 1), (1.0, 0), (3e38, 1)):
        want = fe.expected_series(vs, ad, factor)
        back, derr = decode_slabs(ctx, want.slabs, want.bits, want.T, factor, ad, vs)
        want.check_back(back, derr, (vs, factor, ad))


@pytest.mark.parametrize("vs,factor", [(32, 100.0), (17, 3.3), (26, 0.5), (40, -100.0), (64, 100.0)])
def test_counted_float_entry(ctx, vs, factor):
    """count=: counts 1 .. T; an infinity, a value out of range or a NaN behind a channel's count changes no verdict"""
    v, count = fe.counts_and_poison(vs, factor)
    for ad in (1, 0):
        want = fe.Expected(v, vs, ad, factor, count=count)
        assert (want.err == 0).all()
        want.check_streams(*encoded(ctx.encode_f32(dev_f32(v), factor, ad, cap=want.cap, valuesize=vs, count=dev_i64(count))), (vs, factor, ad, "counted"))


def test_sums_of_two_with_a_nan_and_an_infinity(ctx):
    """num_values=2 in front of the float entry: a channel with a NaN reading has a NaN sum, which is coded as 0; a channel
    with +inf has an infinite sum, which is ERROR_INVALID_VALUE; their neighbours are untouched"""
    bits, cls = fe.values(32, 100.0)
    small = bits[(cls == fe.CLASSES.index("printed")) & (fe.as_f32(bits) > 0)]
    v = np.ascontiguousarray(np.resize(small, fe.T_ROWS * 70).reshape(fe.T_ROWS, 70))
    v[5, 3], v[8, 66] = 0x7FC00000, 0x7F800000
    sums = fe.as_bits(sequential(fe.as_f32(v).reshape(v.shape), 2))
    assert np.isnan(fe.as_f32(sums[2, 3])) and np.isinf(fe.as_f32(sums[4, 66]))
    for ad in (1, 0):
        want = fe.Expected(sums, 32, ad, 100.0)
        assert [c for c in range(70) if want.err[c] != 0] == [66] and int(want.err[66]) == fe.INVALID
        # (the NaN sum is the field 0: the channel's stream is that of the sums with a 0.0 in its place)
        zeroed = sums.copy()
        zeroed[2, 3] = 0
        assert fe.encode_chain(zeroed[:, 3], 32, ad, 100.0) == (0, want.streams[3], int(want.bits[3]))
        want.check_streams(*encoded(ctx.encode_f32(dev_f32(v), 100.0, ad, cap=want.cap, valuesize=32, num_values=2)), ("num_values=2", ad))


def test_eight_pair_decoder(dca, monkeypatch):
    """DEGA_WAVES_PER_WORKGROUP=8 on a fresh context: the float exit of the workgroups of eight pairs of waves, on the
    channel sets and the integer series below 33 bits"""
    monkeypatch.setenv("DEGA_WAVES_PER_WORKGROUP", "8")
    wide = dca.Context(0)
    try:
        for vs, factor, ad in ((32, 100.0, 1), (32, -100.0, 0), (17, 3.3, 1), (26, 0.5, 0)):
            v, kinds, want = fe.expected_channels(vs, factor, ad)
            back, derr = decode_slabs(wide, *want.slabs(), want.T, factor, ad, vs)
            want.check_back(back, derr, (vs, factor, ad, "eight pairs"), kinds)
        for vs, factor, ad in ((32, 100.0, 1), (32, 3e38, 1), (17, 1.0, 0), (26, 100.0, 1)):
            want = fe.expected_series(vs, ad, factor)
            back, derr = decode_slabs(wide, want.slabs, want.bits, want.T, factor, ad, vs)
            want.check_back(back, derr, (vs, factor, ad, "eight pairs"))
    finally:
        wide.close()


@pytest.mark.parametrize("vs", (32, 64))
def test_host_jobs_with_float_samples(dca, ctx, vs):
    """encode_job / decode_job with SAMPLES_F32 on a context and on a group of two: what the device-pointer path gives"""
    factor, ad = 100.0, 1
    v, kinds, want = fe.expected_channels(vs, factor, ad)
    samples = fe.as_f32(v).reshape(v.shape)
    group = dca.Group([0, 0])
    try:
        for who in (ctx, group):
            packed, offsets, bits, err = who.encode_job(samples, adaptive=ad, valuesize=vs, samples=dca.SAMPLES_F32, factor=factor)
            assert fe.as_bits(samples).tobytes() == v.tobytes()  # (the job took the array as it is)
            assert (err == want.err).all(), (vs, who)
            for c in np.flatnonzero(want.err == 0):
                assert int(bits[c]) == int(want.bits[c]) and packed[int(offsets[c]): int(offsets[c + 1])].tobytes() == want.streams[c], (vs, int(c), kinds[c])
            back, derr = who.decode_job(packed, offsets, bits, want.T, adaptive=ad, valuesize=vs, samples=dca.SAMPLES_F32, factor=factor)
            want.check_back(fe.as_bits(back).reshape(back.shape), derr, (vs, "decode_job"), kinds)
    finally:
        group.close()


def test_one_chain_from_text(ctx, fx):
    """lines `nan`, `-nan`, `inf`, `1e-40`, `abc` and ordinary readings through csv_read into encode_f32: the reference's
    `decode csv # encode normalize # encode diff # encode seg # encode bac [adaptive]` on the same texts"""
    import torch
    texts = [crc.lines_text(lines) for lines in fe.TEXT_LINES]
    rows, lens = crc.pack(texts)
    max_T = max(len(lines) for lines in fe.TEXT_LINES)
    v, count, rerr = ctx.csv_read(torch.from_numpy(np.ascontiguousarray(rows)).cuda(), dev_i64(lens), max_T)
    torch.cuda.synchronize()
    assert (rerr.cpu().numpy() == 0).all() and count.cpu().numpy().tolist() == [len(lines) for lines in fe.TEXT_LINES]
    for vs in fe.TEXT_SIZES:
        for ad in (1, 0):
            k = "text.n%d.%s" % (vs, "ad" if ad else "st")
            werr, wbits, wstream = fx.z[k + ".err"], fx.z[k + ".bits"], fx.z[k + ".stream"]
            out, bits, err = encoded(ctx.encode_f32(v, 100.0, ad, cap=fe.stream_cap(max_T, vs), valuesize=vs, count=count))
            assert (err == werr).all() and (werr == 0).sum() >= 6 and (werr != 0).sum() >= 2, (vs, ad, err, werr)
            for c in np.flatnonzero(werr == 0):
                nb = (int(wbits[c]) + 7) // 8
                assert int(bits[c]) == int(wbits[c]) and out[c, :nb].tobytes() == wstream[c, :nb].tobytes(), (vs, ad, int(c))
