"""Diff and exp-Golomb at every codeword length, on the GPU (tests/seg_ladder_common.py has the corpus, its conditions and the
checkers): the entry points that end in the encode kernel's filling wave held to the oracle's stage chain on status, bit
length and every byte, and the decoders -- given the oracle's streams, never the kernels' -- on status, count and every
sample.  390 channels (two `plain` waves, every kind at every pad, a ragged wave) of at most 282 rows per launch; the
oracle's work is done once per value size and model and shared."""
import numpy as np
import pytest

import seg_ladder_common as sl
from __graft_entry__ import load_package
from oracle import orc

pytestmark = pytest.mark.gpu

NARROW = tuple(vs for vs in sl.SIZES if vs <= 32)
WIDE = tuple(vs for vs in sl.SIZES if vs > 32)
MODELS = (1, 0)


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


_checked = set()


def corpus(vs):
    """the corpus of a value size, its conditions asserted (and printed) the first time it is asked for"""
    corp = sl.corpus(vs)
    if vs not in _checked:
        for what, value in sl.conditions(corp).items():
            print("%s: %s" % (what, value))
        _checked.add(vs)
    return corp


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def host(*tensors):
    import torch
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in tensors)


def encode_at(dca, ctx, corp, ptr, ld, ad, cap, device, count=None):
    """the device-resident entry point of the value size's container on rows that start at `ptr`, `ld` samples apart"""
    import torch
    out = torch.zeros((corp.C, cap), dtype=torch.uint8, device=device)
    bits = torch.zeros(corp.C, dtype=torch.int64, device=device)
    err = torch.zeros(corp.C, dtype=torch.int32, device=device)
    L = dca.library()
    tail = (out.data_ptr(), cap, bits.data_ptr(), err.data_ptr(), ctx._stream())
    if count is not None:
        assert corp.vs > 32
        ret = L.dega_hip_encode64_var_dev(ctx._h, ptr, corp.C, corp.T, ld, count.data_ptr(), ad, corp.vs, *tail)
    else:
        ret = (L.dega_hip_encode64_dev if corp.vs > 32 else L.dega_hip_encode_dev)(ctx._h, ptr, corp.C, corp.T, ld, ad, corp.vs, *tail)
    assert ret == 0, ctx.last_error()
    return host(out, bits, err)


# ---- encode ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ad", MODELS)
@pytest.mark.parametrize("vs", sl.SIZES)
def test_encode_device_resident(dca, ctx, vs, ad):
    """Context.encode(valuesize=) up to 32, dega_hip_encode64_dev above"""
    corp = corpus(vs)
    xd = dev(corp.xin)
    if vs <= 32:
        got = host(*ctx.encode(xd, adaptive=ad, cap=corp.cap, valuesize=vs))
    else:
        got = encode_at(dca, ctx, corp, xd.data_ptr(), corp.C, ad, corp.cap, xd.device)
    sl.check_encode(corp, ad, *got, what="device resident")


@pytest.mark.parametrize("ad", MODELS)
@pytest.mark.parametrize("vs", (8, 32))
def test_encode_job_with_big_endian_samples(dca, ctx, vs, ad):
    corp = corpus(vs)
    packed, offsets, bits, err = ctx.encode_job(np.ascontiguousarray(corp.xin.astype(">i4")), adaptive=ad, valuesize=vs, samples=dca.SAMPLES_BE32)
    want_out, want_bits, want_err = corp.encoded(ad)
    assert (err == want_err).all(), np.flatnonzero(err != want_err)[:8].tolist()
    assert len(packed) == int(offsets[-1]) and int(offsets[0]) == 0
    for c in np.flatnonzero(want_err == 0):
        n = (int(want_bits[c]) + 7) // 8
        assert int(bits[c]) == int(want_bits[c]) and int(offsets[c + 1]) - int(offsets[c]) == n, (vs, ad, int(c))
        assert packed[int(offsets[c]): int(offsets[c]) + n].tobytes() == want_out[c, :n].tobytes(), (vs, ad, int(c), sl.KINDS[corp.kind[c]])


@pytest.mark.parametrize("ad", MODELS)
@pytest.mark.parametrize("vs,form", ((32, "ld = C + 7"), (17, "ld = C + 7"), (32, "base off by one element")))
def test_encode_through_the_per_row_fetch(dca, ctx, vs, form, ad):
    """a row pitch of C + 7 (and a base off by one element) turns the x4 row fetch off; what lies between the rows is not the
    batch's -- as a sample, all ones would be refused"""
    import torch
    corp = corpus(vs)
    if form == "ld = C + 7":
        wide = torch.full((corp.T, corp.C + 7), -1, dtype=torch.int32, device="cuda")
        wide[:, : corp.C] = dev(corp.xin)
        got = encode_at(dca, ctx, corp, wide.data_ptr(), corp.C + 7, ad, corp.cap, wide.device)
    else:
        flat = torch.full((corp.T * corp.C + 1,), -1, dtype=torch.int32, device="cuda")
        flat[1:] = dev(corp.xin).reshape(-1)
        got = encode_at(dca, ctx, corp, flat.data_ptr() + 4, corp.C, ad, corp.cap, flat.device)
    sl.check_encode(corp, ad, *got, what=form)


@pytest.mark.parametrize("ad", MODELS)
@pytest.mark.parametrize("vs", (32, 17))
def test_encode_segments(ctx, vs, ad):
    """launch boundaries at rows 1, 7, 8, 9 and inside the ladder: the bit queue and `last` cross launches.  (The method
    takes int32 rows; there is no segmented entry for the 64-bit containers to call.)"""
    corp = corpus(vs)
    cuts = sl.segment_cuts(corp.T)
    sl.check_encode(corp, ad, *host(*ctx.encode_segments(dev(corp.xin), cuts, adaptive=ad, cap=corp.cap, valuesize=vs)), what="cuts %s" % cuts)


@pytest.mark.parametrize("ad", MODELS)
@pytest.mark.parametrize("vs", (32, 17, 40))
def test_encode_counted(dca, ctx, vs, ad):
    """a ragged batch: Context.encode(count=), dega_hip_encode64_var_dev at 40; counts end ladders in front of, inside and behind
    the pair of rows of their longest codeword; expected is the oracle on each channel's own prefix"""
    corp = corpus(vs)
    xd, cd = dev(corp.xin), dev(corp.counts().astype(np.int64))
    if vs <= 32:
        got = host(*ctx.encode(xd, adaptive=ad, cap=corp.cap, valuesize=vs, count=cd)[:3])
    else:
        got = encode_at(dca, ctx, corp, xd.data_ptr(), corp.C, ad, corp.cap, xd.device, count=cd)
    sl.check_encode_counted(corp, ad, *got, what="counted")


@pytest.mark.parametrize("ad", MODELS)
@pytest.mark.parametrize("vs", (17, 32))
def test_encode_f32_with_factor_one(ctx, vs, ad):
    """The float entry on the channels whose samples are all below 2^23 and below 2^(vs-1) - 1 -- Normalize checks its range
    after adding one half (normalize.c:17-22) --: the float32 and the float32 plus one half are exact, the oracle's Normalize
    accepts every value and gives the integer sample (asserted), so the streams are the integer ones."""
    corp = corpus(vs)
    sel = np.flatnonzero(corp.x.max(axis=0) < min(1 << 23, (1 << (vs - 1)) - 1))
    assert len(sel) >= 160 and set(range(64)) <= set(sel.tolist()) and corp.x[:, sel].max() < (1 << 23)
    v = np.ascontiguousarray(corp.x[:, sel]).astype(np.float32)
    status, fields = orc.normalize_each(v.ravel(), 1.0, vs)
    assert not status.any() and (fields.reshape(v.shape) == corp.x[:, sel]).all()
    sl.check_encode(corp, ad, *host(*ctx.encode_f32(dev(v), factor=1.0, adaptive=ad, cap=corp.cap, valuesize=vs)), what="encode_f32", channels=sel)


@pytest.mark.parametrize("part", (2, 4))
@pytest.mark.parametrize("vs", (32, 63))
def test_short_slab_contract(dca, ctx, vs, part):
    """Half the worst case, and a quarter: the worst-case channels do not fit (asserted from the oracle: at the half under the
    static model, at the quarter under both) and report ERROR_MEMORY, the oracle's bit length and the oracle's bytes in front
    of the cap; the others are whole"""
    corp = corpus(vs)
    cap, overflowing = sl.short_cap(corp, part)
    assert overflowing == ([0] if part == 2 else [1, 0])
    xd = dev(corp.xin)
    for ad in MODELS:
        if vs <= 32:
            got = host(*ctx.encode(xd, adaptive=ad, cap=cap, valuesize=vs))
        else:
            got = encode_at(dca, ctx, corp, xd.data_ptr(), corp.C, ad, cap, xd.device)
        sl.check_encode_short(corp, ad, cap, *got, what="short slab")


# ---- decode ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ad", MODELS)
@pytest.mark.parametrize("vs", NARROW)
def test_decode_device_resident_with_fixed_length(ctx, vs, ad):
    corp = corpus(vs)
    slabs, bits, _ = corp.decoder_input(ad)
    y, err = host(*ctx.decode(dev(slabs), dev(bits.astype(np.int64)), corp.T, adaptive=ad, valuesize=vs))
    sl.check_decode(corp, ad, y, None, err, what="Context.decode")


@pytest.mark.parametrize("ad", MODELS)
@pytest.mark.parametrize("vs", sl.SIZES)
def test_decode_var_host(ctx, vs, ad):
    """decode_var_host up to 32, decode64_var_host above, with room for T + 3 samples"""
    corp = corpus(vs)
    slabs, bits, _ = corp.decoder_input(ad)
    if vs <= 32:
        got = ctx.decode_var_host(slabs, bits, corp.T + 3, adaptive=ad, valuesize=vs)
    else:
        got = ctx.decode64_var_host(slabs, bits, corp.T + 3, vs, adaptive=ad)
    sl.check_decode(corp, ad, *got, what="decode_var_host")


@pytest.mark.parametrize("ad", MODELS)
@pytest.mark.parametrize("vs", (32, 12))
def test_decode_job_with_counts(ctx, vs, ad):
    corp = corpus(vs)
    slabs, bits, _ = corp.decoder_input(ad)
    nbytes = ((bits + np.uint64(7)) // np.uint64(8)).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(nbytes)]).astype(np.uint64)
    packed = np.concatenate([slabs[c, : nbytes[c]] for c in range(corp.C)])
    sl.check_decode(corp, ad, *ctx.decode_job(packed, offsets, bits, corp.T + 3, adaptive=ad, valuesize=vs, var=True), what="decode_job(var=True)")


def test_eight_pair_decoders(dca, monkeypatch):
    """DEGA_WAVES_PER_WORKGROUP=8 on a fresh context, as tests/test_valuesize.py does: the workgroups of eight pairs of waves
    that decode batches of more than 64 Ki channels, at value sizes 32, 15 and 64"""
    monkeypatch.setenv("DEGA_WAVES_PER_WORKGROUP", "8")
    ctx = dca.Context(0)
    for vs in (32, 15, 64):
        corp = corpus(vs)
        for ad in MODELS:
            slabs, bits, _ = corp.decoder_input(ad)
            if vs <= 32:
                y, err = ctx.decode_host(slabs, bits, corp.T, adaptive=ad, valuesize=vs)
                sl.check_decode(corp, ad, y, None, err, what="decode_host, eight pairs")
            else:
                sl.check_decode(corp, ad, *ctx.decode64_var_host(slabs, bits, corp.T + 3, vs, adaptive=ad), what="decode64_var_host, eight pairs")
    ctx.close()
