"""The DEGA encoder on steered inputs, on the GPU (tests/encoder_regimes_common.py has the corpus, its conditions and the
checkers): every entry point that ends in the encode kernel, held to the oracle (orc.encode_batch_tc on the same series) on
status, bit length and every byte -- on series that keep the coder off its usual word path: bit at a time, the four-symbol
and the general word path, exchanges of the two symbols, halvings at a different row in every lane, and carries that run
back through hundreds of one-bits already written.  T = 600, C = 650: ten waves and a ragged one."""
import numpy as np
import pytest

import encoder_regimes_common as rc
import hostile_common as hc
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

CN, T = 650, 600


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
def corp():
    corp = rc.corpus(CN, T)
    for what, value in rc.conditions(corp).items():  # (asserted here too: this batch is larger than the emulator's)
        print("%s: %s" % (what, value))
    return corp


@pytest.fixture(scope="module")
def xd(corp):
    import torch
    return torch.from_numpy(corp.x.copy()).cuda()


def host(*tensors):
    import torch
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in tensors)


def encode_at(dca, ctx, ptr, ld, ad, cap, device):
    """the device-resident entry point on rows that start at `ptr`, `ld` samples apart"""
    import torch
    out = torch.zeros((CN, cap), dtype=torch.uint8, device=device)
    bits = torch.zeros(CN, dtype=torch.int64, device=device)
    err = torch.zeros(CN, dtype=torch.int32, device=device)
    ret = dca.library().dega_hip_encode_dev(ctx._h, ptr, CN, T, ld, ad, 32, out.data_ptr(), cap, bits.data_ptr(), err.data_ptr(), ctx._stream())
    assert ret == 0, ctx.last_error()
    return host(out, bits, err)


@pytest.mark.parametrize("ad", (1, 0))
@pytest.mark.parametrize("form", ("natural pitch", "ld = C + 7", "base off by one element"))
def test_encode_device_resident(dca, ctx, corp, xd, ad, form):
    import torch
    if form == "natural pitch":
        got = host(*ctx.encode(xd, adaptive=ad, cap=corp.cap))
    elif form == "ld = C + 7":
        wide = torch.full((T, CN + 7), -1, dtype=torch.int32, device=xd.device)  # (what lies between the rows is not the batch's: as a sample, -1 would be refused)
        wide[:, :CN] = xd
        got = encode_at(dca, ctx, wide.data_ptr(), CN + 7, ad, corp.cap, xd.device)
    else:
        flat = torch.full((T * CN + 1,), -1, dtype=torch.int32, device=xd.device)
        flat[1:] = xd.reshape(-1)
        got = encode_at(dca, ctx, flat.data_ptr() + 4, CN, ad, corp.cap, xd.device)
    rc.check_full(corp, ad, *got, what=form)


@pytest.mark.parametrize("ad", (1, 0))
def test_encode_host_and_packed_host(ctx, corp, ad):
    rc.check_full(corp, ad, *ctx.encode_host(corp.x, adaptive=ad, cap=corp.cap), what="encode_host")
    check_packed(corp, ad, *ctx.encode_packed_host(corp.x, adaptive=ad), what="encode_packed_host")


def check_packed(corp, ad, packed, offsets, bits, err, what, channels=None):
    """the packed form against the oracle (channels: the results are those of these channels)"""
    want_out, want_bits, want_err = corp.oracle(ad)
    if channels is not None:
        want_out, want_bits, want_err = want_out[channels], want_bits[channels], want_err[channels]
    assert (err == want_err).all() and (bits == want_bits).all(), (what, ad)
    nbytes = (want_bits + np.uint64(7)) // np.uint64(8)
    assert int(offsets[0]) == 0 and (np.diff(offsets) == nbytes).all() and len(packed) == int(offsets[-1]), (what, ad)
    for c in range(len(want_bits)):
        assert packed[int(offsets[c]): int(offsets[c + 1])].tobytes() == want_out[c, : int(nbytes[c])].tobytes(), (what, ad, c)


@pytest.mark.parametrize("ad", (1, 0))
def test_encode_f32_with_factor_one(ctx, corp, xd, ad):
    """The float entry, Normalize fused into the fill phase: factor 1.0 on samples below 2^23 (asserted), so that the float32
    and the float32 plus one half (normalize.c:17-18) are exact and the streams are those of the integer series.  Kind 6 is
    left out of the float form: its samples go up to 2^31, far beyond what a float32 holds exactly."""
    import torch
    sel = np.flatnonzero(corp.kind != 6)
    assert corp.x[:, sel].min() >= 0 and corp.x[:, sel].max() < (1 << 23)
    v = torch.from_numpy(np.ascontiguousarray(corp.x[:, sel]).astype(np.float32)).cuda()
    assert (v.cpu().numpy().astype(np.int64) == corp.x[:, sel]).all()
    rc.check_full(corp, ad, *host(*ctx.encode_f32(v, factor=1.0, adaptive=ad, cap=corp.cap)), what="encode_f32", channels=sel)


@pytest.mark.parametrize("ad", (1, 0))
def test_encode_segments_cut_inside_the_runs(ctx, corp, xd, ad):
    """launch boundaries from the replay: the row where a run of >= 100 owed bits is settled, the row before it, a single row
    inside the run"""
    cuts = corp.cuts()
    rc.check_full(corp, ad, *host(*ctx.encode_segments(xd, cuts, adaptive=ad, cap=corp.cap)), what="cuts %s" % cuts)


def test_encode_segments_of_single_rows_across_a_long_run(ctx, corp, xd):
    cuts = corp.single_rows()
    assert len(cuts) > 12
    rc.check_full(corp, 1, *host(*ctx.encode_segments(xd, cuts, adaptive=1, cap=corp.cap)), what="cuts %s" % cuts)


def test_encode_job_in_bands_that_end_inside_a_run(ctx, corp, monkeypatch):
    """The host pipeline, rows uploaded in bands of 32 with a launch each and the lanes' state saved in between (the knob of
    tests/test_gpu_pipeline.py): band ends fall inside runs of >= 100 owed bits (asserted from the replay).  Without kind 6:
    the pipeline codes first into slabs of 4 T + 64 bytes and, if ONE stream of a chunk does not fit, codes the whole
    chunk again in single launches (encode_redo_chunk), whose result replaces the banded one -- so every stream here must
    fit (asserted from the oracle's lengths), and what is compared is what the banded launches wrote."""
    sel = np.flatnonzero(corp.kind != 6)
    x = np.ascontiguousarray(corp.x[:, sel])
    _, want_bits, _ = corp.oracle(1)
    assert int(want_bits[sel].max() + 7) // 8 <= 4 * T + 64
    steered = [c for c in corp.runs_across(32) if corp.kind[c] != 6]
    assert max(65536 // (4 * len(sel)), 32) == 32 < T and len(steered) >= 3
    monkeypatch.setenv("DEGA_PIPELINE_BAND_BYTES", "65536")
    check_packed(corp, 1, *ctx.encode_job(x, adaptive=1), what="encode_job, bands", channels=sel)
    monkeypatch.setenv("DEGA_PIPELINE_BAND_BYTES", "0")
    check_packed(corp, 1, *ctx.encode_job(x, adaptive=1), what="encode_job, no bands", channels=sel)


def test_encode_job_with_streams_longer_than_their_samples(ctx, corp, monkeypatch):
    """The whole corpus through the host pipeline: the jumps' streams (asserted: all of kind 6 and no other) outgrow the
    first attempt's slabs of 4 T + 64 bytes, so the chunk reports ERROR_MEMORY from the banded launches and is coded once
    more into worst-case slabs, in single launches -- the redo path, not the bands, is what this case holds to the oracle."""
    _, want_bits, _ = corp.oracle(1)
    assert (((want_bits + np.uint64(7)) // np.uint64(8) > 4 * T + 64) == (corp.kind == 6)).all()
    monkeypatch.setenv("DEGA_PIPELINE_BAND_BYTES", "65536")
    check_packed(corp, 1, *ctx.encode_job(corp.x, adaptive=1), what="encode_job, redone")


@pytest.mark.parametrize("ad", (1, 0))
def test_encode64_host_at_valuesize_40(ctx, corp, ad):
    """the 64-bit containers' kernel (the same writer behind another filling wave) against the oracle's stage chain, as
    tests/test_valuesize.py does"""
    x = corp.x.view(np.uint32).astype(np.uint64)
    want = hc.oracle_encode(x, 40, ad)
    out, bits, err = ctx.encode64_host(x.view(np.int64), 40, adaptive=ad)
    assert (err == 0).all()
    for c in range(CN):
        data, n = want[c]
        assert int(bits[c]) == n and out[c, : len(data)].tobytes() == data, (ad, c, rc.KINDS[c % 8])
        assert not out[c, len(data):].any()


@pytest.mark.parametrize("cap", rc.CAPS)
def test_short_slab_contract(ctx, corp, xd, cap):
    """ERROR_MEMORY, the oracle's length, and the stream's own bytes in front of the cap, while carries arrive beyond the cap
    after runs of owed bits that reach back over whole words (tests/test_encoder_regimes_host.py has the story)"""
    rc.check_short_is_not_vacuous(corp, cap)
    for ad in (1, 0):
        rc.check_short(corp, ad, cap, *host(*ctx.encode(xd, adaptive=ad, cap=cap)), what="encode")
    rc.check_short(corp, 1, cap, *ctx.encode_host(corp.x, adaptive=1, cap=cap), what="encode_host")


@pytest.mark.parametrize("ad", (1, 0))
def test_round_trip(ctx, corp, xd, ad):
    """the decoder gives the series back from the encoder's streams -- streams with 195 one-bits in a row in them"""
    out, bits, err = ctx.encode(xd, adaptive=ad, cap=corp.cap)
    y, derr = ctx.decode(out, bits, T, adaptive=ad)
    o, b, y, derr = host(out, bits, y, derr)
    assert (derr == 0).all() and (y == corp.x).all()
    if ad:
        assert max(rc.longest_run(o[c].tobytes(), int(b[c]), 1) for c in corp.of_kind(4, 5, 7)) >= 195
