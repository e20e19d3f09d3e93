"""GPU tests (-m gpu) of the host pipeline with everything at once that a call at production size has: a batch cut into
several chunks, every chunk's rows crossing the link in bands (encode: one launch per band, the lanes' state kept in the
slot's seg_state; decode: every wave reports rows_done to a pinned word and the host downloads the band on a second
stream), more chunks than slots, and the eight-pair decode workgroups -- at the smallest shapes that have them
(bands_chunks_common.py): DEGA_PIPELINE_CHUNKS and DEGA_PIPELINE_BAND_BYTES together on more than 8 192 channels.

What is compared against: the same call with neither knob set -- one chunk, no bands, which the other files hold to the
oracle -- byte for byte, and the oracle itself (orc.encode_i32 / orc.encode_f32 / the stage chain of hostile_common.py) on
the first and last channel of every chunk and on every steered channel: the references are held to it once, and every
result under the knobs is the reference's, whole.  There is no tolerance anywhere."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from __graft_entry__ import load_package
from oracle import orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bands_chunks_common as bc  # noqa: E402
import hostile_common as hc  # noqa: E402

pytestmark = pytest.mark.gpu

CA, TA, CB, TB = bc.CA, bc.TA, bc.CB, bc.TB
ALL_KNOBS = ("DEGA_PIPELINE_CHUNKS", "DEGA_PIPELINE_BAND_BYTES", "DEGA_PIPELINE_AHEAD", "DEGA_PIPELINE_AHEAD_DECODE", "DEGA_PIPELINE_UPLOADS_FIRST",
             "DEGA_PIPELINE_IN_PLACE", "DEGA_WAVES_PER_WORKGROUP")
NAMES = ("packed", "offsets", "bits", "err")


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


def set_knobs(monkeypatch, chunks, **more):
    for k, v in dict(bc.knobs(chunks), **more).items():
        monkeypatch.setenv(k, v)


# ---- the oracle on single channels ---------------------------------------------------------------------------------------------

def oracle_stream(col, kw):
    """one channel through the oracle's encoder: (status, stream bytes, bits)"""
    vs, ad = kw["valuesize"], kw["adaptive"]
    if kw["samples"] == 3:  # float32
        if vs == 32:
            return orc.encode_f32(np.ascontiguousarray(col), kw["factor"], ad)
        data, n, names = np.ascontiguousarray(col).tobytes(), 32 * col.size, ("normalize", "diff", "seg", "bac")
    else:
        if vs == 32:
            return orc.encode_i32(np.ascontiguousarray(col.astype(np.int32)), ad)
        (data, n), names = hc.pack_be(col.astype(np.int64).view(np.uint64), vs), ("diff", "seg", "bac")
    for name in names:
        r, data, n = orc.stage(name, True, data, n, valuesize=vs, adaptive=ad, factor=kw.get("factor", 100.0))
        if r != 0:
            return r, b"", 0
    return 0, data[: (n + 7) // 8], n


def oracle_floats(stream, nbits, kw):
    """what the oracle's decoder makes of a float stream: the bytes of its float32 samples"""
    data, n = stream, nbits
    for name in ("bac", "seg", "diff", "normalize"):
        r, data, n = orc.stage(name, False, data, n, valuesize=kw["valuesize"], adaptive=kw["adaptive"], factor=kw["factor"])
        assert r == 0, name
    return data[: n // 8]


def hold_to_the_oracle(x, kw, enc, dec, channels, tag):
    """the reference call's streams, statuses and decoded samples on `channels` are the oracle's"""
    packed, offsets, bits, err = enc
    back, derr = dec
    for c in channels:
        r, b, n = oracle_stream(x[:, c], kw)
        assert int(err[c]) == r, (tag, c, int(err[c]), r)
        if r != 0:
            continue
        assert int(bits[c]) == n and packed[int(offsets[c]): int(offsets[c + 1])].tobytes() == b, (tag, c)
        assert int(derr[c]) == 0, (tag, c)
        if kw["samples"] == 3:
            assert np.ascontiguousarray(back[:, c]).tobytes() == oracle_floats(b, n, kw), (tag, c)
        else:
            assert (back[:, c] == x[:, c]).all(), (tag, c)


def same_job(got, want, tag):
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (tag, name)


def same_samples(got, want, tag):
    (y, derr), (wy, wderr) = got, want
    assert (derr == wderr).all(), (tag, "err", np.nonzero(derr != wderr)[0][:8].tolist())
    assert y.dtype == wy.dtype and y.shape == wy.shape, tag
    if y.tobytes() != wy.tobytes():
        bits_of = {4: np.uint32, 8: np.uint64}[y.dtype.itemsize]  # (floats are compared as the bits they are)
        rows, cols = np.nonzero(np.ascontiguousarray(y).view(bits_of) != np.ascontiguousarray(wy).view(bits_of))
        raise AssertionError((tag, "samples differ in %d places, first at row %d, channel %d (chunk %d, band %d), status %d"
                              % (len(rows), int(rows[0]), int(cols[0]), int(cols[0]) // bc.CHUNK, int(rows[0]) // bc.BAND_ROWS, int(wderr[cols[0]]))))


# ---- shape A: the references ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def refs(dca, ctx):
    """for every sample type: shape A's steered batch, its one-chunk encode and its one-chunk fixed-count decode -- computed
    once with no knob set, held to the oracle on the chunks' first and last channels and on every steered channel, never
    changed"""
    assert not [k for k in ALL_KNOBS if k in os.environ]
    out = {}
    watch = sorted(set(bc.chunk_edges(CA)) | set(bc.NOISY) | set(bc.BROKEN) | set(bc.CONSTANT))
    for kind in bc.KINDS:
        x, kw = bc.input_a(kind, dca)
        enc = ctx.encode_job(x, **kw)
        dec = ctx.decode_job(enc[0], enc[1], enc[2], TA, **kw)
        hold_to_the_oracle(x, kw, enc, dec, watch, kind)
        err = enc[3]
        assert (err[list(bc.BROKEN)] == dca.ERROR_INVALID_VALUE).all() and int((err != 0).sum()) == len(bc.BROKEN), kind
        for a in (x,) + tuple(enc) + tuple(dec):
            a.flags.writeable = False
        out[kind] = (x, kw, enc, dec)
    return out


def test_shape_a_is_what_it_claims(dca, refs):
    """the noisy channels' streams outgrow the usual slab of 4 T + 64 bytes, so the middle and the last chunk -- coded in bands
    -- are redone with worst-case slabs from the rows the bands brought; the streams lie back to back from 0"""
    for kind in ("i32", "i32 static", "be32", "f32"):
        _, _, (packed, offsets, bits, err), _ = refs[kind]
        for c in bc.NOISY:
            assert int(err[c]) == 0 and int(offsets[c + 1] - offsets[c]) > 4 * TA + 64, (kind, c)
        assert int(offsets[0]) == 0 and int(offsets[CA]) == packed.size
    assert bc.BROKEN_FROM // bc.BAND_ROWS == 4 and bc.bands_of(TA) == 7 and TA % bc.BAND_ROWS == 8
    assert [c // bc.CHUNK for c in bc.NOISY] == [1, 2] and [c // bc.CHUNK for c in bc.BROKEN] == [0, 1, 2] == [c // bc.CHUNK for c in bc.CONSTANT]


# ---- proof that chunks and bands are really there ---------------------------------------------------------------------------------

def traced_child(shape, env_knobs):
    """stderr of a fresh process that runs the shape's encode and decode once under DEGA_PIPELINE_TRACE=1 (the flag is read
    once per process), split at the marker into (fixed-count part, variable-count part)"""
    env = {k: v for k, v in os.environ.items() if k not in ALL_KNOBS}
    env.update(env_knobs)
    env["DEGA_PIPELINE_TRACE"] = "1"
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "bands_chunks_common.py"), shape], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    fixed, _, var = p.stderr.partition("== variable count ==")
    return fixed, var


def check_trace(shape, env_knobs):
    Cn, T, nchunks = (CA, TA, bc.CHUNKS_A) if shape == "A" else (CB, TB, bc.CHUNKS_B)
    nslots, nbands = min(nchunks, bc.SLOTS), bc.bands_of(T)
    fixed, var = traced_child(shape, env_knobs)
    plan = "C %d T %d, %d chunks of %d channels, %d slots" % (Cn, T, nchunks, bc.CHUNK, nslots)
    enc_plans = re.findall(r"encode share: (.*)", fixed)
    assert enc_plans == [plan], ("the encode call's plan", enc_plans, "expected", plan)
    enc_bands = re.findall(r"\] chunk (\d+): (\d+ bands of \d+ rows), one launch each", fixed)
    assert enc_bands == [(str(k), "%d bands of %d rows" % (nbands, bc.BAND_ROWS)) for k in range(nchunks)], ("the encode call's bands", enc_bands)
    dec_plans = re.findall(r"decode share: (.*)", fixed)
    want = plan + (", chunk by chunk" if nchunks > nslots else ", all uploads first")  # (more chunks than slots: decode's run_chunks branch)
    assert dec_plans == [want], ("the decode call's plan", dec_plans, "expected", want)
    dec_bands = re.findall(r"decode chunk (\d+): (\d+ bands of \d+ rows)", fixed)
    assert sorted(dec_bands, key=lambda e: int(e[0])) == [(str(k), "%d bands of %d rows" % (nbands, bc.BAND_ROWS)) for k in range(nchunks)], \
        ("the decode call's bands", dec_bands)
    # a variable-count decode has the same chunks and NO bands (decode_share: band_rows = 0 when counts are asked for): which
    # is why every decode below is a fixed-count one
    assert re.findall(r"decode share: (.*)", var) == [want] and "bands of" not in var, var[-1000:]


@pytest.mark.parametrize("shape", ("A", "B"))
def test_the_calls_have_the_chunks_and_the_bands_they_claim(shape):
    """From the pipeline's own trace in a fresh process: the encode and the decode call of the shape are cut into 3 (17) chunks of
    8 192 channels on 3 (16) slots, every chunk goes in 7 (3) bands of 32 rows, and shape B's decode -- more chunks than slots
    -- takes the run_chunks branch.  Without this, a knob that stopped taking effect would turn every test of this file into
    a comparison of the one-chunk call with itself."""
    check_trace(shape, bc.knobs(bc.CHUNKS_A if shape == "A" else bc.CHUNKS_B))


# ---- shape A: encode ---------------------------------------------------------------------------------------------------------------

def test_encode_from_pageable_and_pinned_memory_on_contexts_and_groups(dca, ctx, refs, monkeypatch):
    """Three chunks of seven launches each, however far the first stages run ahead (DEGA_PIPELINE_AHEAD 1, 2, 16), from
    pageable and pinned memory, on a context, a group of one and a group of two (two chunks per member).  Catches: the
    running base of the packed streams across chunks (a redone chunk in the middle included), a band uploaded from or to
    the wrong row (t0 * ld on the host side, t0 * n on the device side), seg_state handed from one launch to the next --
    the refused channels' error from band 4 to the end -- and reuse_ev / band_ev when a slot's second stream is used again."""
    x, kw, want, _ = refs["i32"]
    groups = {"one": dca.Group([0]), "two": dca.Group([0, 0])}
    pin = dca.PinnedArray((TA, CA), np.int32)
    try:
        pin.array[:] = x
        for ahead in ("1", "2", "16"):
            set_knobs(monkeypatch, bc.CHUNKS_A, DEGA_PIPELINE_AHEAD=ahead)
            for who, src, tag in ((ctx, x, "context"), (ctx, pin.array, "context, pinned"), (groups["one"], x, "group of one"), (groups["two"], x, "group of two")):
                same_job(who.encode_job(src, **kw), want, (tag, ahead))
    finally:
        pin.free()
        for g in groups.values():
            g.close()


@pytest.mark.parametrize("kind", [k for k in bc.KINDS if k != "i32"])
def test_encode_sample_types(dca, ctx, refs, monkeypatch, kind):
    """The static model, big-endian samples, int64 samples at value size 40 (walks near 2^37) and the float entry at value
    sizes 32 and 48 through chunks and bands.  Catches: the band row offsets at 8 bytes a sample (t0 * n * esz), seg_state's
    64-bit `last` (a non-zero high half) between the launches of a chunk and -- the slot's state is not cleared -- after
    another chunk's, the byte swap and the normalize of a band that is not the first."""
    x, kw, want, _ = refs[kind]
    set_knobs(monkeypatch, bc.CHUNKS_A)
    same_job(ctx.encode_job(x, **kw), want, kind)


@pytest.mark.parametrize("kind", ("i32", "i64"))
def test_encode_from_a_wider_array(dca, ctx, refs, monkeypatch, kind):
    """channels= with a source pitch of C + 5 whose padding holds -1, at 4 and at 8 bytes a sample.  Catches: a band's source
    address (t0 * ld, not t0 * C) and a chunk's first column, a padding column read as a channel (-1 is refused)."""
    x, kw, want, _ = refs[kind]
    wide = np.full((TA, CA + 5), -1, dtype=x.dtype)
    wide[:, :CA] = x
    set_knobs(monkeypatch, bc.CHUNKS_A)
    same_job(ctx.encode_job(wide, channels=CA, **kw), want, kind)


def test_encode_packed_buffer_one_byte_short(dca, ctx, refs, monkeypatch):
    """through the C ABI with packed_cap one byte short of the total: ERROR_MEMORY, offsets[C] the size needed, bits and err
    complete -- as test_plain_packed_buffer_too_small asserts without bands.  Catches: the running base when the last
    chunk (redone, coded in bands) no longer fits."""
    x, kw, (packed, offsets, bits, err), _ = refs["i32"]
    job = dca.Job(CA, TA, CA, 1, 32, dca.SAMPLES_I32, 0.0)
    set_knobs(monkeypatch, bc.CHUNKS_A)
    cap = packed.size - 1
    buf = np.zeros(cap, dtype=np.uint8)
    o, b, e = np.full(CA + 1, 7, dtype=np.uint64), np.full(CA, 7, dtype=np.uint64), np.full(CA, 7, dtype=np.int32)
    ret = dca.library().dega_hip_encode_job_host(ctx._h, C.byref(job), x.ctypes.data, buf.ctypes.data, cap, o.ctypes.data, b.ctypes.data, e.ctypes.data)
    assert ret == dca.ERROR_MEMORY and int(o[CA]) == packed.size
    assert (o == offsets).all() and (b == bits).all() and (e == err).all()
    assert buf[: int(offsets[2 * bc.CHUNK])].tobytes() == packed[: int(offsets[2 * bc.CHUNK])].tobytes()  # (the chunks that did fit are delivered)


# ---- shape A: decode (fixed count: a variable-count decode has no bands, see check_trace) -----------------------------------------

@pytest.mark.parametrize("ahead", ("1", "16"))
@pytest.mark.parametrize("uploads_first", ("0", "1"))
def test_decode_into_pageable_and_pinned_memory(dca, ctx, refs, monkeypatch, uploads_first, ahead):
    """Three chunks whose rows come home in seven bands each, beside the running kernels: into a pageable and a pinned array,
    from pageable and pinned streams, uploads first or chunk by chunk (DEGA_PIPELINE_UPLOADS_FIRST=0 is decode's
    run_chunks branch), one or all chunks ahead.  Catches: a band copied from the wrong row of the device image or to the
    wrong row or column of the caller's (t0 * n, t0 * ld + c0), progress words of the wrong chunk, a band sent before its
    rows were stored."""
    x, kw, (packed, offsets, bits, err), want = refs["i32"]
    set_knobs(monkeypatch, bc.CHUNKS_A, DEGA_PIPELINE_UPLOADS_FIRST=uploads_first, DEGA_PIPELINE_AHEAD_DECODE=ahead)
    same_samples(ctx.decode_job(packed, offsets, bits, TA, **kw), want, "pageable")
    pin, pk = dca.PinnedArray((TA, CA), np.int32), dca.PinnedArray((packed.size,), np.uint8)
    try:
        pin.array[:] = -7
        pk.array[:] = packed
        y, derr = ctx.decode_job(packed, offsets, bits, TA, out=pin.array, **kw)
        same_samples((np.array(y), derr), want, "pinned out")
        pin.array[:] = -7
        y, derr = ctx.decode_job(pk.array, offsets, bits, TA, out=pin.array, **kw)
        same_samples((np.array(y), derr), want, "pinned out, pinned packed")
        same_samples(ctx.decode_job(pk.array, offsets, bits, TA, **kw), want, "pinned packed")
    finally:
        pin.free()
        pk.free()


@pytest.mark.parametrize("kind", [k for k in bc.KINDS if k != "i32"])
def test_decode_sample_types(dca, ctx, refs, monkeypatch, kind):
    """The static model, big-endian samples, int64 samples and the float exit at value sizes 32 and 48 through chunks and
    bands -- none of which a banded decode had run with.  Catches: the 8-byte band arithmetic (t0 * n * osz and
    (t0 * ld + c0) * osz with osz = 8), the float exit and the byte swap of rows that go home while the kernel runs."""
    x, kw, (packed, offsets, bits, err), want = refs[kind]
    set_knobs(monkeypatch, bc.CHUNKS_A)
    same_samples(ctx.decode_job(packed, offsets, bits, TA, **kw), want, kind)


@pytest.mark.parametrize("kind", ("i32", "i64"))
def test_decode_into_a_wider_array(dca, ctx, refs, monkeypatch, kind):
    """layout="time" into an array of pitch C + 5 filled with a poison value: the samples are the reference's and every
    padding element keeps the poison, at 4 and at 8 bytes a sample.  Catches: a band's destination (t0 * ld + c0) computed
    with the chunk's or the batch's width instead of the caller's pitch, rows copied at the wrong width."""
    x, kw, (packed, offsets, bits, err), want = refs[kind]
    poison = -0x5A5A5A5B
    out = np.full((TA, CA + 5), poison, dtype=x.dtype)
    set_knobs(monkeypatch, bc.CHUNKS_A)
    y, derr = ctx.decode_job(packed, offsets[: CA + 1], bits, TA, out=out, **kw)
    assert y is out and (out[:, CA:] == poison).all(), kind
    same_samples((np.ascontiguousarray(out[:, :CA]), derr), want, kind)


def test_decode_with_the_eight_pair_workgroups(dca, refs, monkeypatch):
    """A fresh context under DEGA_WAVES_PER_WORKGROUP=8 (as test_gpu_eight_pair_decoders_on_a_small_batch has it): the
    workgroups of eight pairs of waves report rows_done too.  int32 and the float exit.  Catches: a wave of the wide
    workgroup reporting into another wave's progress word, or none."""
    set_knobs(monkeypatch, bc.CHUNKS_A, DEGA_WAVES_PER_WORKGROUP="8")
    wide = dca.Context(0)
    try:
        for kind in ("i32", "f32"):
            x, kw, (packed, offsets, bits, err), want = refs[kind]
            same_samples(wide.decode_job(packed, offsets, bits, TA, **kw), want, kind)
    finally:
        wide.close()


def test_damaged_streams_through_the_banded_decode(dca, ctx, refs, monkeypatch):
    """One channel in nine of shape A with 1 ... 3 flipped bits -- the first and last channel of every chunk, whole waves of 64
    and lone channels -- decoded with and without the two knobs into poisoned arrays: the statuses and the whole [T][C]
    array are the same, the zero rows behind a failed channel's last sample included, and the damaged channels that still
    decode give the oracle's samples.  Catches: a wave whose channels fail in the middle of a band and stops reporting or
    reports too early (rows sent home before they were zeroed), a failed lane's rows of a later band left as the slot's
    previous chunk wrote them."""
    x, kw, (packed, offsets, bits, err), _ = refs["i32"]
    sel = bc.damaged_channels()
    assert CA // 10 < len(sel) < CA // 7 and (err[sel] == 0).all()
    bad = bc.damage(packed, offsets, bits, sel)
    poison = -0x5A5A5A5B
    plain = ctx.decode_job(bad, offsets, bits, TA, out=np.full((TA, CA), poison, dtype=np.int32), **kw)
    set_knobs(monkeypatch, bc.CHUNKS_A)
    banded = ctx.decode_job(bad, offsets, bits, TA, out=np.full((TA, CA), poison, dtype=np.int32), **kw)
    y, derr = banded
    # the oracle on the damaged channels (its batch call: slabs)
    lens = (offsets[sel + 1] - offsets[sel]).astype(np.int64)
    slabs = np.zeros((len(sel), int(lens.max()) + 8), dtype=np.uint8)
    for i, c in enumerate(sel):
        slabs[i, : lens[i]] = bad[int(offsets[c]): int(offsets[c]) + int(lens[i])]
    oy, oerr = orc.decode_batch_tc(slabs, bits[sel], TA, 1)
    failed, decoded = int((derr[sel] != 0).sum()), int((derr[sel] == 0).sum())
    print("damaged %d channels: %d fail (%s), %d still decode; oracle: %d fail" % (len(sel), failed, {int(k): int((derr[sel] == k).sum()) for k in np.unique(derr[sel])},
                                                                                decoded, int((oerr != 0).sum())))
    assert failed >= 20 and decoded >= 5
    assert ((derr[sel] == 0) == (oerr == 0)).all(), sel[(derr[sel] == 0) != (oerr == 0)][:8].tolist()
    ok = oerr == 0
    assert (y[:, sel[ok]] == oy[:, ok]).all()
    rest = np.ones(CA, dtype=bool)
    rest[sel] = False
    rest[list(bc.BROKEN)] = False
    assert (derr[rest] == 0).all() and (y[:, rest] == x[:, rest]).all()
    same_samples(banded, plain, "banded against plain")


# ---- shape B: more chunks than slots, more than 65 536 channels ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def refs_b(dca, ctx):
    """shape B's int32 and float batches with their one-chunk encode and decode, held to the oracle on the first and last
    channel of chunks 0, 1, 15 and 16"""
    assert not [k for k in ALL_KNOBS if k in os.environ]
    out = {}
    edges = bc.chunk_edges(CB)
    watch = edges[:4] + edges[-4:]
    assert watch == [0, 8191, 8192, 16383, 15 * 8192, 16 * 8192 - 1, 16 * 8192, CB - 1]
    for kind in ("i32", "f32"):
        x, kw = bc.input_b(kind, dca)
        enc = ctx.encode_job(x, **kw)
        dec = ctx.decode_job(enc[0], enc[1], enc[2], TB, **kw)
        assert (enc[3] == 0).all() and (dec[1] == 0).all()
        hold_to_the_oracle(x, kw, enc, dec, watch, ("B", kind))
        for a in (x,) + tuple(enc) + tuple(dec):
            a.flags.writeable = False
        out[kind] = (x, kw, enc, dec)
    return out


def test_seventeen_chunks_on_sixteen_slots_encode(dca, ctx, refs_b, monkeypatch):
    """17 chunks of 3 launches each on 16 slots: chunk 16 takes over slot 0 -- its buffers, its second stream, reuse_ev, band_ev
    and seg_state -- within the call.  Catches: seg_state of chunk 0 leaking into chunk 16 (the first launch of a chunk must
    not continue), uploads of chunk 16 overtaking chunk 0's gather and download, the running base over 17 chunks."""
    x, kw, want, _ = refs_b["i32"]
    set_knobs(monkeypatch, bc.CHUNKS_B)
    same_job(ctx.encode_job(x, **kw), want, "B")


@pytest.mark.parametrize("kind", ("i32", "f32"))
def test_seventeen_chunks_on_sixteen_slots_decode(dca, ctx, refs_b, monkeypatch, kind):
    """The decode of the same: more chunks than slots is decode's run_chunks branch (otherwise taken only when device memory
    is short), the batch is above 65 536 channels, so every chunk's kernel has the eight-pair workgroups, and slot 0's
    progress words are zeroed again for chunk 16.  int32 and the float exit.  Catches: stale progress words on slot re-use
    (bands of chunk 16 sent home before they were stored: chunk 0's samples in chunk 16's columns), the second stream's
    downloads of chunk 0 still running when chunk 16's kernel writes the slot's image."""
    x, kw, (packed, offsets, bits, err), want = refs_b[kind]
    set_knobs(monkeypatch, bc.CHUNKS_B)
    same_samples(ctx.decode_job(packed, offsets, bits, TB, **kw), want, ("B", kind))
