"""The HIP LZMH decoder on damaged and hand-assembled streams (-m gpu): the streams and the checker of
tests/lzmh_hostile_common.py -- status 0, the oracle's length and the oracle's bytes for every channel, with and without
garbage behind the streams -- through the host entry, the device entry with a slab base off by a word and a stream that
ends with its slab, rows that are one byte too short, the group's host pipeline, and the chain into the csv reader."""
import os
import time

import numpy as np
import pytest

import csv_read_common as crc
import lzmh_hostile_common as lc
from __graft_entry__ import load_package
from oracle import orc

pytestmark = pytest.mark.gpu

CN = 130  # one workgroup: two full waves, a ragged one, an idle one


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


def timed(what, streams, t0):
    print("%s: %d channels, cap %d, stride %d, %.2f s" % (what, streams.C, streams.cap, streams.stride(), time.time() - t0))


@pytest.mark.parametrize("n", (40, 600, 3000))
def test_decode_host_on_the_damaged_corpus(ctx, n):
    """n = 40: a few codes and an end; 600: a list and a history worth the name; 3000: counts in the hundreds, long matches"""
    got, damaged = lc.check_not_vacuous(CN, n)
    t0 = time.time()
    lc.check_both(ctx.lzmh_decode_host, lc.corpus(CN, n))
    timed("corpus n=%d (differ %d, longer %d, shorter %d of %d damaged)" % (n, *got, damaged), lc.corpus(CN, n), t0)


@pytest.mark.parametrize("which", ("named", "every_cut", "token_soup", "copy_grid"))
def test_decode_host_on_the_assembler_sets(ctx, which):
    streams = getattr(lc, which)()
    t0 = time.time()
    lc.check_both(ctx.lzmh_decode_host, streams)
    timed(which, streams, t0)


def test_device_entry_slab_base_off_by_a_word_and_a_stream_that_ends_with_its_slab(ctx):
    """dega_hip_lzmh_decode_dev itself: cap a multiple of 4 but not of 16, the slabs' base 4 bytes into its allocation, the
    channel whose last bit is its slab's last bit in the last slab -- behind its last word the allocation ends, and the
    word the reading wave fetches ahead is that last word again.  Garbage behind every other stream."""
    import torch
    corp = lc.corpus(CN, 600)
    ending = int(np.flatnonzero(corp.bits == 8 * corp.cap)[0])
    streams = corp.pick([c for c in range(CN) if c != ending] + [ending])
    assert streams.cap == corp.cap and streams.cap % 4 == 0 and streams.cap % 16 != 0 and int(streams.bits[-1]) == 8 * streams.cap

    def decode(slabs, bits, stride):
        flat = torch.zeros(4 + slabs.size, dtype=torch.uint8, device="cuda")
        d_in = flat[4:].view(slabs.shape)
        d_in.copy_(torch.from_numpy(np.array(slabs)))
        assert d_in.data_ptr() % 16 == 4
        d_bits = torch.from_numpy(np.array(bits).view(np.int64)).cuda()
        out, lens, err = ctx.lzmh_decode(d_in, d_bits, stride)
        torch.cuda.synchronize()
        return out.cpu().numpy(), lens.cpu().numpy(), err.cpu().numpy()

    lc.check_both(decode, streams)


# ---- the end of the row --------------------------------------------------------------------------------------------------------
def test_a_channel_that_does_not_fit_its_row_reports_it_and_touches_no_other_row(ctx):
    """include/dega_hip.h: "ERROR_MEMORY when a channel does not fit its row".  The writer stores 8 bytes at a time and checks
    each store, at the end of a match as in the middle of one, so for a stride that is a multiple of 8 (the only kind the
    entry point takes): len <= stride -> status 0 and the bytes; len > stride -> ERROR_MEMORY and out_len 0
    (lzmh_hostile_common.check_boundary).  The code agrees with the header as it stands."""
    import torch

    def decode_rows(slabs, bits, stride, rows):
        d_in = torch.from_numpy(np.array(slabs)).cuda()
        d_bits = torch.from_numpy(np.array(bits).view(np.int64)).cuda()
        d_rows = torch.from_numpy(rows).cuda()
        _, lens, err = ctx.lzmh_decode(d_in, d_bits, stride, out=d_rows)
        torch.cuda.synchronize()
        rows[:] = d_rows.cpu().numpy()
        return lens.cpu().numpy(), err.cpu().numpy()

    lc.check_boundary(decode_rows)


# ---- the group's host pipeline ---------------------------------------------------------------------------------------------------
def packed_form(streams, form):
    """the streams back to back, ceil(bits / 8) bytes each (what dega_hip_group_lzmh_encode writes and the glzmh plugin reads
    from disk); of the garbage form the last byte's spare bits stay garbage"""
    nbytes = (streams.bits.astype(np.int64) + 7) // 8
    offsets = np.concatenate([[0], np.cumsum(nbytes)]).astype(np.uint64)
    packed = np.concatenate([streams.slabs[form][c, : int(nbytes[c])] for c in range(streams.C)] + [np.zeros(0, dtype=np.uint8)])
    return np.ascontiguousarray(packed), offsets


@pytest.mark.parametrize("devices", ([0], [0, 0]))
def test_group_decode_of_the_packed_corpus_equals_the_slab_call(dca, ctx, devices):
    """dega_hip_group_lzmh_decode: one member and two (both on device 0).  No chunk is narrower than min(C, 8192) channels
    whatever DEGA_PIPELINE_CHUNKS says: the corpus (130 channels) is one chunk per member, and the copy grid (12 000 cells)
    two chunks of 8 192 and 3 808 channels on one member, one chunk each on two.  More chunks: test_gpu_pipeline_chunks.py"""
    os.environ["DEGA_PIPELINE_CHUNKS"] = "3"
    g = dca.Group(devices)
    try:
        for streams in (lc.corpus(CN, 600), lc.corpus(CN, 3000), lc.copy_grid()):
            stride = (streams.stride() + 15) // 16 * 16
            for form in ("clean", "garbage"):
                want = lc.check(ctx.lzmh_decode_host, streams, form, stride)

                def decode(slabs, bits, stride):
                    packed, offsets = packed_form(streams, form)
                    return g.lzmh_decode_job(packed, offsets, bits, stride)

                got = lc.check(decode, streams, form, stride)
                # (both calls have passed the checker: every length, every status and every byte below a channel's length is
                # the oracle's.  Behind a channel's last 8-byte store the pipeline hands back what its scratch rows held.)
                assert (got[1] == want[1]).all() and (got[2] == want[2]).all(), (devices, form, streams.C)
    finally:
        g.close()
        del os.environ["DEGA_PIPELINE_CHUNKS"]


# ---- the chain into the csv reader -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (40, 600, 3000))
def test_chain_into_the_csv_reader_on_damaged_texts(ctx, n):
    """dega_hip_lzmh_decode_f32_dev on the corpus channels made from meter lines and from digits: what csv_read makes of
    lzmh_decode's text on the device, and what libc's strtof makes of the text the ORACLE decodes (csv_read_common.expected):
    counts, statuses and bit patterns.  The damaged texts hold what no csv test writes on purpose: NUL bytes from list
    entries never used, fields cut anywhere, runs of one byte."""
    import torch
    corp = lc.corpus(CN, n)
    streams = corp.pick([c for c in range(CN) if corp.sort[c] in (0, 1)])
    stride = (streams.stride() + 15) // 16 * 16
    max_T = stride  # (a text of `stride` bytes has no more values than that)
    want, status = zip(*[crc.expected(t) for t in streams.want])
    for form in ("clean", "garbage"):
        d_in = torch.from_numpy(np.array(streams.slabs[form])).cuda()
        d_bits = torch.from_numpy(np.array(streams.bits).view(np.int64)).cuda()
        v, count, tlen, err = ctx.lzmh_decode_f32(d_in, d_bits, stride, max_T)
        text, lens, derr = ctx.lzmh_decode(d_in, d_bits, stride)
        v2, count2, err2 = ctx.csv_read(text, lens, max_T)
        torch.cuda.synchronize()
        assert int((derr != 0).sum().item()) == 0 and torch.equal(tlen, lens)
        assert lens.cpu().numpy().tolist() == [len(t) for t in streams.want]
        assert torch.equal(count, count2) and torch.equal(err, err2)
        v, v2, count, err = v.cpu().numpy().view(np.uint32), v2.cpu().numpy().view(np.uint32), count.cpu().numpy(), err.cpu().numpy()
        values = crc.check_channels(v, count, err, want, status, max_T, ("chain", n, form))
        crc.check_channels(v2, count, err, want, status, max_T, ("lzmh_decode then csv_read", n, form))
    assert values > 0
    print("chain n=%d: %d channels, %d values, statuses %s" % (n, streams.C, values, sorted(set(status))))


# ---- the encoder: the longest match at every window alignment -----------------------------------------------------------------
def test_encoder_longest_match_at_every_window_alignment(ctx):
    """the 32 strings of test_lzmh_longest_match_at_every_window_alignment (tests/test_lzmh_kernel_sim.py: minutes under the
    emulator) through the HIP encoder, against the oracle; and back"""
    strings = lc.longest_match_strings()
    out, bits, err = ctx.lzmh_encode_host(strings)
    assert (err == 0).all()
    for i, s in enumerate(strings):
        b, n = lc.oracle_encode(s)
        assert int(bits[i]) == n and out[i, : (n + 7) // 8].tobytes() == b, (i, len(s))
    dec, lens, derr = ctx.lzmh_decode_host(out, bits, 8 * ((max(len(s) for s in strings) + 7) // 8))
    assert (derr == 0).all() and all(dec[i, : int(lens[i])].tobytes() == s for i, s in enumerate(strings))
