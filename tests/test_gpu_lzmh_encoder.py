"""The HIP LZMH encoder on steered texts (-m gpu): the corpus and the checkers of tests/lzmh_encoder_common.py -- status 0, the
oracle's exact bit length and the oracle's bytes for every channel, whatever lies behind a channel's length -- through the
host entry, the device entry on rows that end with their tensor, the end of the slab, the group's host pipeline, and back
through the decoder.  What the emulator of tests/test_lzmh_encoder_host.py does not model is tried here: the alignbyte,
alignbit and bitop3 forms, ctz on the device, and the timing between the searching and the coding wave."""
import time

import numpy as np
import pytest

import lzmh_encoder_common as ec
import lzmh_hostile_common as lc
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

CN = 130  # one workgroup: two full pairs of waves, a ragged one, an idle one


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


def device_entry(ctx):
    """encode of the checker: dega_hip_lzmh_encode_dev on a rows tensor of exactly C x stride bytes"""
    import torch

    def encode(rows, lens, cap):
        d_rows = torch.from_numpy(np.array(rows)).cuda()
        d_lens = torch.from_numpy(np.array(lens).view(np.int64)).cuda()
        assert tuple(d_rows.shape) == rows.shape and d_rows.data_ptr() % 16 == 0
        out, bits, err = ctx.lzmh_encode(d_rows, d_lens, cap=cap)
        torch.cuda.synchronize()
        return out.cpu().numpy(), bits.cpu().numpy().view(np.uint64), err.cpu().numpy()
    return encode


@pytest.mark.parametrize("n", (40, 600, 3000))
def test_encode_host_on_the_corpus(dca, ctx, n):
    """dega_hip_lzmh_encode_host builds its own rows from the strings: the clean form"""
    got = ec.check_not_vacuous(CN, n)
    corp = ec.corpus(CN, n)
    assert ec.worst_case_bytes(corp.stride) == dca.lzmh_worst_case_bytes(corp.stride)
    t0 = time.time()
    ec.check(lambda rows, lens, cap: ctx.lzmh_encode_host([corp.seen(c) for c in range(CN)], cap), corp, "clean")
    print("host entry n=%d: %.2f s; %s" % (n, time.time() - t0, ", ".join("%s %d" % (name, v) for name, v in zip(ec.EVENTS, got.tolist()))))


@pytest.mark.parametrize("n", (40, 600, 3000))
def test_device_entry_on_all_forms(ctx, n):
    """the rows are exactly C x stride bytes and the last channel fills its row: nothing of this batch lies behind it"""
    ec.check_not_vacuous(CN, n)
    corp = ec.corpus(CN, n)
    assert int(corp.lens[CN - 1]) == corp.stride
    t0 = time.time()
    ec.check_all_forms(device_entry(ctx), corp)
    print("device entry n=%d: %.2f s" % (n, time.time() - t0))


def test_device_entry_on_all_forms_with_a_second_ragged_workgroup(ctx):
    ec.check_not_vacuous(300, 600)
    corp = ec.corpus(300, 600)
    assert int(corp.lens[299]) == corp.stride
    ec.check_all_forms(device_entry(ctx), corp)


def test_a_stream_that_does_not_fit_its_slab_reports_it_and_touches_no_other_slab(ctx):
    """include/dega_hip.h: a channel whose stream, in whole 32-bit words, and 16 bytes more fit cap is coded; one whose stream
    does not fit cap reports ERROR_MEMORY and out_bits 0; in between either (lzmh_encoder_common.check_slab_end).  The slabs
    are the test's own, filled with a canary, one canary row behind the last."""
    import torch

    def encode_rows(rows, lens, cap, out):
        d_rows = torch.from_numpy(np.array(rows)).cuda()
        d_lens = torch.from_numpy(np.array(lens).view(np.int64)).cuda()
        d_out = torch.from_numpy(out).cuda()
        _, bits, err = ctx.lzmh_encode(d_rows, d_lens, cap=cap, out=d_out[: rows.shape[0]])
        torch.cuda.synchronize()
        out[:] = d_out.cpu().numpy()
        return bits.cpu().numpy().view(np.uint64), err.cpu().numpy()

    for form in ("continued", "garbage"):
        ec.check_slab_end(encode_rows, CN, form)
    rows, lens, cap, (want, nb) = ec.tightest_fit()
    out = np.full((2, cap), ec.CANARY, dtype=np.uint8)
    bits, err = encode_rows(rows, lens, cap, out)
    assert err[0] == 0 and int(bits[0]) == nb and out[0, : len(want)].tobytes() == want
    assert (out[0, len(want):] == ec.CANARY).all() and (out[1] == ec.CANARY).all()


@pytest.mark.parametrize("devices", ([0], [0, 0]))
def test_group_encode_of_the_corpus_equals_the_slab_call(dca, ctx, devices):
    """dega_hip_group_lzmh_encode on one member and on two (both on device 0): the packed streams are the slab call's and the
    oracle's, stream by stream, on the forms with something behind the lengths"""
    corp = ec.corpus(CN, 600)
    want_out, want_bits, want_err = ec.check(device_entry(ctx), corp, "clean")
    g = dca.Group(devices)
    try:
        for form in ("garbage", "continued"):
            packed, offsets, bits, err = g.lzmh_encode_job(np.array(corp.rows[form]), corp.lens)
            assert (err == 0).all() and (bits == want_bits).all(), (devices, form)
            assert int(offsets[0]) == 0 and (np.diff(offsets.astype(np.int64)) == (bits.astype(np.int64) + 7) // 8).all()
            for c in range(CN):
                stream = packed[int(offsets[c]): int(offsets[c + 1])].tobytes()
                assert stream == corp.want[c][0] and stream == want_out[c, : len(stream)].tobytes(), (devices, form, c, ec.KINDS[c % 8])
    finally:
        g.close()


@pytest.mark.parametrize("n", (40, 600, 3000))
def test_every_stream_decodes_to_what_the_oracle_decodes_it_to(ctx, n):
    """not always the input: a text of 403 bytes encodes to nothing, and nothing decodes to one zero byte"""
    corp = ec.corpus(CN, n)
    out, bits, err = ec.check(device_entry(ctx), corp, "continued")
    want = [lc.oracle_decode(*corp.want[c]) for c in range(CN)]
    stride = max(8, (max(len(w) for w in want) + 7) // 8 * 8)
    dec, lens, derr = ctx.lzmh_decode_host(out, bits, stride)
    plain = 0
    for c in range(CN):
        assert derr[c] == 0 and int(lens[c]) == len(want[c]) and dec[c, : len(want[c])].tobytes() == want[c], (c, ec.KINDS[c % 8])
        plain += want[c] == corp.seen(c)
    assert plain >= CN - 6  # (the empty and the 403-byte texts)
