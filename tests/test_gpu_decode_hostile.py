"""The HIP decoders on damaged streams (-m gpu): the corpus and the checker of tests/hostile_common.py -- status, count and
every sample the oracle's, channel by channel, with every kind of damage next to healthy lanes in every wave -- through the
host entries (value sizes 5 .. 64, both models, with and without garbage behind the streams), the device entry with an odd
pitch and a slab that ends with its longest stream, the fixed-count entry, the float exit and the wide workgroup shape."""
import time

import numpy as np
import pytest

import hostile_common as hc
from __graft_entry__ import load_package
from oracle import orc

pytestmark = pytest.mark.gpu

CN = 130  # two full waves and a ragged one


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


def both_forms(decode_var, corp, what):
    """the checker on the clean and on the garbage form; the two results are the same arrays wherever they are defined"""
    t0 = time.time()
    clean, s1 = hc.check(decode_var, corp, "clean")
    garbage, s2 = hc.check(decode_var, corp, "garbage")
    assert hc.same_where_defined(clean, garbage), (what, corp.vs, corp.ad, corp.T, "the result depends on what lies beyond the stream's exact length")
    print("%s vs=%d ad=%d T=%d: refused %d, excused %d + %d, room %d, %.2f s" % (what, corp.vs, corp.ad, corp.T, s1["refused"], s1["excused"], s2["excused"], s1["room"],
                                                                               time.time() - t0))


@pytest.mark.parametrize("vs", (32, 31, 12, 5, 33, 48, 64))
def test_corpus_holds_every_ending(vs):
    """(the oracle alone; the corpora made here are the ones the tests below decode)"""
    for ad in (1, 0):
        got, damaged = hc.check_not_vacuous(CN, vs, ad)
        print("corpus C=%d vs=%d ad=%d: wrong samples %d, refused -3 %d, refused -11 %d, of %d damaged" % (CN, vs, ad, *got, damaged))


@pytest.mark.parametrize("vs,T", ((32, 33), (32, 300), (32, 3000), (31, 33), (31, 300), (12, 33), (12, 300), (5, 33), (5, 300)))
def test_decode_var_host_on_damaged_streams(ctx, vs, T):
    """T = 33: one word and a symbol; 300: the steady word path, cuts inside a word; 3000: past the first halvings of the counts"""
    for ad in (1, 0):
        both_forms(lambda slabs, bits, room: ctx.decode_var_host(slabs, bits, room, adaptive=ad, valuesize=vs), hc.corpus(CN, T, vs, ad), "decode_var_host")


@pytest.mark.parametrize("vs", (33, 48, 64))
@pytest.mark.parametrize("T", (33, 300))
def test_decode64_var_host_on_damaged_streams(ctx, vs, T):
    """SegParser64 and the 64-bit sample ring: codewords of up to 127 bits, a zero-prefix cap of their own"""
    for ad in (1, 0):
        both_forms(lambda slabs, bits, room: ctx.decode64_var_host(slabs, bits, room, vs, adaptive=ad), hc.corpus(CN, T, vs, ad), "decode64_var_host")


def test_named_cut_streams_and_stumps(ctx):
    """the named cases of hostile_common.NAMED_CUT_STREAMS: -3 and nothing else, in rows that a decoder which went on into
    the zeros behind the stream would overrun"""
    def decode_var_for(vs, ad):
        if vs > 32:
            return lambda slabs, bits, room: ctx.decode64_var_host(slabs, bits, room, vs, adaptive=ad)
        return lambda slabs, bits, room: ctx.decode_var_host(slabs, bits, room, adaptive=ad, valuesize=vs)
    hc.check_named_cut_streams(decode_var_for)
    hc.check_named_stumps(decode_var_for, (32, 12, 48))  # and the ending the adaptive corpus is short of: seg's short read, -11


def test_device_entry_odd_pitch_misaligned_base_and_a_stream_that_ends_with_its_slab(ctx, dca):
    """dega_hip_decode_var_dev itself: ld = C + 5, the output's base off by one dword, the slabs exactly as long as the longest
    stream needs (a multiple of 4 bytes; one lengthened stream's last bit is its slab's last bit, and the last slab ends
    the allocation), garbage behind every other stream.  Columns >= C and rows >= room keep the sentinel."""
    import torch
    lib = dca.library()
    for ad in (1, 0):
        corp = hc.corpus(CN, 300, 32, ad)
        assert corp.cap % 4 == 0 and (corp.bits == 8 * corp.cap).sum() == 1
        seen = {}

        def decode_var(slabs, bits, room):
            ld, rows = CN + 5, room + 8
            flat = torch.full((rows * ld + 8,), -9, dtype=torch.int32, device="cuda")
            view = flat[1: 1 + rows * ld].view(rows, ld)
            d_in = torch.from_numpy(np.ascontiguousarray(slabs)).cuda()
            d_bits = torch.from_numpy(np.ascontiguousarray(bits).view(np.int64)).cuda()
            counts = torch.zeros(CN, dtype=torch.int64, device="cuda")
            err = torch.zeros(CN, dtype=torch.int32, device="cuda")
            ret = lib.dega_hip_decode_var_dev(ctx._h, d_in.data_ptr(), corp.cap, d_bits.data_ptr(), CN, room, ld, ad, 32, view.data_ptr(), counts.data_ptr(),
                                              err.data_ptr(), None)
            assert ret == 0
            torch.cuda.synchronize()
            seen["flat"], seen["view"], seen["counts"] = flat.cpu().numpy(), view.cpu().numpy(), counts.cpu().numpy()
            return seen["view"][:room, :CN], seen["counts"].astype(np.uint64), err.cpu().numpy()

        (y, counts, err), stats = hc.check(decode_var, corp, "garbage")
        room = stats["room"]
        assert (seen["view"][:, CN:] == -9).all(), "the decoder wrote outside its C columns"
        assert (seen["view"][room:] == -9).all(), "the decoder wrote below its last row"
        assert seen["flat"][0] == -9 and (seen["flat"][1 + (room + 8) * (CN + 5):] == -9).all()
        # rows a wave does write: up to its longest channel, zeros below a shorter channel's last sample
        healthy = corp.kind == 0
        assert (err[healthy] == 0).all() and (counts[healthy] == corp.T).all()
        assert (y[: corp.T, healthy].view(np.uint32) == corp.x[:, healthy]).all()
        print("decode_var_dev ad=%d: %s" % (ad, stats))


def fixed_count_expectation(corp, c, T):
    """What the fixed-count form of the fused decoder says about channel c, from the oracle's stages, and the rule that
    makes it differ from orc.decode_batch_tc's code (None: it does not).  DESIGN.md 4.2 states the rules."""
    n = int(corp.bits[c])
    r, want = corp.verdict(c)
    if r == 0:
        if len(want) > T:
            return orc.ERROR_INVALID_FORMAT, "count"  # the restatement's batch call says ERROR_MEMORY: its word for `more than asked for`
        return (0 if len(want) == T else orc.ERROR_INVALID_FORMAT), None
    if r == orc.ERROR_LIBRARY_CALL:
        # seg's short read comes at the very end of its input; the fused decoder has counted the whole codewords before it
        rb, seg, nseg = orc.stage("bac", False, corp.slabs["clean"][c, : (n + 7) // 8].tobytes(), n, adaptive=corp.ad)
        assert rb == 0
        if hc.whole_codewords(seg, nseg, corp.vs) > T:
            return orc.ERROR_INVALID_FORMAT, "count before the stump"
    return r, None


def stump_streams(x_col, T, ad):
    """named cases for the second rule, which the seeded corpus does not reach: seg streams of T + 2, T and T - 1 whole
    codewords followed by a codeword cut short inside its residual (hostile_common.stump_stream)"""
    longer = np.concatenate([x_col, x_col[-1:] + np.uint64(1), x_col[-1:] + np.uint64(2)])
    return hc.slabs_of([hc.stump_stream(longer[:n], 32, ad) for n in (T + 2, T, T - 1)])


@pytest.mark.parametrize("T", (33, 300))
def test_fixed_count_decode_on_damaged_streams(ctx, T):
    """decode_host(..., T) against orc.decode_batch_tc: the same channels accepted, the same samples, the same codes where both
    refuse -- but for two named rules of the fused decoder's order of checks (fixed_count_expectation)."""
    for ad in (1, 0):
        corp = hc.corpus(CN, T, 32, ad)
        oy, oerr = orc.decode_batch_tc(corp.slabs["clean"], corp.bits, T, ad)
        used = {"count": 0, "count before the stump": 0}
        for form in ("clean", "garbage"):
            y, derr = ctx.decode_host(corp.slabs[form], corp.bits, T, adaptive=ad)
            for c in range(CN):
                tag = (ad, T, form, c, corp.made_from[c])
                want, rule = fixed_count_expectation(corp, c, T)
                assert (want == 0) == (oerr[c] == 0), tag
                if rule is None:
                    assert want == oerr[c], tag
                elif rule == "count":
                    assert oerr[c] == orc.ERROR_MEMORY, tag
                else:
                    assert oerr[c] == orc.ERROR_LIBRARY_CALL, tag
                if rule is not None:
                    used[rule] += 1
                assert derr[c] == want, (tag, int(derr[c]), want, int(oerr[c]), rule)
                if want == 0:
                    assert (y[:, c] == oy[:, c]).all(), tag
            healthy = corp.kind == 0
            assert (derr[healthy] == 0).all() and (y[:, healthy].view(np.uint32) == corp.x[:, healthy]).all()
        # the second rule by name: more than T whole codewords before the stump -> the count is what the fused decoder trips
        # over (-3); T or fewer -> the stump itself (-11), as in the stage-wise chain
        slabs, bits = stump_streams(corp.x[:, 0], T, ad)
        _, oerr3 = orc.decode_batch_tc(slabs, bits, T, ad)
        _, derr3 = ctx.decode_host(slabs, bits, T, adaptive=ad)
        assert oerr3.tolist() == [orc.ERROR_LIBRARY_CALL] * 3
        assert derr3.tolist() == [orc.ERROR_INVALID_FORMAT, orc.ERROR_LIBRARY_CALL, orc.ERROR_LIBRARY_CALL], (T, ad, derr3.tolist())
        print("decode_host T=%d ad=%d: accepted %d, refused -3 %d, -11 %d; rules used (both forms) %s" % (
            T, ad, int((oerr == 0).sum()), int((derr == -3).sum()), int((derr == -11).sum()), used))


@pytest.mark.parametrize("T", (33, 300))
def test_float_exit_on_damaged_streams(ctx, T):
    """decode_f32(var=True): the statuses and the counts of the integer call, and (float)n / factor of its samples, byte for
    byte -- the denormalize fused into the row write sees every damaged lane the integer write sees"""
    import torch
    for ad in (1, 0):
        corp = hc.corpus(CN, T, 32, ad)
        (y, counts, err), stats = hc.check(lambda slabs, bits, room: ctx.decode_var_host(slabs, bits, room, adaptive=ad), corp, "garbage")
        room = stats["room"]
        d_in = torch.from_numpy(np.ascontiguousarray(corp.slabs["garbage"])).cuda()
        d_bits = torch.from_numpy(np.ascontiguousarray(corp.bits).view(np.int64)).cuda()
        v, fcounts, ferr = ctx.decode_f32(d_in, d_bits, room, factor=100.0, adaptive=ad, var=True)
        torch.cuda.synchronize()
        v, fcounts, ferr = v.cpu().numpy(), fcounts.cpu().numpy(), ferr.cpu().numpy()
        ok = err == 0
        assert (ferr == err).all() and (fcounts[ok].astype(np.uint64) == counts[ok]).all(), (T, ad)
        want = (y.astype(np.float32) / np.float32(100.0)).astype(np.float32)  # (float)n / factor, normalize.c:38
        valid = (np.arange(room, dtype=np.uint64)[:, None] < counts[None, :]) & ok[None, :]  # (rows beyond a count are not defined)
        assert v.view(np.uint32)[valid].tobytes() == want.view(np.uint32)[valid].tobytes(), (T, ad)
        assert ok.sum() > CN // 4 and (counts[ok] != T).any()  # accepted channels, some of them not of the encoder's making


def test_wide_workgroups_on_damaged_streams(ctx):
    """More than 64 Ki channels: 8 pairs of waves, the coding wave stages its own words.  The healthy channels are exact
    everywhere; every 997th channel (997 = 7 mod 10: the kinds in turn) is held to the oracle."""
    Cn, T = 65600, 33
    corp = hc.corpus(Cn, T, 32, 1)
    room = 2 * int(corp.bits.max()) + 64
    sample = [c for c in range(0, Cn, 997) if corp.kind[c] != 0] + [c for c in range(Cn - 64, Cn) if corp.kind[c] != 0]
    (y, counts, err), stats = hc.check(lambda slabs, bits, room: ctx.decode_var_host(slabs, bits, room, adaptive=1), corp, "garbage", channels=sample, room=room)
    healthy = corp.kind == 0
    assert (err[healthy] == 0).all() and (counts[healthy] == T).all()
    assert (y[:T, healthy].view(np.uint32) == corp.x[:, healthy]).all()
    assert len(set(int(corp.kind[c]) for c in sample)) == 9 and stats["refused"] >= len(sample) // 4
    print("wide: %d damaged channels sampled, %s" % (len(sample), stats))
