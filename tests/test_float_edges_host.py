"""The float boundary of the DEGA chain across float32, without a GPU: the reference's answers (tests/golden/float_edges.npz),
the oracle and the plain restatement of float_edges_common agree on every value of the corpus; the corpus meets its
conditions; and the kernels' source, run by the emulator, gives the same -- dega_normalize_kernel / dega_denormalize_kernel one
value per channel, the fused float entry of dega_encode_kernel (32-bit, narrow, 64-bit, counted and short-table forms) and the
fused float exit of dega_decode_kernel (four groups and eight pairs) on the channel sets."""
import ctypes as C
import os

import numpy as np
import pytest

import csv_read_common as crc
import float_edges_common as fe
from oracle import orc
from sim_build import sim_library

NAN = 0x7FC00000


@pytest.fixture(scope="module")
def fx():
    return fe.EdgeFixture()


def at(vs, factor, pattern):
    """the place of one bit pattern in the corpus"""
    bits, _ = fe.values(vs, factor)
    where = np.flatnonzero(bits == np.uint32(pattern))
    assert where.size, hex(pattern)
    return int(where[0])


def f32_bits(x):
    return int(fe.as_bits(np.array([x], dtype=np.float32))[0])


# ---- fixture, oracle, restatement -------------------------------------------------------------------------------------------

def test_fixture_is_not_blind(fx):
    """entries named literally (the arrays of the fixture are differences to the restatement, zero where it is right)"""
    for vs, want in ((32, 0), (17, 0), (64, 0x8000000000000000)):
        failed, fields = fx.normalized(vs, 100.0)
        for nan in (NAN, 0xFFC00000, 0x7F800001):  # a NaN passes the range check and is converted: 0, the indefinite at 64 bits
            i = at(vs, 100.0, nan)
            assert not failed[i] and int(fields[i]) == want, (vs, hex(nan))
    failed, fields = fx.normalized(32, 1.0)
    i = at(32, 1.0, 0x4F000000)  # 2^31 passes at 32 bits (the upper bound rounds up to it) and wraps
    assert not failed[i] and int(fields[i]) == 0x80000000
    i = at(32, 1.0, 0x4F000001)  # the next float does not pass
    assert failed[i] and int(fields[i]) == 0
    i = at(32, 1.0, f32_bits(-1e-30))  # -1e-30 becomes -0.5, which truncates to 0
    assert not failed[i] and int(fields[i]) == 0
    i = at(32, 1.0, f32_bits(2.5))  # a tie goes up: 2.5 + 0.5
    assert not failed[i] and int(fields[i]) == 3
    i = at(32, 1.0, f32_bits(-2.5))  # ... and down
    assert not failed[i] and int(fields[i]) == 0xFFFFFFFD
    i = at(32, 1.0, f32_bits(8388609.5))  # 2^23 + 1 + 0.5 is no float: the reading is 2^23 + 2 already, and + 0.5 rounds to even
    assert not failed[i] and int(fields[i]) == 8388610
    failed, fields = fx.normalized(32, 100.0)
    for pattern, field in ((0x7F800000, None), (0xFF800000, None), (f32_bits(1.005), 101), (f32_bits(2.675), 268), (f32_bits(0.005), 1), (f32_bits(0.015), 2)):  # (worked out in exact rational arithmetic: each product rounds onto k + 0.5)
        i = at(32, 100.0, pattern)
        assert (failed[i], int(fields[i])) == ((True, 0) if field is None else (False, field)), hex(pattern)
    # the classes stored in full say the same without the restatement
    z = fx.z
    lit = list(z["n32.f0.lit.in"])
    assert int(z["n32.f0.lit.status"][lit.index(NAN)]) == 0 and int(z["n32.f0.lit.int"][lit.index(NAN)]) == 0
    assert int(z["n32.f0.lit.status"][lit.index(0x7F800000)]) == fe.INVALID
    lit = list(z["n64.f0.lit.in"])
    assert int(z["n64.f0.lit.int"][lit.index(NAN)]) == 0x8000000000000000
    assert int(z["n64.f1.lit.int"][list(z["n64.f1.lit.in"]).index(0x5F000000)]) == 0x8000000000000000  # 2^63 passes at 64 bits
    # Denormalize: 2^24 + 1 lies between two floats and goes to the even one; a subnormal quotient is kept
    u = fe.integers(32)
    den = fx.denormalized(32, 1.0)
    assert int(den[list(u).index((1 << 24) + 1)]) == f32_bits(16777216.0) and int(den[list(u).index((1 << 24) + 3)]) == f32_bits(16777220.0)
    den = fx.denormalized(32, 3e38)
    for n in (1, 2, 3):
        assert int(den[list(u).index(n)]) == f32_bits(n / float(np.float32(3e38))) and 0 < int(den[list(u).index(n)]) < 0x00800000
    assert os.path.getsize(fe.FIXTURE) <= 472283


@pytest.mark.parametrize("vs", fe.VALUE_SIZES)
def test_fixture_oracle_and_restatement_agree(fx, vs):
    """status and integer of every value alone, the float of every integer: three ways, one answer"""
    for factor in [f for v, f in fe.KEYS if v == vs]:
        bits, cls = fe.values(vs, factor)
        ok, n = fe.normalize(bits, factor, vs)
        status, fields = orc.normalize_each(fe.as_f32(bits), factor, vs)
        failed, ref_fields = fx.normalized(vs, factor)
        assert ((status != 0) == ~ok).all() and (status[~ok] == fe.INVALID).all() and (failed == ~ok).all(), (vs, factor)
        wrong = np.flatnonzero((fields != n) | (ref_fields != n))
        assert wrong.size == 0, (vs, factor, fe.CLASSES[cls[wrong[0]]], hex(int(bits[wrong[0]])), hex(int(fields[wrong[0]])), hex(int(ref_fields[wrong[0]])), hex(int(n[wrong[0]])))
        # the oracle's stage on a stream: the values in range as one stream, and the first one out of range ends it
        r, data, nb = orc.stage("normalize", True, bits[ok].tobytes(), 32 * int(ok.sum()), valuesize=vs, factor=factor)
        assert r == 0 and (fe.unpack_fields(data, nb, vs) == n[ok]).all(), (vs, factor)
        if (~ok).any():
            r, _, _ = orc.stage("normalize", True, np.concatenate([bits[ok][:5], bits[~ok][:1]]).tobytes(), 32 * 6, valuesize=vs, factor=factor)
            assert r == fe.INVALID
        u = fe.integers(vs)
        want = fe.denormalize(u, factor, vs)
        assert fe.same_float_bits(fe.as_bits(orc.denormalize_each(u, factor, vs)), want).all(), (vs, factor)
        assert fe.same_float_bits(fx.denormalized(vs, factor), want).all(), (vs, factor)
    # the conversion of the integers to float32 against integer arithmetic
    u = fe.integers(vs)
    exact = fe.as_bits(np.array([fe.float_of_int(int(s)) for s in fe.sign_extend(u, vs)], dtype=np.float32))
    assert (fe.denormalize(u, 1.0, vs) == exact).all(), vs


@pytest.mark.parametrize("vs", fe.VALUE_SIZES)
def test_conditions_hold(vs):
    for factor in [f for v, f in fe.KEYS if v == vs]:
        assert fe.conditions(vs, factor) == [], (vs, factor)


def test_reference_chains_are_the_oracles(fx):
    """the thin sample of channels that went through the compiled reference: status, bits, stream and the floats back"""
    for vs, factor in fe.FUSED_IN_FIXTURE:
        for ad in (1, 0):
            v, kinds, want = fe.expected_channels(vs, factor, ad)
            k = "%s.%s.chain" % (fe.key(vs, factor), "ad" if ad else "st")
            idx, err, nbits, streams, back = (fx.z[k + s] for s in (".idx", ".err", ".bits", ".stream", ".back"))
            assert (err == 0).any() and (err != 0).any()
            for j, c in enumerate(idx):
                assert int(err[j]) == int(want.err[c]) and (err[j] != 0 or int(nbits[j]) == int(want.bits[c])), (vs, factor, ad, c, kinds[c])
                if err[j] == 0:
                    assert streams[j, : len(want.streams[c])].tobytes() == want.streams[c] and not streams[j, len(want.streams[c]):].any(), (vs, factor, ad, c)
                    _, fields = fe.normalize(v[:, c], factor, vs)
                    assert fe.same_float_bits(back[:, j] ^ fe.denormalize(fields, factor, vs), want.back[c]).all(), (vs, factor, ad, c)


def text_floats():
    """TEXT_LINES as `decode csv` reads them (libc's strtof, which the csv reader's tests hold to the reference): a batch
    [T, C] of bit patterns and a count per channel"""
    cols = [crc.expected(crc.lines_text(lines))[0] for lines in fe.TEXT_LINES]
    T = max(c.size for c in cols)
    v = np.full((T, len(cols)), 0x7F800000, dtype=np.uint32)  # (+inf behind every count: it must not be looked at)
    for c, col in enumerate(cols):
        v[: col.size, c] = col
    return v, np.array([c.size for c in cols], dtype=np.int64)


def text_expected(fx, vs, ad):
    """(Expected of the oracle on text_floats(), having checked it against what the reference made of the texts)"""
    v, count = text_floats()
    want = fe.Expected(v, vs, ad, 100.0, count=count)
    k = "text.n%d.%s" % (vs, "ad" if ad else "st")
    assert (fx.z[k + ".err"] == want.err).all() and sorted(set(want.err.tolist())) == [fe.INVALID, 0]
    for c in np.flatnonzero(want.err == 0):
        assert int(fx.z[k + ".bits"][c]) == int(want.bits[c]) and fx.z[k + ".stream"][c, : len(want.streams[c])].tobytes() == want.streams[c], (vs, ad, c)
    return v, count, want


def test_text_chain_of_the_reference_is_the_oracles(fx):
    for vs in fe.TEXT_SIZES:
        for ad in (1, 0):
            _, _, want = text_expected(fx, vs, ad)
            # nan / -nan lines are coded (as 0, as the indefinite at 64 bits), inf lines are not, 1e-40 and abc are 0
            # -- and 21474836.48 x 100 = 2^31 passes Normalize at 32 bits, wraps, and is more than diff takes as a first step
            assert want.err.tolist() == [0, 0, 0, fe.INVALID, 0, 0, 0, fe.INVALID] + ([fe.INVALID, fe.INVALID] if vs == 32 else [0, 0]), (vs, ad)


# ---- the kernels' source under the emulator -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sim():
    S = sim_library("dega")
    Z, P, I, F = C.c_size_t, C.c_void_p, C.c_int, C.c_float
    S.sim_normalize_vs.argtypes = [P, Z, Z, Z, F, I, P, P]
    S.sim_denormalize_vs.argtypes = [P, Z, Z, Z, F, I, P]
    S.sim_encode_f32.argtypes = [P, Z, Z, Z, F, I, I, P, Z, P, P]
    S.sim_encode_f32_short.argtypes = [P, Z, Z, Z, F, I, P, Z, P, P]
    S.sim_decode_f32.argtypes = [P, Z, P, Z, Z, Z, F, I, I, P, P, P]
    S.sim_decode_f32_wide.argtypes = [P, Z, P, Z, Z, Z, F, I, I, P, P, P]
    return S


@pytest.fixture(scope="module")
def sim_ragged():
    S = sim_library("ragged")
    Z, P = C.c_size_t, C.c_void_p
    S.sim_encode_f32_var.argtypes = [P, Z, Z, Z, P, C.c_float, C.c_int, C.c_int, P, Z, P, P]
    return S


@pytest.mark.parametrize("vs", [v for v in fe.VALUE_SIZES if v <= 32])
def test_standalone_kernels_on_every_value(sim, fx, vs):
    """dega_normalize_kernel and dega_denormalize_kernel, one value per channel (T = 1), so that every value has a verdict of
    its own; 4 133 channels and 4 096"""
    for factor in [f for v, f in fe.KEYS if v == vs]:
        bits, cls = fe.values(vs, factor)
        failed, fields = fx.normalized(vs, factor)
        u = fe.integers(vs)
        den = fx.denormalized(vs, factor)
        for Cn in (fe.N_VALUES, fe.N_ALIGNED) if factor in (100.0, 3.3) else (fe.N_VALUES,):  # (the emulator takes its time: two factors at both)
            v = np.ascontiguousarray(bits[:Cn])
            x = np.full(Cn, 0x5A5A5A5A, dtype=np.uint32)
            err = np.zeros(Cn, dtype=np.int32)
            assert sim.sim_normalize_vs(v.ctypes.data, Cn, 1, Cn, factor, vs, x.ctypes.data, err.ctypes.data) == 0
            wrong = np.flatnonzero(((err != 0) != failed[:Cn]) | ((err != 0) & (err != fe.INVALID)) | (~failed[:Cn] & (x != fields[:Cn].astype(np.uint32))))
            assert wrong.size == 0, (vs, factor, Cn, [(fe.CLASSES[cls[i]], hex(int(v[i])), int(err[i]), hex(int(x[i])), bool(failed[i]), hex(int(fields[i]))) for i in wrong[:4]])
            xin = np.ascontiguousarray(u[:Cn].astype(np.uint32))
            back = np.zeros(Cn, dtype=np.uint32)
            assert sim.sim_denormalize_vs(xin.ctypes.data, Cn, 1, Cn, factor, vs, back.ctypes.data) == 0
            same = fe.same_float_bits(back, den[:Cn])
            assert same.all(), (vs, factor, Cn, [(hex(int(xin[i])), hex(int(back[i])), hex(int(den[i]))) for i in np.flatnonzero(~same)[:4]])


def run_encode(fn, v, factor, ad, vs, cap, count=None):
    """fn: sim_encode_f32, sim_encode_f32_short (no model argument: adaptive) or sim_encode_f32_var (with count)"""
    v = np.ascontiguousarray(v, dtype=np.uint32)
    T, Cn = v.shape
    out = np.zeros((Cn, cap), dtype=np.uint8)
    bits = np.full(Cn, 99999, dtype=np.uint64)
    err = np.full(Cn, 77, dtype=np.int32)
    tail = (out.ctypes.data, cap, bits.ctypes.data, err.ctypes.data)
    if count is not None:
        count = np.ascontiguousarray(count, dtype=np.uint64)
        assert fn(v.ctypes.data, Cn, T, Cn, count.ctypes.data, factor, ad, vs, *tail) == 0
    elif ad is None:
        assert fn(v.ctypes.data, Cn, T, Cn, factor, vs, *tail) == 0
    else:
        assert fn(v.ctypes.data, Cn, T, Cn, factor, ad, vs, *tail) == 0
    return out, bits, err


def run_decode(fn, slabs, sbits, T, factor, ad, vs):
    Cn, cap = slabs.shape
    back = np.zeros((T, Cn), dtype=np.uint32)
    counts = np.zeros(Cn, dtype=np.uint64)
    derr = np.full(Cn, 77, dtype=np.int32)
    assert fn(slabs.ctypes.data, cap, sbits.ctypes.data, Cn, T, Cn, factor, ad, vs, back.ctypes.data, counts.ctypes.data, derr.ctypes.data) == 0
    return back, counts, derr


def test_nan_reading_is_coded_as_zero(sim):
    """the channel [1.0, 2.0, NaN, 3.0] at 32 bits, factor 100: the reference writes the sample 00000000 for the NaN and codes
    the channel in 65 bits"""
    v = fe.as_bits(np.array([1.0, 2.0, np.nan, 3.0], dtype=np.float32)).reshape(4, 1)
    want = fe.Expected(v, 32, 1, 100.0)
    assert int(want.err[0]) == 0 and int(want.bits[0]) == 65
    r, data, n = orc.stage("normalize", True, v.tobytes(), 128, valuesize=32, factor=100.0)
    assert r == 0 and data[:16].hex() == "00000064" "000000c8" "00000000" "0000012c"
    want.check_streams(*run_encode(sim.sim_encode_f32, v, 100.0, 1, 32, want.cap), "nan channel")


@pytest.mark.parametrize("vs,factor", fe.FUSED)
def test_fused_float_entry_and_exit(sim, vs, factor):
    """sim_encode_f32 / sim_decode_f32 as the library launches them on the channel sets, both models: status, bits and bytes
    per channel against the oracle's chain, floats back against its inverse chain; below 33 bits also the short-table entry
    and the eight-pair exit"""
    for ad in (1, 0):
        v, kinds, want = fe.expected_channels(vs, factor, ad)
        want.check_streams(*run_encode(sim.sim_encode_f32, v, factor, ad, vs, want.cap), (vs, factor, ad), kinds)
        slabs, sbits = want.slabs()
        back, counts, derr = run_decode(sim.sim_decode_f32, slabs, sbits, want.T, factor, ad, vs)
        assert (counts[want.err == 0] == want.T).all()
        want.check_back(back, derr, (vs, factor, ad), kinds)
        if vs <= 32:
            if ad:
                want.check_streams(*run_encode(sim.sim_encode_f32_short, v, factor, None, vs, want.cap), (vs, factor, "short table"), kinds)
            back, counts, derr = run_decode(sim.sim_decode_f32_wide, slabs, sbits, want.T, factor, ad, vs)
            want.check_back(back, derr, (vs, factor, ad, "eight pairs"), kinds)


@pytest.mark.parametrize("vs", fe.FUSED_SIZES)
def test_fused_float_exit_on_integer_series(sim, vs):
    """the decoders' row write on integers over the whole range of the value size: sign extension, the conversion to float32
    (above 2^24 it rounds; integers exactly between two floats), the division -- by 100, and by 3e38 for subnormal quotients"""
    for factor, ad in ((100.0, 1), (1.0, 0), (3e38, 1)):
        want = fe.expected_series(vs, ad, factor)
        back, counts, derr = run_decode(sim.sim_decode_f32, want.slabs, want.bits, want.T, factor, ad, vs)
        assert (counts == want.T).all()
        want.check_back(back, derr, (vs, factor, ad))
        if vs <= 32:
            back, counts, derr = run_decode(sim.sim_decode_f32_wide, want.slabs, want.bits, want.T, factor, ad, vs)
            want.check_back(back, derr, (vs, factor, ad, "eight pairs"))
    # (the last but one channel is all codewords of the longest kind: more than 65 bits a sample above 32 bits, which the decoder has to take)
    r, data, n = orc.stage("diff", True, *fe.pack_fields(fe.series(vs)[:, -2], vs), valuesize=vs)
    r, data, n = orc.stage("seg", True, data, n, valuesize=vs)
    assert r == 0 and n >= fe.T_ROWS * (2 * min(vs, 63) - 1)
    sub = fe.as_f32(fe.expected_series(vs, 1, 3e38).back)
    assert np.unique(sub[(sub != 0) & (np.abs(sub) < np.float32(1.17549435e-38))]).size == (6 if vs > 2 else 2)  # +-1 .. +-3 over 3e38: all the subnormal quotients there are, kept


@pytest.mark.parametrize("vs,factor", [(32, 100.0), (17, 3.3), (26, 0.5), (40, -100.0), (64, 100.0)])
def test_counted_float_entry(sim_ragged, vs, factor):
    """counts 1 .. T; an infinity, a value out of range or a NaN behind a channel's count changes nothing"""
    v, count = fe.counts_and_poison(vs, factor)
    for ad in (1, 0):
        want = fe.Expected(v, vs, ad, factor, count=count)
        assert (want.err == 0).all()
        want.check_streams(*run_encode(sim_ragged.sim_encode_f32_var, v, factor, ad, vs, want.cap, count=count), (vs, factor, ad, "counted"))


def test_text_chain_through_the_counted_entry(sim_ragged, fx):
    for vs in fe.TEXT_SIZES:
        for ad in (1, 0):
            v, count, want = text_expected(fx, vs, ad)
            want.check_streams(*run_encode(sim_ragged.sim_encode_f32_var, v, 100.0, ad, vs, want.cap, count=count), ("text", vs, ad))
