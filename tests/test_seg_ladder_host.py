"""Diff and exp-Golomb at every codeword length, without a GPU (tests/seg_ladder_common.py has the corpus, its conditions and
the checkers):
  * the corpus itself at all 13 value sizes: deterministic, every condition holds and is printed,
  * the oracle on it against tests/golden/seg_ladder.npz, which the compiled reference wrote,
  * the encode and decode kernels' source under the thread-per-lane emulator of tests/sim/ on the head of the batch -- both
    `plain` waves, a third wave and a ragged one, with every kind and both signs of the refused difference in them -- at
    value sizes 2, 15, 16, 17, 31, 32 (also at a row pitch of C + 7 and over several launches), 33 and 64."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import seg_ladder_common as sl
from oracle import orc

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "sim")
HEAD = 200  # channels 180, 188 and 196 are the first refused ones whose spoiled difference is the negative one
EMULATED = (2, 15, 16, 17, 31, 32, 33, 64)


# ---- the corpus ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vs", sl.SIZES)
def test_corpus_conditions(vs):
    corp = sl.corpus(vs)
    for what, value in sl.conditions(corp).items():
        print("%s: %s" % (what, value))
    assert corp.C == 390 and corp.T == sl.length(vs)
    assert {1: 32, 32: 157, 64: 282}.get(vs, corp.T) == corp.T


def test_corpus_is_deterministic_and_the_head_is_the_head():
    corp, again = sl.corpus(17), sl.Corpus(17)
    assert (again.x == corp.x).all() and (again.xin == corp.xin).all()
    head = corp.head(HEAD)
    assert (head.xin == corp.xin[:, :HEAD]).all() and sorted(set(head.kind[128:].tolist())) == list(range(8))
    assert [sl.refused(17, c, corp.T)[2] for c in head.refused_channels()].count(-1) == 3
    # kind 6 carries bits above the value size in its containers, and only there; masked they are the samples
    dirty = corp.xin.view(np.uint32).astype(np.uint64) != corp.x
    assert dirty[:, corp.kind == 6].any() and not dirty[:, corp.kind != 6].any() and not dirty[:, :128].any()
    assert ((corp.xin.view(np.uint32).astype(np.uint64) & np.uint64((1 << 17) - 1)) == corp.x).all()
    c40 = sl.corpus(40)
    assert ((c40.xin.view(np.uint64) != c40.x).any(axis=0) == ((c40.kind == 6) & (np.arange(c40.C) >= 128))).all()
    # the ragged batch: counts that cut inside, before and behind the longest codeword's pair, and whole channels
    n = corp.counts()
    assert n[2] == 0 and n[3] == 1 and (n[::4][1:] == corp.T).all() and (n < corp.T).sum() > corp.C // 2


# ---- the golden: the oracle against the compiled reference -------------------------------------------------------------------
def test_oracle_reproduces_the_reference_on_the_corpus():
    """tests/golden/seg_ladder.npz (tests/golden/make_golden_seg_ladder.py): the reference's own `encode diff` / `encode seg`
    / `encode bac [adaptive]` with valuesize=n and the three decodes, on one channel of every accepted kind and two refused
    ones per value size"""
    gold = np.load(os.path.join(HERE, "golden", "seg_ladder.npz"))
    chans = gold["channels"].tolist()
    assert chans == sl.golden_channels() and tuple(gold["sizes"].tolist()) == sl.SIZES
    lossy = {(int(s), int(m), int(i)): gold["lossy_dec"][n] for n, (s, m, i) in enumerate(gold["lossy"])}
    refused = 0
    for s, vs in enumerate(sl.SIZES):
        corp = sl.corpus(vs)
        digest = hashlib.sha256(np.ascontiguousarray(corp.x[:, chans]).tobytes()).digest()
        assert digest == gold["input_sha256"][s].tobytes(), ("the corpus is not the one the reference was given", vs)
        for m, ad in enumerate((1, 0)):
            out, bits, err = corp.encoded(ad)
            _, _, verdicts = corp.decoder_input(ad)
            for i, c in enumerate(chans):
                tag = (vs, ad, c)
                assert int(err[c]) == int(gold["err"][s, m, i]), tag
                if err[c] != 0:
                    assert err[c] == orc.ERROR_INVALID_VALUE
                    refused += 1
                    continue
                nb = int(gold["bits"][s, m, i])
                stream = out[c, : (nb + 7) // 8].tobytes()
                assert int(bits[c]) == nb, tag
                if ad:
                    assert stream == gold["vs%d.stream" % vs][i, : (nb + 7) // 8].tobytes(), tag
                else:
                    assert hashlib.sha256(stream).digest() == gold["static_sha256"][s, i].tobytes(), tag
                r, back = verdicts[c]
                assert r == 0 and (back == lossy.get((s, m, i), corp.x[:, c])).all(), tag
    # value size 64 refuses nothing: its two wrapped differences are coded, and lost, under both models
    assert refused == 2 * 2 * 12 and sorted(lossy) == [(12, m, i) for m in (0, 1) for i in (chans.index(156), chans.index(180))]


# ---- the emulator ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim():
    subprocess.run(["make", "-s", "-C", SIM_DIR], check=True)
    S = C.CDLL(os.path.join(SIM_DIR, "libdega_sim.so"))
    P, Z, I = C.c_void_p, C.c_size_t, C.c_int
    S.sim_encode_vs.argtypes = [P, Z, Z, Z, I, I, P, Z, P, P]
    S.sim_encode64.argtypes = [P, Z, Z, Z, I, I, P, Z, P, P]
    S.sim_decode_var_vs.argtypes = [P, Z, P, Z, Z, Z, I, I, P, P, P]
    S.sim_decode64.argtypes = [P, Z, P, Z, Z, Z, I, I, P, P, P]
    S.sim_encode_segments.argtypes = [P, Z, Z, Z, I, C.c_float, I, I, P, I, P, Z, P, P]
    return S


def emulated_encode(S, head, ad, xin=None, ld=None, cuts=None):
    xin = head.xin if xin is None else xin
    Cn, T, vs, cap = head.C, head.T, head.vs, head.cap
    ld = Cn if ld is None else ld
    out = np.zeros((Cn, cap), dtype=np.uint8)
    bits = np.zeros(Cn, dtype=np.uint64)
    err = np.zeros(Cn, dtype=np.int32)
    if cuts is not None:
        cu = np.array(cuts, dtype=np.uint64)
        S.sim_encode_segments(xin.ctypes.data, Cn, T, ld, 0, 0.0, ad, vs, cu.ctypes.data, len(cu), out.ctypes.data, cap, bits.ctypes.data, err.ctypes.data)
    else:
        (S.sim_encode64 if vs > 32 else S.sim_encode_vs)(xin.ctypes.data, Cn, T, ld, ad, vs, out.ctypes.data, cap, bits.ctypes.data, err.ctypes.data)
    return out, bits, err


def emulated_decode(S, head, ad, room):
    slabs, bits, _ = head.decoder_input(ad)
    slabs, bits = np.ascontiguousarray(slabs), np.ascontiguousarray(bits)
    Cn, vs = head.C, head.vs
    y = np.zeros((room, Cn), dtype=np.int64 if vs > 32 else np.int32)
    counts = np.zeros(Cn, dtype=np.uint64)
    err = np.zeros(Cn, dtype=np.int32)
    (S.sim_decode64 if vs > 32 else S.sim_decode_var_vs)(slabs.ctypes.data, head.cap, bits.ctypes.data, Cn, room, Cn, ad, vs, y.ctypes.data, counts.ctypes.data,
                                                         err.ctypes.data)
    return y, counts, err


@pytest.mark.parametrize("ad", (1, 0))
@pytest.mark.parametrize("vs", EMULATED)
def test_emulated_encoder(sim, vs, ad):
    head = sl.corpus(vs).head(HEAD)
    sl.check_encode(head, ad, *emulated_encode(sim, head, ad), what="emulator, one launch")


@pytest.mark.parametrize("ad", (1, 0))
@pytest.mark.parametrize("vs", EMULATED)
def test_emulated_decoder(sim, vs, ad):
    head = sl.corpus(vs).head(HEAD)
    sl.check_decode(head, ad, *emulated_decode(sim, head, ad, head.T + 3), what="emulator, room T + 3")


@pytest.mark.parametrize("vs", (32, 17))
def test_emulated_encoder_at_a_row_pitch_of_c_plus_7_and_over_several_launches(sim, vs):
    """the per-row fetch instead of the x4 one (what lies between the rows would be refused as a sample), and launch
    boundaries at rows 1, 7, 8, 9 and inside the ladder"""
    head = sl.corpus(vs).head(HEAD)
    wide = np.full((head.T, HEAD + 7), -1, dtype=np.int32)
    wide[:, :HEAD] = head.xin
    sl.check_encode(head, 1, *emulated_encode(sim, head, 1, xin=wide, ld=HEAD + 7), what="emulator, ld = C + 7")
    cuts = sl.segment_cuts(head.T)
    sl.check_encode(head, 1, *emulated_encode(sim, head, 1, cuts=cuts), what="emulator, cuts %s" % cuts)
