"""The DEGA encoder on steered inputs, without a GPU (tests/encoder_regimes_common.py has the corpus, its conditions and
the checkers):
  * the corpus itself: deterministic, the replay's stream is the oracle's on every channel, every condition holds -- the
    rare paths are the common ones --, the restatement's streams are the compiled reference's where that is built,
  * the encode kernel's source under the thread-per-lane emulator of tests/sim/: one launch at the full slab, several
    launches with cuts where the long runs of owed bits are settled, one launch into slabs too short for the streams,
  * the same calls as a stand-alone program under the address and undefined-behaviour sanitizers.
T = 600, C = 200: three waves and a ragged one."""
import ctypes as C
import os
import struct
import subprocess
import time

import numpy as np
import pytest

import encoder_regimes_common as rc
from oracle import orc

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "sim")
CN, T = 200, 600
MAGIC = 0x53454d49474552


@pytest.fixture(scope="module")
def corp():
    return rc.corpus(CN, T)


@pytest.fixture(scope="module")
def sim():
    subprocess.run(["make", "-s", "-C", SIM_DIR], check=True)
    S = C.CDLL(os.path.join(SIM_DIR, "libdega_sim.so"))
    S.sim_encode.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    S.sim_encode_segments.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    return S


def emulated(S, x, ad, cap, cuts=None):
    Tn, Cn = x.shape
    out = np.zeros((Cn, cap), dtype=np.uint8)
    bits = np.zeros(Cn, dtype=np.uint64)
    err = np.zeros(Cn, dtype=np.int32)
    if cuts is None:
        S.sim_encode(x.ctypes.data, Cn, Tn, Cn, ad, out.ctypes.data, cap, bits.ctypes.data, err.ctypes.data)
    else:
        cu = np.array(cuts, dtype=np.uint64)
        S.sim_encode_segments(x.ctypes.data, Cn, Tn, Cn, 0, 0.0, ad, 32, cu.ctypes.data, len(cu), out.ctypes.data, cap, bits.ctypes.data, err.ctypes.data)
    return out, bits, err


# ---- the corpus ------------------------------------------------------------------------------------------------------------
def test_corpus_is_deterministic_and_a_smaller_batch_is_the_head_of_a_larger_one(corp):
    again = rc.Corpus(CN, T)
    assert (again.x == corp.x).all()
    assert (rc.Corpus(20, T).x == corp.x[:, :20]).all()
    assert sorted(set(corp.kind[:64].tolist())) == list(range(8))
    # every sample but kind 6's is below 2^23: exact in float32, and so is the sample + 0.5 (the float entry is tested on those)
    assert corp.x[:, corp.kind != 6].min() >= 0 and corp.x[:, corp.kind != 6].max() < (1 << 23)
    assert (corp.x.view(np.uint32)[:, corp.kind == 6] >= (1 << 31)).any()


def test_replay_reproduces_the_oracle_and_the_conditions_hold(corp):
    for ad in (1, 0):
        for c in range(CN):
            corp.trace(c, ad)  # asserts: the replay's stream is the oracle's, bit for bit
    t = corp.trace(4)
    pend, row = t.pending_of_every_bit()
    assert len(pend) == len(row) == t.nbits and int(pend.max()) == int(t.ev_pend.max())
    for what, value in rc.conditions(corp).items():
        print("%s: %s" % (what, value))
    for cap in rc.CAPS:
        print("cap %d: %d channels with a carry after >= 33 owed bits beyond it" % (cap, rc.check_short_is_not_vacuous(corp, cap)))
    cuts = corp.cuts()
    print("cuts:", cuts)
    assert cuts[0] == 0 and cuts[-1] == T and any(b - a == 1 for a, b in zip(cuts, cuts[1:]))
    # the static model: the same series, no condition (rc's docstring) -- what it does reach, for the record
    print("static model: longest run of owed bits %d" % max(int(corp.trace(c, 0).ev_pend.max()) for c in range(CN)))


def test_restatement_equals_the_compiled_reference_on_the_corpus(corp):
    """(oracle/_ref/libdcref.so is built where the reference's sources are; elsewhere the golden vectors made from it pin
    the restatement, tests/test_oracle_golden.py)"""
    if not orc.have_ref():
        pytest.skip("oracle/_ref/libdcref.so is built where the reference's sources are; elsewhere the golden vectors stand for it")
    for ad in (1, 0):
        out, bits, _ = corp.oracle(ad)
        for c in range(CN):
            ret, stream, n, _ = orc.ref_encode_i32(corp.x[:, c], ad)
            assert ret == 0 and n == int(bits[c]) and stream == out[c, : (n + 7) // 8].tobytes(), (ad, c, rc.KINDS[c % 8])


# ---- the emulator ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ad", (1, 0))
def test_emulated_encoder_at_the_full_slab(sim, corp, ad):
    rc.check_full(corp, ad, *emulated(sim, corp.x, ad, corp.cap), what="one launch")


@pytest.mark.parametrize("ad", (1, 0))
def test_emulated_encoder_over_several_launches_cut_inside_the_runs(sim, corp, ad):
    """cuts from the replay: the row where a run of >= 100 owed bits is settled, the row before it, a single-row range inside
    the run -- the held-back word and the collector cross launches while they are all ones"""
    rc.check_full(corp, ad, *emulated(sim, corp.x, ad, corp.cap, cuts=corp.cuts()), what="cuts %s" % corp.cuts())


@pytest.mark.parametrize("cap", rc.CAPS)
@pytest.mark.parametrize("ad", (1, 0))
def test_emulated_encoder_into_a_short_slab(sim, corp, ad, cap):
    """The short-slab contract: ERROR_MEMORY, the oracle's length, and the stream's own bytes in front of the cap -- with
    carries arriving beyond the cap after runs of owed bits that reach back over whole words (asserted from the replay).
    A writer that takes every word it dropped for all ones lets such a carry run into the last words it kept:
    BacWriter::ripple_carry_from did, and every adaptive case here failed (at cap 64 channel 4 differed from byte 56 on,
    channels 12, 29 and 36 in byte 63, ...).  The static cases pin the contract; the static model builds no such runs."""
    rc.check_short_is_not_vacuous(corp, cap)
    rc.check_short(corp, ad, cap, *emulated(sim, corp.x, ad, cap), what="short slab")


@pytest.mark.parametrize("ad", (1, 0))
def test_emulated_encoder_over_several_launches_into_a_short_slab(sim, corp, ad):
    """what the writer knows about the words it dropped travels with the saved state"""
    rc.check_short(corp, ad, 200, *emulated(sim, corp.x, ad, 200, cuts=corp.cuts()), what="cuts, short slab")


# ---- the sanitizers ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sanitized():
    # the one excuse is a toolchain that cannot link the sanitizers' runtimes: probed with a trivial program; anything else
    # that keeps the real one from building is a failure
    probe = subprocess.run(["make", "-s", "-C", SIM_DIR, "sanitizer_probe"], capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the toolchain here cannot link -fsanitize=address,undefined: " + probe.stderr.strip()[-300:])
    r = subprocess.run(["make", "-s", "-C", SIM_DIR, "regimes_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return os.path.join(SIM_DIR, "sim_regimes_asan")


@pytest.mark.parametrize("ad", (1, 0))
def test_sanitized_emulator_on_the_corpus(sanitized, tmp_path, ad):
    """A child process, never loaded here: exit 0 (no report from either sanitizer -- every slab is a heap block of exactly
    cap bytes per channel) and the oracle's results from all three kinds of call.  On the corpus's first 72 channels, a wave
    and a ragged one: at the emulator tests' 200 channels the sanitized program took 49 s (static) and 63 s (adaptive) per
    call here, as much as the eighteen unsanitized emulator cases together."""
    CN, corp = 72, rc.corpus(72, T)
    for cap in rc.CAPS:
        rc.check_short_is_not_vacuous(corp, cap)
    src, dst = str(tmp_path / "corpus.bin"), str(tmp_path / "result.bin")
    cuts = corp.cuts()
    with open(src, "wb") as f:
        f.write(struct.pack("<8Q", MAGIC, CN, T, ad, corp.cap, len(cuts), len(rc.CAPS), 0))
        f.write(np.array(cuts, dtype=np.uint64).tobytes())
        f.write(np.array(rc.CAPS, dtype=np.uint64).tobytes())
        f.write(np.ascontiguousarray(corp.x).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    t0 = time.time()
    r = subprocess.run([sanitized, src, dst], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (ad, r.returncode, r.stderr[-3000:])
    print("sanitized ad=%d: %.1f s" % (ad, time.time() - t0))
    with open(dst, "rb") as f:
        for call, cap in enumerate((corp.cap, corp.cap) + rc.CAPS):
            err = np.frombuffer(f.read(4 * CN), dtype=np.int32)
            bits = np.frombuffer(f.read(8 * CN), dtype=np.uint64)
            out = np.frombuffer(f.read(CN * cap), dtype=np.uint8).reshape(CN, cap)
            if call < 2:
                rc.check_full(corp, ad, out, bits, err, what=("sanitized, one launch", "sanitized, cuts")[call])
            else:
                rc.check_short(corp, ad, cap, out, bits, err, what="sanitized, short slab")
        assert f.read() == b""
