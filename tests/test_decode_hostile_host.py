"""Decoders on damaged streams, without a GPU (tests/hostile_common.py has the corpus and the checker):
  * the corpus itself: deterministic, every way a damaged stream can end is in it, the restatement's verdicts are the
    compiled reference's where that is built,
  * the decode kernel's source under the thread-per-lane emulator of tests/sim/ -- the three-wave groups, the wide pairs
    and the 64-bit containers -- held to the oracle channel by channel, once more with a slow parsing side,
  * the same emulated decoders as a stand-alone program under the address and undefined-behaviour sanitizers, every buffer
    exactly as large as the decoder is told it is."""
import ctypes as C
import os
import struct
import subprocess
import time

import numpy as np
import pytest

import hostile_common as hc
from oracle import orc

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "sim")
CN = 70  # a full wave and a ragged one
SIZES = (32, 12, 40, 64)
MAGIC = 0x454c4954534f48


@pytest.fixture(scope="module")
def sim():
    subprocess.run(["make", "-s", "-C", SIM_DIR], check=True)
    S = C.CDLL(os.path.join(SIM_DIR, "libdega_sim.so"))
    S.sim_decode_var_vs.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    S.sim_decode_wide_var.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    S.sim_decode64.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    S.sim_set_drag.argtypes = [C.c_int, C.c_int]
    return S


def emulated(S, vs, ad, wide=False):
    """decode_var of the checker: the emulator's entry point for this value size and workgroup shape"""
    def decode_var(slabs, bits, room):
        slabs, bits = np.ascontiguousarray(slabs), np.ascontiguousarray(bits)
        Cn, cap = slabs.shape
        y = np.zeros((room, Cn), dtype=np.int64 if vs > 32 else np.int32)
        counts = np.zeros(Cn, dtype=np.uint64)
        err = np.zeros(Cn, dtype=np.int32)
        if vs > 32:
            S.sim_decode64(slabs.ctypes.data, cap, bits.ctypes.data, Cn, room, Cn, ad, vs, y.ctypes.data, counts.ctypes.data, err.ctypes.data)
        elif wide:
            assert vs == 32
            S.sim_decode_wide_var(slabs.ctypes.data, cap, bits.ctypes.data, Cn, room, Cn, ad, y.ctypes.data, counts.ctypes.data, err.ctypes.data)
        else:
            S.sim_decode_var_vs(slabs.ctypes.data, cap, bits.ctypes.data, Cn, room, Cn, ad, vs, y.ctypes.data, counts.ctypes.data, err.ctypes.data)
        return y, counts, err
    return decode_var


# ---- the corpus ------------------------------------------------------------------------------------------------------------
def test_corpus_is_deterministic_and_holds_every_ending():
    a, b = hc.Corpus(CN, 33, 32, 1), hc.corpus(CN, 33, 32, 1)
    assert a.cap == b.cap and (a.bits == b.bits).all() and a.made_from == b.made_from
    assert all((a.slabs[f] == b.slabs[f]).all() for f in ("clean", "garbage"))
    for vs in SIZES:
        for ad in (1, 0):
            got, damaged = hc.check_not_vacuous(CN, vs, ad)
            print("corpus C=%d vs=%d %s: wrong samples %d, refused -3 %d, refused -11 %d, of %d damaged" % (CN, vs, "adaptive" if ad else "static", *got, damaged))
    # every kind is there, in every wave; one stream ends with its slab; an empty one is there
    corp = hc.corpus(CN, 300, 32, 1)
    assert sorted(set(corp.kind[:64].tolist())) == list(range(10)) and (corp.bits == 8 * corp.cap).sum() == 1 and (corp.bits == 0).any()
    if orc.have_ref():  # (oracle/_ref/libdcref.so is built where the reference's sources are)
        restatement_equals_the_compiled_reference()


def test_garbage_form_differs_only_beyond_the_exact_lengths_and_the_oracle_ignores_it():
    for T in (33, 300):
        corp = hc.corpus(CN, T, 32, 1)
        clean, garbage = corp.slabs["clean"], corp.slabs["garbage"]
        changed = 0
        for c in range(CN):
            n = int(corp.bits[c])
            bc, bg = np.unpackbits(clean[c]), np.unpackbits(garbage[c])
            assert (bc[:n] == bg[:n]).all()
            changed += int((bc[n:] != bg[n:]).sum())
            r, want = hc.oracle_verdict(garbage[c].tobytes(), n, 32, 1)  # (orc_bits_assign copies and masks: nothing to mask here)
            r0, want0 = corp.verdict(c)
            assert r == r0 and (r != 0 or (want == want0).all())
        assert changed > 8 * CN  # and it is garbage: bits differ in the last byte's tail and in the bytes behind it


def restatement_equals_the_compiled_reference():
    """value size 32, every kind: the reference is well defined on all of them -- it is handed a stream of an exact number
    of bits in memory and never looks beyond (dcref_run_chain)"""
    for T in (33, 300):
        for ad in (1, 0):
            corp = hc.corpus(CN, T, 32, ad)
            room = corp.room()
            for c in range(CN):
                n = int(corp.bits[c])
                r, want = corp.verdict(c)
                ret, x, _ = orc.ref_decode_i32(corp.slabs["clean"][c, : (n + 7) // 8].tobytes(), n, room, ad)
                assert ret == r, (T, ad, c, corp.made_from[c], ret, r)
                assert r != 0 or (x.view(np.uint32) == want).all(), (T, ad, c, corp.made_from[c])


# ---- the emulator ------------------------------------------------------------------------------------------------------------
def run_emulator(sim, vs, T, wide=False, drag=0):
    stats = []
    for ad in (1, 0):
        corp = hc.corpus(CN, T, vs, ad)
        if drag:
            sim.sim_set_drag(8 if wide else 4, drag)  # the parsing waves (and the loading waves behind them): the rings run full
        try:
            clean, s1 = hc.check(emulated(sim, vs, ad, wide), corp, "clean")
            garbage, s2 = hc.check(emulated(sim, vs, ad, wide), corp, "garbage")
        finally:
            sim.sim_set_drag(1 << 30, 0)
        assert hc.same_where_defined(clean, garbage), (vs, ad, T, "the result depends on what lies beyond the stream's exact length")
        stats.append((ad, s1, s2))
    print("emulator vs=%d T=%d wide=%d drag=%d: %s" % (vs, T, wide, drag, stats))


@pytest.mark.parametrize("vs", SIZES)
@pytest.mark.parametrize("T", (33, 300))
def test_emulated_decoder_on_damaged_streams(sim, vs, T):
    run_emulator(sim, vs, T)


@pytest.mark.parametrize("T", (33, 300))
def test_emulated_wide_workgroups_on_damaged_streams(sim, T):
    run_emulator(sim, 32, T, wide=True)


@pytest.mark.parametrize("vs,wide,T", ((32, False, 33), (32, False, 300), (32, True, 33), (12, False, 33), (40, False, 33), (64, False, 33)))
def test_emulated_decoder_on_damaged_streams_with_a_slow_parsing_side(sim, vs, wide, T):
    """(T = 300: the steady word path under back-pressure, cuts inside a word)"""
    run_emulator(sim, vs, T, wide=wide, drag=20)


def test_emulated_decoder_refuses_cut_streams_at_the_15th_phantom_bit(sim):
    hc.check_named_cut_streams(lambda vs, ad: emulated(sim, vs, ad))
    hc.check_named_cut_streams(lambda vs, ad: emulated(sim, vs, ad, wide=vs == 32))


def test_emulated_decoder_on_streams_that_end_in_a_stump(sim):
    hc.check_named_stumps(lambda vs, ad: emulated(sim, vs, ad), (32, 12, 40))


# ---- the sanitizers ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sanitized():
    # the one excuse is a toolchain that cannot link the sanitizers' runtimes: probed with a trivial program; anything else
    # that keeps the real one from building is a failure
    probe = subprocess.run(["make", "-s", "-C", SIM_DIR, "sanitizer_probe"], capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the toolchain here cannot link -fsanitize=address,undefined: " + probe.stderr.strip()[-300:])
    r = subprocess.run(["make", "-s", "-C", SIM_DIR, "hostile_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return os.path.join(SIM_DIR, "sim_hostile_asan")


def sanitized_child(program, tmp_path, vs, ad, shape, drag=0):
    def decode_var(slabs, bits, room):
        Cn, cap = slabs.shape
        src, dst = str(tmp_path / "corpus.bin"), str(tmp_path / "result.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("<8Q", MAGIC, Cn, cap, room, vs, ad, shape, drag))
            f.write(np.ascontiguousarray(bits, dtype=np.uint64).tobytes())
            f.write(np.ascontiguousarray(slabs).tobytes())
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([program, src, dst], capture_output=True, text=True, env=env)
        assert r.returncode == 0, (vs, ad, shape, r.returncode, r.stderr[-3000:])
        with open(dst, "rb") as f:
            err = np.frombuffer(f.read(4 * Cn), dtype=np.int32)
            counts = np.frombuffer(f.read(8 * Cn), dtype=np.uint64)
            y = np.frombuffer(f.read(), dtype=np.int64 if shape == 2 else np.int32).reshape(room, Cn)
        return y, counts, err
    return decode_var


@pytest.mark.parametrize("vs,shape", ((32, 0), (32, 1), (12, 0), (64, 2)))
def test_sanitized_emulator_on_damaged_streams(sim, sanitized, tmp_path, vs, shape):
    """A child process, never loaded here: exit 0 (no report from either sanitizer), the oracle's verdicts, and the very
    arrays the emulator gives in this process -- on the garbage form, whose slabs hold no zero the decoder could lean on."""
    for ad in (1, 0):
        corp = hc.corpus(CN, 33, vs, ad)
        t0 = time.time()
        got, stats = hc.check(sanitized_child(sanitized, tmp_path, vs, ad, shape), corp, "garbage")
        here, _ = hc.check(emulated(sim, vs, ad, wide=shape == 1), corp, "garbage")
        assert hc.same_where_defined(got, here), (vs, ad, shape)
        print("sanitized vs=%d shape=%d ad=%d: %s, %.1f s" % (vs, shape, ad, stats, time.time() - t0))
