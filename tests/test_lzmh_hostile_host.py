"""The LZMH decoder on damaged and hand-assembled streams, without a GPU (tests/lzmh_hostile_common.py has the streams and
the checker):
  * the corpus itself: deterministic, every kind in every wave, the garbage form differs only beyond the exact lengths, the
    damage does damage, the restatement is the compiled reference where that is built and defines the answer,
  * lzmh_reading_wave / lzmh_writing_wave under the thread-per-lane emulator of tests/sim/, held to the oracle channel by
    channel on the corpus and on every assembler set, once more with a slow writing wave,
  * the same as a stand-alone program under the address and undefined-behaviour sanitizers, every buffer exactly as large
    as the decoder is told it is."""
import ctypes as C
import os
import struct
import subprocess
import time

import numpy as np
import pytest

import csv_read_common as crc
import lzmh_hostile_common as lc
from oracle import orc
from test_csv_read_host import sim as csv_sim, sim_read  # noqa: F401  (the emulated `decode csv` and its fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "sim")
CN = 70  # a full wave and a ragged one
MAGIC = 0x454c4954534f48
GRID_THIN = 25   # the emulator's share of the copy grid: 480 of the 12 000 cells, every pair (o, L) with one p
CHILD_PS = tuple(range(250, 258))
CHILD_THIN = 8   # the sanitized child's: p = 250 .. 257, every pair (o, L) with one of them


@pytest.fixture(scope="module")
def sim():
    subprocess.run(["make", "-s", "-C", SIM_DIR], check=True)
    S = C.CDLL(os.path.join(SIM_DIR, "libdega_sim.so"))
    S.sim_lzmh_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    S.sim_set_drag.argtypes = [C.c_int, C.c_int]
    return S


def emulated(S, drag=0, rows=None):
    """decode of the checker: the emulator's entry point; drag: microseconds the writing waves (4 .. 7 of the workgroup) sleep
    whenever they look at their partner's word, so that the token ring runs full and the reading wave waits; rows: the
    output array, if the caller brings one"""
    def decode(slabs, bits, stride):
        slabs, bits = np.ascontiguousarray(slabs), np.ascontiguousarray(bits)
        Cn, cap = slabs.shape
        out = np.zeros((Cn, stride), dtype=np.uint8) if rows is None else rows
        lens = np.zeros(Cn, dtype=np.uint64)
        err = np.zeros(Cn, dtype=np.int32)
        S.sim_set_drag(4 if drag else 1 << 30, drag)
        try:
            S.sim_lzmh_decode(slabs.ctypes.data, cap, bits.ctypes.data, Cn, out.ctypes.data, stride, lens.ctypes.data, err.ctypes.data)
        finally:
            S.sim_set_drag(1 << 30, 0)
        return out, lens, err
    return decode


# ---- the corpus ------------------------------------------------------------------------------------------------------------
def test_corpus_is_deterministic_and_every_kind_sits_in_every_wave():
    a, b = lc.Corpus(CN, 600), lc.corpus(CN, 600)
    assert a.cap == b.cap and (a.bits == b.bits).all() and a.name == b.name and a.text == b.text
    assert all((a.slabs[f] == b.slabs[f]).all() for f in ("clean", "garbage"))
    for Cn, n in sorted(lc.ORACLE_COUNTS):
        corp = lc.corpus(Cn, n)
        for w in range(0, Cn - 9, 64):
            assert sorted(set(corp.kind[w: w + 64].tolist())) == list(range(10))
        assert sorted(set(corp.sort.tolist())) == list(range(5))
        # one stream ends with its slab, an empty one is there
        assert (corp.bits == 8 * corp.cap).sum() == 1 and (corp.bits == 0).any() and corp.cap % 4 == 0


@pytest.mark.parametrize("Cn,n", sorted(lc.ORACLE_COUNTS))
def test_corpus_damage_does_damage(Cn, n):
    got, damaged = lc.check_not_vacuous(Cn, n)
    print("corpus C=%d n=%d: differ %d, longer %d, shorter %d, of %d damaged; longest output %d" % (Cn, n, *got, damaged, max(len(w) for w in lc.corpus(Cn, n).want)))


def test_garbage_form_differs_only_beyond_the_exact_lengths_and_the_oracle_ignores_it():
    for s in (lc.corpus(CN, 40), lc.corpus(CN, 600), lc.every_cut(), lc.named(), lc.token_soup()):
        clean, garbage = s.slabs["clean"], s.slabs["garbage"]
        changed = 0
        for c in range(s.C):
            n = int(s.bits[c])
            bc, bg = np.unpackbits(clean[c]), np.unpackbits(garbage[c])
            assert (bc[:n] == bg[:n]).all()
            changed += int((bc[n:] != bg[n:]).sum())
            assert lc.oracle_decode(garbage[c].tobytes(), n) == s.want[c]
        assert changed > 8 * s.C


def test_assembler_sets_hold_what_they_promise():
    g = lc.copy_grid()
    assert g.C == 12000 and all(len(g.want[c]) == p + L + 9 for c, (o, L, p) in enumerate(g.cells))
    for thin, ps in ((GRID_THIN, lc.GRID_P), (CHILD_THIN, CHILD_PS)):
        cells = lc.grid_cells(thin, ps)
        assert {o for o, _, _ in cells} == set(lc.GRID_O) and {L for _, L, _ in cells} == set(lc.GRID_L) and {p for _, _, p in cells} == set(ps)
        assert len({(o, L) for o, L, _ in cells}) == len(lc.GRID_O) * len(lc.GRID_L)
    soup = lc.token_soup()
    assert soup.C == 520 and max(len(w) for w in soup.want) > 1000
    cuts, whole = lc.every_cut(), lc.cut_stream()
    assert 90 <= whole.n <= 110 and cuts.bits.tolist() == list(range(whole.n + 1))
    named = lc.named()
    assert named.want[0] == bytes(6) + b"\x41" and named.want[named.name.index("an empty stream")] == b"\0"
    # the 19 list codes one bit short end their channels silently: nothing is decoded from the stump
    assert all(named.want[c] == b"\x41\x42\x42" for c in range(named.C) if "one bit short" in named.name[c])


def test_restatement_equals_the_compiled_reference_where_it_defines_the_answer():
    """(oracle/_ref/libdcref.so is built where the reference's sources are; elsewhere there is nothing to compare)"""
    if not orc.have_ref():
        return
    for n in (40, 600, 3000):
        corp = lc.corpus(130, n)
        lc.check_reference(corp, [c for c in range(corp.C) if corp.kind[c] == 0])
    g = lc.copy_grid()
    lc.check_reference(g, [c for c, (o, L, p) in enumerate(g.cells) if o <= p])


# ---- the emulator ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (40, 600))
def test_emulated_decoder_on_the_damaged_corpus(sim, n):
    t0 = time.time()
    lc.check_both(emulated(sim), lc.corpus(CN, n))
    print("emulator corpus n=%d: %.1f s" % (n, time.time() - t0))


@pytest.mark.parametrize("which", ("named", "every_cut", "token_soup", "copy_grid"))
def test_emulated_decoder_on_the_assembler_sets(sim, which):
    streams = lc.copy_grid(GRID_THIN) if which == "copy_grid" else getattr(lc, which)()
    t0 = time.time()
    lc.check_both(emulated(sim), streams)
    print("emulator %s: %d channels, %.1f s" % (which, streams.C, time.time() - t0))


def test_emulated_decoder_with_a_slow_writing_wave(sim):
    """the token ring runs full: the reading wave finds no room and waits; a channel whose reader finished early is drained"""
    t0 = time.time()
    for streams in (lc.corpus(CN, 40), lc.named(), lc.every_cut()):
        lc.check(emulated(sim, drag=20), streams, "garbage")
    print("emulator, slow writing wave: %.1f s" % (time.time() - t0))


def rows_decoder(S, drag=0):
    """decode_rows of lzmh_hostile_common.check_boundary: the emulator writes into the rows it is given"""
    def decode_rows(slabs, bits, stride, rows):
        out, lens, err = emulated(S, drag, rows)(slabs, bits, stride)
        return lens, err
    return decode_rows


def test_emulated_decoder_at_the_end_of_the_row(sim):
    """a channel that does not fit its row reports ERROR_MEMORY and touches no other row (lzmh_hostile_common.check_boundary;
    tests/test_gpu_lzmh_hostile.py has the same on the device)"""
    lc.check_boundary(rows_decoder(sim))


def test_emulated_decoder_at_the_end_of_the_row_with_a_slow_writing_wave(sim):
    """the reading wave's `stop`: the writer gives a channel up while its ring is full of tokens it will not take"""
    lc.check_boundary(rows_decoder(sim, drag=20))

# ---- the csv reader behind the decoder ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", (40, 600))
def test_emulated_csv_reader_on_the_texts_damaged_streams_decode_to(csv_sim, n):
    """the second half of dega_hip_lzmh_decode_f32_dev, without a GPU: the texts the oracle decodes the meter-line and digit
    channels to -- NUL bytes, fields cut anywhere, runs of one byte -- through the csv reader, against libc's strtof"""
    corp = lc.corpus(130, n)
    texts = [corp.want[c] for c in range(corp.C) if corp.sort[c] in (0, 1)]
    max_T = max(len(t) for t in texts)
    v, count, err = sim_read(csv_sim, texts, max_T)
    want, status = zip(*[crc.expected(t) for t in texts])
    values = crc.check_channels(v, count, err, want, status, max_T, ("emulated csv reader", n))
    assert values > 0 and any(b"\0" in t for t in texts)


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


def sanitized_child(program, tmp_path):
    def decode(slabs, bits, stride):
        Cn, cap = slabs.shape
        src, dst = str(tmp_path / "streams.bin"), str(tmp_path / "result.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("<8Q", MAGIC, Cn, cap, stride, 0, 0, 3, 0))
            f.write(np.ascontiguousarray(bits, dtype=np.uint64).tobytes())
            f.write(np.ascontiguousarray(slabs).tobytes())
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([program, src, dst], capture_output=True, text=True, env=env)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        with open(dst, "rb") as f:
            err = np.frombuffer(f.read(4 * Cn), dtype=np.int32)
            lens = np.frombuffer(f.read(8 * Cn), dtype=np.uint64)
            out = np.frombuffer(f.read(), dtype=np.uint8).reshape(Cn, stride)
        return out, lens, err
    return decode


@pytest.mark.parametrize("which", ("corpus 40", "corpus 600", "named", "copy_grid"))
def test_sanitized_emulator_on_lzmh_streams(sim, sanitized, tmp_path, which):
    """A child process, never loaded here: exit 0 (no report from either sanitizer), the oracle's answers, and the very arrays
    the emulator gives in this process -- on the garbage form, whose slabs hold no zero the decoder could lean on.  The
    grid at p = 250 .. 257: the matches that cross the seam of the writer's 256-byte ring."""
    streams = (lc.copy_grid(CHILD_THIN, CHILD_PS) if which == "copy_grid" else lc.named() if which == "named" else lc.corpus(CN, int(which.split()[1])))
    t0 = time.time()
    got = lc.check(sanitized_child(sanitized, tmp_path), streams, "garbage")
    here = lc.check(emulated(sim), streams, "garbage")
    assert all((x == y).all() for x, y in zip(got, here)), which
    print("sanitized %s: %d channels, %.1f s" % (which, streams.C, time.time() - t0))
