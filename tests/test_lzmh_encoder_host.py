"""The LZMH encoder on steered texts, without a GPU (tests/lzmh_encoder_common.py has the corpus, its conditions and the
checkers):
  * the corpus itself: deterministic, a smaller batch the head of a larger one, the three forms alike up to the lengths, the
    replay's stream the oracle's on every channel, every condition of every batch, the tokenizer against the assembler;
  * the encode kernel's source under the thread-per-lane emulator of tests/sim/: the three forms at the full slab, the end
    of the slab, and both again with the coding waves dragged, so that the token ring runs full (the searcher waits) and a
    coder that gives a channel up does so with tokens in flight (`stop`);
  * the same calls as a stand-alone program under the address and undefined-behaviour sanitizers.
C = 70: a wave and a ragged one."""
import ctypes as C
import os
import struct
import subprocess
import time

import numpy as np
import pytest

import lzmh_encoder_common as ec
from oracle import orc

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "sim")
CN = 70
MAGIC = 0x434e45484d5a4c
DRAG_US = 20


@pytest.fixture(scope="module")
def sim():
    subprocess.run(["make", "-s", "-C", SIM_DIR], check=True)
    S = C.CDLL(os.path.join(SIM_DIR, "libdega_sim.so"))
    S.sim_lzmh_encode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    S.sim_set_drag.argtypes = [C.c_int, C.c_int]
    return S


def emulated_rows(S, drag=0):
    """encode_rows of the checkers: the emulator's entry point, into slabs the caller brings; drag: microseconds the coding
    waves (4 .. 7 of the workgroup) sleep per pass"""
    def encode_rows(rows, lens, cap, out):
        rows, lens = np.ascontiguousarray(rows), np.ascontiguousarray(lens, dtype=np.uint64)
        Cn, stride = rows.shape
        assert rows.ctypes.data % 16 == 0 and out.ctypes.data % 16 == 0 and out.shape[1] == cap and out.shape[0] >= Cn
        bits = np.zeros(Cn, dtype=np.uint64)
        err = np.zeros(Cn, dtype=np.int32)
        S.sim_set_drag(4 if drag else 1 << 30, drag)
        try:
            S.sim_lzmh_encode(rows.ctypes.data, stride, lens.ctypes.data, Cn, out.ctypes.data, cap, bits.ctypes.data, err.ctypes.data)
        finally:
            S.sim_set_drag(1 << 30, 0)
        return bits, err
    return encode_rows


def emulated(S, drag=0):
    def encode(rows, lens, cap):
        out = np.zeros((rows.shape[0], cap), dtype=np.uint8)
        return (out,) + emulated_rows(S, drag)(rows, lens, cap, out)
    return encode


# ---- the corpus ------------------------------------------------------------------------------------------------------------
def test_corpus_is_deterministic_and_a_smaller_batch_is_the_head_of_a_larger_one():
    corp = ec.corpus(CN, 600)
    again, head = ec.Corpus(CN, 600), ec.Corpus(20, 600)
    assert again.text == corp.text and (again.lens == corp.lens).all()
    assert head.text == corp.text[:20] and (head.lens == corp.lens[:20]).all() and (head.rows["continued"] == corp.rows["continued"][:20]).all()
    assert all((again.rows[form] == corp.rows[form]).all() for form in ec.FORMS)
    assert sorted(set(corp.kind[:64].tolist())) == list(range(8))
    lens = set(corp.lens.tolist())
    assert set(ec.SPECIAL) <= lens and corp.stride in lens and int(corp.lens[CN - 1]) == corp.stride
    assert ec.corpus(CN, 40).stride == 48 and int(ec.corpus(CN, 40).lens.max()) == 48


@pytest.mark.parametrize("n", (40, 600))
def test_the_forms_differ_only_behind_the_lengths(n):
    corp = ec.corpus(CN, n)
    behind = np.arange(corp.stride)[None, :] >= corp.lens[:, None].astype(np.int64)
    for form in ec.FORMS:
        assert (corp.rows[form][~behind] == corp.rows["continued"][~behind]).all()
    assert not corp.rows["clean"][behind].any()
    # ... and behind them they do differ: the continued form goes on as the text does, the garbage form does not
    short = [c for c in range(CN) if int(corp.lens[c]) + 16 <= corp.stride]
    assert len(short) >= CN // 3
    differ = sum((corp.rows["garbage"][c] != corp.rows["continued"][c]).any() for c in short)
    assert differ == len(short)
    assert sum(corp.rows["continued"][c, int(corp.lens[c]):].any() for c in short) >= len(short) - CN // 8  # (all but the zero runs)


@pytest.mark.parametrize("Cn,n", sorted(ec.ORACLE_COUNTS))
def test_the_conditions_hold(Cn, n):
    t0 = time.time()
    got = ec.check_not_vacuous(Cn, n)  # (the replay's stream is the oracle's on every channel: Corpus.trace asserts it)
    print("C=%d n=%d, %.2f s: %s" % (Cn, n, time.time() - t0, ", ".join("%s %d" % (name, v) for name, v in zip(ec.EVENTS, got.tolist()))))
    if n == ec.SLAB_N:
        print("slab end (fit, either, err) per cap:", ec.check_slab_is_not_vacuous(ec.corpus(Cn, n)))


def test_the_ladder_does_what_it_says():
    """at the last X of a block the best length rises at least 8 times, and the longest prefix is beyond 16 bytes in some block"""
    corp = ec.corpus(CN, 600)
    for c in corp.of_kind(1):
        if int(corp.lens[c]) >= 300:
            t = corp.trace(c)
            assert int(t.improved.max()) >= 8 and int(t.cand[t.improved >= 7].max()) >= 8, c
    assert max(int(corp.trace(c).length[corp.trace(c).improved >= 7].max(initial=0)) for c in corp.of_kind(1)) > 16


@pytest.mark.parametrize("n", (40, 600))
def test_tokenizer_round_trips(n):
    """the oracle's stream taken apart code by code is the replay's steps, and put together again by the assembler of
    lzmh_hostile_common it is the oracle's stream"""
    corp = ec.corpus(CN, n)
    for c in range(CN):
        tokens = corp.tokens(c)
        assert tokens == corp.trace(c).tokens(), (c, ec.KINDS[c % 8])
        assert ec.assemble(tokens) == corp.want[c], (c, ec.KINDS[c % 8])
        # what the codes stand for is the text: literals and copies, replayed
        text = bytearray()
        for step, t in enumerate(tokens):
            if t[0] in ("raw", "lst"):
                text.append(int(corp.trace(c).sym[step]))
            else:
                for _ in range(t[2]):
                    text.append(text[-(t[1] if t[0] == "match" else t[3])])
        assert bytes(text) == (corp.seen(c) if len(corp.seen(c)) != 403 else b""), c


def test_restatement_equals_the_compiled_reference_on_the_corpus():
    if not orc.have_ref():
        pytest.skip("oracle/_ref/libdcref.so is built where the reference's sources are; elsewhere the golden vectors stand for it")
    corp = ec.corpus(CN, 600)
    for c in range(CN):
        text = corp.seen(c)
        ret, stream, nbits, _ = orc.ref_run_chain(text, 8 * len(text), ["encode lzmh"])
        assert ret == 0 and (stream, nbits) == corp.want[c], (c, ec.KINDS[c % 8])


# ---- the emulator ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drag", (0, DRAG_US))
@pytest.mark.parametrize("n", (40, 600))
def test_emulated_encoder_on_all_forms(sim, n, drag):
    ec.check_not_vacuous(CN, n)
    t0 = time.time()
    ec.check_all_forms(emulated(sim, drag), ec.corpus(CN, n))
    print("emulator n=%d drag=%d: %.1f s" % (n, drag, time.time() - t0))


@pytest.mark.parametrize("drag", (0, DRAG_US))
def test_emulated_encoder_at_the_end_of_the_slab(sim, drag):
    """dragged: the coder that errs leaves its searcher with a full ring and tokens in flight"""
    t0 = time.time()
    ec.check_slab_end(emulated_rows(sim, drag), CN)
    print("emulator, slab end, drag=%d: %.1f s" % (drag, time.time() - t0))


def test_emulated_encoder_never_overflows_the_worst_case_at_its_tightest(sim):
    rows, lens, cap, (want, nb) = ec.tightest_fit()
    out = np.full((2, cap), ec.CANARY, dtype=np.uint8)
    bits, err = emulated_rows(sim)(rows, lens, cap, out)
    assert err[0] == 0 and int(bits[0]) == nb and out[0, : len(want)].tobytes() == want
    assert (out[0, len(want):] == ec.CANARY).all() and (out[1] == ec.CANARY).all()


# ---- the sanitizers ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sanitized():
    # the one excuse is a toolchain that cannot link the sanitizers' runtimes: probed with a trivial program; anything else
    # that keeps the real one from building is a failure
    probe = subprocess.run(["make", "-s", "-C", SIM_DIR, "sanitizer_probe"], capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the toolchain here cannot link -fsanitize=address,undefined: " + probe.stderr.strip()[-300:])
    r = subprocess.run(["make", "-s", "-C", SIM_DIR, "lzmh_encoder_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return os.path.join(SIM_DIR, "sim_lzmh_encoder_asan")


@pytest.mark.parametrize("drag", (0, DRAG_US))
def test_sanitized_emulator_on_the_corpus(sim, sanitized, tmp_path, drag):
    """A child process, never loaded here: exit 0 (no report from either sanitizer -- the rows are one heap block of exactly
    C * stride bytes, the full-stride channel last, every slab array one of exactly C * cap) and, on the garbage and the
    continued form and at the end of the slab, the oracle's results and the very arrays the emulator gives in this process."""
    corp = ec.corpus(CN, ec.SLAB_N)
    assert int(corp.lens[CN - 1]) == corp.stride
    forms, full = ("garbage", "continued"), ec.worst_case_bytes(corp.stride)
    src, dst = str(tmp_path / "corpus.bin"), str(tmp_path / "result.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<8Q", MAGIC, CN, corp.stride, len(forms), full, len(ec.CAPS), drag, 0))
        f.write(np.array(ec.CAPS, dtype=np.uint64).tobytes())
        f.write(corp.lens.tobytes())
        for form in forms:
            f.write(np.ascontiguousarray(corp.rows[form]).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    t0 = time.time()
    r = subprocess.run([sanitized, src, dst], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (drag, r.returncode, r.stderr[-3000:])
    print("sanitized drag=%d: %.1f s" % (drag, time.time() - t0))
    blocks = []
    with open(dst, "rb") as f:
        for cap in (full,) * len(forms) + ec.CAPS:
            err = np.frombuffer(f.read(4 * CN), dtype=np.int32)
            bits = np.frombuffer(f.read(8 * CN), dtype=np.uint64)
            blocks.append((np.frombuffer(f.read(CN * cap), dtype=np.uint8).reshape(CN, cap), bits, err))
        assert f.read() == b""
    calls = iter(blocks)
    for form in forms:
        ec.check(lambda rows, lens, cap: next(calls), corp, form, full)

    def from_the_child(rows, lens, cap, out):
        child_out, bits, err = next(calls)
        out[:CN] = child_out
        return bits, err

    ec.check_slab_end(from_the_child, CN, form=forms[-1])
    # ... and the emulator in this process gives the same arrays, byte for byte (a channel that errs included: whatever it
    # wrote before it gave up, it wrote the same).  Undragged: what a dragged coder that errs leaves behind depends on no timing
    # either -- it stops at the same store --, so the child's dragged arrays are compared with these too.
    for k, cap in enumerate((full,) * len(forms) + ec.CAPS):
        out = np.full((CN, cap), ec.CANARY, dtype=np.uint8)
        bits, err = emulated_rows(sim)(corp.rows[forms[min(k, len(forms) - 1)]], corp.lens, cap, out)
        assert (bits == blocks[k][1]).all() and (err == blocks[k][2]).all() and (out == blocks[k][0]).all(), (drag, k, cap)
