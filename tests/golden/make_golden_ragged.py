#!/usr/bin/env python3
"""Generates tests/golden/ragged.npz from the COMPILED REFERENCE LIBRARY in process (oracle/_ref/libdcref.so through
orc.ref_run_chain).  Build container only:

    make -C oracle && python tests/golden/make_golden_ragged.py

Ragged batches: a float32 matrix [T][C] and a count per channel, as `decode csv` delivers meter files of different
lengths.  Channel c IS its first count[c] readings; per channel every stored result is what the reference's chain gives
on exactly those floats.  Data only.  Per case (`long`: T = 200, C = 136 -- two full waves and eight lanes, a multiple of
4; `short`: T = 96, C = 70 -- one full wave and six lanes, the dword form only) and level N = 1, 7, 60:
  <case>.v                      float32 [T][C]   the readings (agg_common.meter, at most 5.00 so that the level-60 sums still
                                                 fit 16 bits at factor 100; the full wave of `long` at most 0.30, which
                                                 keeps its streams and the fixture small); every row at or beyond a channel's count holds
                                                 POISON, cycling NaN, +inf, 3e38, -0.0: a kernel that lets one of them into a
                                                 sum, a stream, a text or a status fails
  <case>.count                  int64 [C]
  <case>.N<N>.sums / .rows      float32 [ceil(T / N)][C] (zeros beyond a channel's rows) / int64 [C] = ceil(count / N):
                                                 `encode aggregate num_values=N`
  <case>.N<N>.text / .text_len  uint8 [C][longest] / int64 [C]: `encode aggregate num_values=N # encode csv num_decimal_places=2`
  <case>.N<N>.lzmh / .lzmh_bits uint8 [C][longest] / uint64 [C]: the same `# encode lzmh`
  <case>.N<N>.vs<V>.<ad|st>.stream / .bits / .err   `encode aggregate num_values=N # encode normalize normalization_factor=100
                                                 valuesize=V # encode diff # encode seg # encode bac [adaptive]` for
                                                 (32, ad), (32, st), (16, ad), (64, ad); err is the chain's return code
One honest error: channel HONEST of each case has a reading of 400.0 INSIDE its count, which leaves 16 bits at factor 100;
its ERROR_INVALID_VALUE is the only one of the (16, ad) sets, at every level.

The generator asserts that the fixture is not blind: the numpy restatement on the prefix reproduces the reference; a
restatement that ignores the counts differs on every ragged channel; one that pads the short channels with zeros differs
in a sum or a stream on at least one channel per level.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from agg_common import meter, same_floats, sequential  # noqa: E402
from oracle import orc  # noqa: E402

LEVELS = (1, 7, 60)
SETS = ((32, 1), (32, 0), (16, 1), (64, 1))
FACTOR = 100.0
HONEST = 5
POISON = np.array([np.nan, np.inf, 3e38, -0.0], dtype=np.float32)


def chain(col, stages):
    col = np.ascontiguousarray(col, dtype=np.float32)
    ret, b, n, _ = orc.ref_run_chain(col.tobytes(), 32 * col.size, stages)
    return ret, (b[: (n + 7) // 8] if ret == 0 else b""), (n if ret == 0 else 0)


def dega_stages(N, vs, ad):
    return ["encode aggregate num_values=%d" % N, "encode normalize normalization_factor=%s valuesize=%d" % (repr(FACTOR), vs),
            "encode diff valuesize=%d" % vs, "encode seg valuesize=%d" % vs, "encode bac" + (" adaptive" if ad else "")]


def rows_of(items):
    out = np.zeros((len(items), max(1, max(len(s) for s in items))), dtype=np.uint8)
    for c, s in enumerate(items):
        out[c, : len(s)] = np.frombuffer(s, dtype=np.uint8)
    return out


def make_case(rng, T, Cn, count):
    v = meter(rng, T, Cn, top=5.0)
    if Cn > 128:
        v[:, 64:128] = meter(rng, T, 64, top=0.3)  # (the full wave: small readings, short streams -- the fixture stays below the largest one)
    assert count[HONEST] > 10
    v[10, HONEST] = 400.0
    for c in range(Cn):
        for t in range(int(count[c]), T):
            v[t, c] = POISON[(t - int(count[c])) % 4]  # (the first dead row is a NaN, the second an infinity)
    return v


def add_case(out, name, v, count):
    T, Cn = v.shape
    out[name + ".v"], out[name + ".count"] = v, count.astype(np.int64)
    ragged = [c for c in range(Cn) if count[c] < T]
    zeroed = v.copy()
    for c in range(Cn):
        zeroed[int(count[c]):, c] = 0.0
    for N in LEVELS:
        key = "%s.N%d" % (name, N)
        rows = -(-count // N)
        sums = np.zeros((-(-T // N), Cn), dtype=np.float32)
        texts, lz, lz_bits = [], [], np.zeros(Cn, dtype=np.uint64)
        agg = ["encode aggregate num_values=%d" % N]
        for c in range(Cn):
            own = v[: int(count[c]), c]
            ret, b, n = chain(own, agg)
            assert ret == 0 and n == 32 * int(rows[c]), (name, N, c, ret, n)
            sums[: int(rows[c]), c] = np.frombuffer(b, dtype=np.float32)
            # the restatement on the prefix is the reference
            assert same_floats(sequential(own.reshape(-1, 1), N)[:, 0], sums[: int(rows[c]), c]), (name, N, c)
            ret, t, n = chain(own, agg + ["encode csv num_decimal_places=2"])
            assert ret == 0 and n % 8 == 0 and t.count(b"\n") == int(rows[c])
            texts.append(t)
            ret, s, n = chain(own, agg + ["encode csv num_decimal_places=2", "encode lzmh"])
            assert ret == 0
            lz.append(s)
            lz_bits[c] = n
            if count[c] == 0:
                assert t == b"" and n == 0  # `aggregate` writes nothing, `encode csv # encode lzmh` gives 0 bits
        out[key + ".sums"], out[key + ".rows"] = sums, rows.astype(np.int64)
        out[key + ".text"], out[key + ".text_len"] = rows_of(texts), np.array([len(t) for t in texts], dtype=np.int64)
        out[key + ".lzmh"], out[key + ".lzmh_bits"] = rows_of(lz), lz_bits
        for vs, ad in SETS:
            streams, bits, err = [], np.zeros(Cn, dtype=np.uint64), np.zeros(Cn, dtype=np.int32)
            for c in range(Cn):
                ret, s, n = chain(v[: int(count[c]), c], dega_stages(N, vs, ad))
                err[c], bits[c] = ret, n
                streams.append(s)
                if count[c] == 0 and ad:
                    assert ret == 0 and n == 3 and s == b"\x20", (name, N, vs, s, n)  # the reference on an empty input
            k = "%s.vs%d.%s" % (key, vs, "ad" if ad else "st")
            out[k + ".stream"], out[k + ".bits"], out[k + ".err"] = rows_of(streams), bits, err
            if (vs, ad) == (16, 1):
                assert [c for c in range(Cn) if err[c] != 0] == [HONEST] and err[HONEST] == orc.ERROR_INVALID_VALUE, (name, N, err.nonzero())
            else:
                assert (err == 0).all(), (name, N, vs, ad)
        # a restatement that pads the short channels with zeros: more rows, another stream
        differs = 0
        for c in ragged:
            ret, s, n = chain(zeroed[:, c], dega_stages(N, 32, 1))
            stored = out[key + ".vs32.ad.stream"][c, : (int(out[key + ".vs32.ad.bits"][c]) + 7) // 8].tobytes()
            differs += not (same_floats(sequential(zeroed[:, c : c + 1], N)[:, 0], sums[:, c]) and int(rows[c]) == sums.shape[0] and s == stored)
        assert differs >= 1, (name, N)
    # a restatement that ignores the counts (all T rows, poison included) is told apart on every ragged channel: at level 1
    # the row count differs, and so do the floats
    whole1 = sequential(v, 1)
    for c in ragged:
        assert int(out[name + ".N1.rows"][c]) != T and not same_floats(whole1[:, c], out[name + ".N1.sums"][:, c]), (name, c)
    return len(ragged)


def main():
    assert orc.have_ref(), "oracle/_ref/libdcref.so is not built (make -C oracle)"
    rng = np.random.default_rng(20154)
    out = {}
    # long: wave 0 mixed, wave 1 all T (the steady path must still be taken), the last eight lanes end long before T
    T = 200
    first = [0, 1, 6, 7, 8, 59, 60, 61, 63, 64, 65, 127, 199, 200]
    wave0 = np.array(first + [int(n) for n in rng.integers(0, T + 1, 64 - len(first))])
    wave0[HONEST], wave0[0] = 59, 0
    count_long = np.concatenate([wave0, np.full(64, T), np.array([50, 0, 13, 49, 7, 1, 33, 50])]).astype(np.int64)
    assert count_long.size == 136 and count_long[128:].max() <= 50
    n_long = add_case(out, "long", make_case(rng, T, 136, count_long), count_long)
    # short: one ragged wave and a ragged rest, dword form (70 is no multiple of 4)
    T = 96
    count_short = np.array([int(n) for n in rng.integers(0, T + 1, 70)]).astype(np.int64)
    count_short[[0, 1, 2, HONEST, 63, 64, 69]] = [96, 0, 1, 61, 95, 9, 96]
    n_short = add_case(out, "short", make_case(rng, T, 70, count_short), count_short)
    path = os.path.join(HERE, "ragged.npz")
    np.savez_compressed(path, **out)
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f != "ragged.npz")
    print("%s: %d arrays, %d bytes (largest other fixture %d); ragged channels: long %d of 136, short %d of 70"
          % (path, len(out), os.path.getsize(path), largest, n_long, n_short))
    assert os.path.getsize(path) <= largest


if __name__ == "__main__":
    main()
