#!/usr/bin/env python3
"""Generates tests/golden/aggregate.npz from the COMPILED REFERENCE LIBRARY in process (oracle/_ref/libdcref.so through
orc.ref_run_chain; not the DCCLI binary, whose fast-math start-up code flushes subnormals).  Build container only:

    make -C oracle && python tests/golden/make_golden_aggregate.py

Data only.  Per case `name`:
  name.v        float32 [T][C]   the fine readings (time-major, as the library takes them)
  name.N        int64            num_values
  name.a        float32 [ceil(T/N)][C]   what `encode aggregate num_values=N` writes for every channel
and for the cases that go on into the coder, per (valuesize, adaptive) in CHAIN_CONFIGS:
  name.vs<V>.<ad|st>.stream   uint8 [C][longest]   `encode aggregate # encode normalize # encode diff # encode seg # encode bac`
  name.vs<V>.<ad|st>.bits     uint64 [C]           exact bit lengths
  name.vs<V>.<ad|st>.err      int32 [C]            the chain's return code per channel (0, or the reference's error code)
  name.factor                 float32              normalization_factor of those chains
`series.*` is the chain over the reference's own test series (input.txt.gz after `decode csv`), N = 60, one channel; its
input is not stored again.

The generator asserts, on every case, that a strict left-to-right float32 loop reproduces the reference bit for bit,
and that a pairwise sum (np.add.reduceat) differs on at least one case -- otherwise the fixture could not tell a
reassociating kernel from a correct one.
"""
import gzip
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import orc  # noqa: E402

CHAIN_CONFIGS = ((32, 1), (32, 0), (16, 1), (16, 0))


def ref_aggregate(v_tc, N):
    T, Cn = v_tc.shape
    T_out = (T + N - 1) // N
    a = np.zeros((T_out, Cn), dtype=np.float32)
    for c in range(Cn):
        col = np.ascontiguousarray(v_tc[:, c])
        ret, b, n, _ = orc.ref_run_chain(col.tobytes(), T * 32, ["encode aggregate num_values=%d" % N])
        assert ret == 0 and n == T_out * 32, (ret, n, T_out)
        a[:, c] = np.frombuffer(b, dtype=np.float32)
    return a


def ref_chain(v_tc, N, factor, vs, ad):
    T, Cn = v_tc.shape
    streams, bits, err = [], np.zeros(Cn, dtype=np.uint64), np.zeros(Cn, dtype=np.int32)
    for c in range(Cn):
        col = np.ascontiguousarray(v_tc[:, c])
        ret, b, n, _ = orc.ref_run_chain(col.tobytes(), T * 32, [
            "encode aggregate num_values=%d" % N, "encode normalize normalization_factor=%s valuesize=%d" % (repr(float(factor)), vs),
            "encode diff valuesize=%d" % vs, "encode seg valuesize=%d" % vs, "encode bac" + (" adaptive" if ad else "")])
        err[c] = ret
        bits[c] = n if ret == 0 else 0
        streams.append(b[: (n + 7) // 8] if ret == 0 else b"")
    out = np.zeros((Cn, max(1, max(len(s) for s in streams))), dtype=np.uint8)
    for c, s in enumerate(streams):
        out[c, : len(s)] = np.frombuffer(s, dtype=np.uint8)
    return out, bits, err


def sequential(v_tc, N):
    """aggregate.c:13-22 restated: float32 accumulator from +0.0f, one rounding per add, short last group"""
    T, Cn = v_tc.shape
    T_out = (T + N - 1) // N
    a = np.zeros((T_out, Cn), dtype=np.float32)
    with np.errstate(all="ignore"):
        for j in range(T_out):
            acc = np.zeros(Cn, dtype=np.float32)
            for t in range(j * N, min((j + 1) * N, T)):
                acc = acc + v_tc[t]
            a[j] = acc
    return a


def pairwise(v_tc, N):
    T = v_tc.shape[0]
    with np.errstate(all="ignore"):
        return np.add.reduceat(v_tc, np.arange(0, T, N), axis=0).astype(np.float32)


def same_floats(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    nan = np.isnan(x) & np.isnan(y)
    return x.shape == y.shape and bool(((x.view(np.uint32) == y.view(np.uint32)) | nan).all())


def meter(rng, T, Cn, top=5000.0):
    return (np.round(rng.uniform(0.0, top, (T, Cn)) * 100.0) / 100.0).astype(np.float32)


def main():
    assert orc.have_ref(), "oracle/_ref/libdcref.so is not built (make -C oracle)"
    rng = np.random.default_rng(20151)
    cases = {}
    # meter-like magnitudes: every N, T a multiple of N, T = kN +- 1, T < N
    for name, N, T, Cn in (("n1", 1, 50, 70), ("n2_plus1", 2, 101, 70), ("n3_mult", 3, 30, 72), ("n7_short", 7, 5, 70), ("n7_minus1", 7, 62, 72),
                           ("n60_mult", 60, 600, 70), ("n60_plus1", 60, 601, 8), ("n60_short", 60, 59, 8), ("n900_plus1", 900, 1801, 8),
                           ("n900_minus1", 900, 1799, 8), ("n900_mult", 900, 900, 12)):
        cases[name] = (meter(rng, T, Cn), N)
    # large alternating values: the order of the adds is visible in the result
    T = 240
    alt = meter(rng, T, 4)
    big = np.float32(16777216.0) * (1 + np.arange(T) % 5).astype(np.float32)
    alt[:, 1] = np.where(np.arange(T) % 2 == 0, big, -big) + alt[:, 1]
    alt[:, 2] = np.where(np.arange(T) % 3 == 0, np.float32(3.0e9), np.float32(-1.5e9)) + alt[:, 2]
    cases["alternating_n60"] = (alt.astype(np.float32), 60)
    cases["alternating_n7"] = (alt.astype(np.float32), 7)
    # float-only: zeros of both signs, infinities, subnormals (NaN results from inf - inf compare as NaN)
    tiny = np.float32(1e-45)
    sp = np.zeros((12, 8), dtype=np.float32)
    sp[:, 0] = -0.0
    sp[:, 1] = [0.0, -0.0] * 6
    sp[:, 2] = tiny * np.arange(1, 13, dtype=np.float32)
    sp[:, 3] = [np.float32(1.1754942e-38), -np.float32(1.1754942e-38) + tiny] * 6  # sums that stay subnormal
    sp[:, 4] = [np.inf, 1.0, 2.0, -np.inf, 5.0, np.inf, 1.0, 1.0, 1.0, 1.0, 1.0, -0.0]
    sp[:, 5] = [-np.inf] + [3.5] * 11
    sp[:, 6] = [np.float32(3.0e38), np.float32(3.0e38), -np.float32(3.0e38)] * 4  # overflow to inf inside a group
    sp[:, 7] = [-0.0, tiny, -tiny, 0.0, -0.0, -0.0, 1.0, -1.0, -0.0, 0.0, tiny, tiny]
    for N in (1, 2, 3, 7):
        cases["special_n%d" % N] = (sp.copy(), N)

    out = {}
    differs = 0
    for name, (v, N) in cases.items():
        a = ref_aggregate(v, N)
        assert same_floats(sequential(v, N), a), "a strict sequential float32 sum does not reproduce the reference on " + name
        differs += 0 if same_floats(pairwise(v, N), a) else 1
        out[name + ".v"], out[name + ".N"], out[name + ".a"] = v, np.int64(N), a
    assert differs > 0, "no case tells a pairwise sum from the sequential one"

    # cases that go on into the coder (no NaN / inf here); chain_small has one channel whose sums leave 16 bits at factor 100
    small = meter(rng, 601, 6, top=5.0)
    small[:, 3] = meter(rng, 601, 1, top=50.0)[:, 0]
    chains = {"chain_meter": (cases["n60_plus1"][0], 60, 1.0), "chain_small": (small, 60, 100.0), "chain_n7": (meter(rng, 62, 70, top=40.0), 7, 100.0)}
    for name, (v, N, factor) in chains.items():
        a = ref_aggregate(v, N)
        assert same_floats(sequential(v, N), a), name
        out[name + ".v"], out[name + ".N"], out[name + ".a"], out[name + ".factor"] = v, np.int64(N), a, np.float32(factor)
        for vs, ad in CHAIN_CONFIGS:
            s, b, e = ref_chain(v, N, factor, vs, ad)
            key = "%s.vs%d.%s." % (name, vs, "ad" if ad else "st")
            out[key + "stream"], out[key + "bits"], out[key + "err"] = s, b, e
    e16 = out["chain_small.vs16.ad.err"]
    assert e16[3] == orc.ERROR_INVALID_VALUE and (np.delete(e16, 3) == 0).all(), e16
    assert (out["chain_small.vs32.ad.err"] == 0).all()

    # the reference's own float test series, N = 60, one channel
    with gzip.open(os.path.join(HERE, "input.txt.gz"), "rb") as f:
        series = np.array(f.read().split(), dtype=np.float64).astype(np.float32)
    v = series.reshape(-1, 1)
    out["series.N"], out["series.a"] = np.int64(60), ref_aggregate(v, 60)
    assert same_floats(sequential(v, 60), out["series.a"])
    s, b, e = ref_chain(v, 60, 100.0, 32, 1)
    assert e[0] == 0
    out["series.vs32.ad.stream"], out["series.vs32.ad.bits"] = s, b

    path = os.path.join(HERE, "aggregate.npz")
    np.savez_compressed(path, **out)
    print("%s: %d arrays, %d bytes; pairwise differs from the reference on %d of %d float cases" % (path, len(out), os.path.getsize(path), differs, len(cases)))


if __name__ == "__main__":
    main()
