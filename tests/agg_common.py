"""Shared by tests/test_aggregate_host.py and tests/test_gpu_aggregate.py: the numpy restatement of the reference's
`aggregate` stage and the float comparison of this feature.  (tests/golden/make_golden_aggregate.py keeps its own copy:
the generator stands alone.)"""
import numpy as np


def same_floats(got, want):
    """bit for bit; a NaN only has to be a NaN (payloads are not compared)"""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    nan = np.isnan(got) & np.isnan(want)
    return got.shape == want.shape and bool(((got.view(np.uint32) == want.view(np.uint32)) | nan).all())


def sequential(v_tc, N):
    """DCLib/src/aggregate.c:13-22 restated: a float32 accumulator from +0.0f, one rounding per add, short last group"""
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


def meter(rng, T, Cn, top=5000.0):
    """meter-like magnitudes: 0 ... top with two decimals"""
    return (np.round(rng.uniform(0.0, top, (T, Cn)) * 100.0) / 100.0).astype(np.float32)
