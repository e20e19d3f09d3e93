"""Several granularities of the `aggregate` stage from one pass over the base series, without a GPU: the new symbols of
the C ABI, the planner that decides which levels share a pass (dega_hip_aggregate_levels_plan is pure), and the kernel's
LOGIC -- the shipped kernel source compiled by g++ under the thread-per-lane emulator of tests/sim/ against
tests/golden/aggregate_levels.npz (the compiled reference's floats, one run per level).  The parity tests proper are
tests/test_gpu_aggregate_levels.py."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

from __graft_entry__ import load_package

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from agg_common import same_floats, sequential  # noqa: E402
from agg_levels_common import Fixture  # noqa: E402
from sim_build import sim_library  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("dega_hip_aggregate_levels_plan", "dega_hip_aggregate_levels_dev", "dega_hip_encode_levels_f32_dev", "dega_hip_encode_levels_job_host",
               "dega_hip_group_encode_levels")
SENTINEL = np.float32(-12345.0)


@pytest.fixture(scope="module")
def dca():
    mod = load_package()
    if not os.path.exists(mod.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return mod


@pytest.fixture(scope="module")
def fx():
    return Fixture()


# ---- C ABI ---------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_declared_and_exported(dca):
    with open(os.path.join(ROOT, "include", "dega_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(dega_hip_[a-z0-9_]+)\s*\(", header))
    lib = C.CDLL(dca.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in dca.exported_symbols(), name
    top = header[: header.index("#ifndef DEGA_HIP_H")]
    assert "dega_hip_aggregate_levels_" in top and "encode_levels" in top  # the block comment lists what each entry replaces
    assert re.search(r"#define\s+DEGA_AGG_MAX_LEVELS\s+8\b", header) and dca.AGG_MAX_LEVELS == 8


def test_null_context_or_group_is_rejected(dca):
    L = dca.library()
    job = dca.Job(1, 4, 1, 1, 32, dca.SAMPLES_F32, 100.0)
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    nv = (C.c_size_t * 2)(2, 4)
    two = (C.c_void_p * 2)(p, p)
    sizes = (C.c_size_t * 2)(4, 4)
    E = dca.ERROR_INVALID_VALUE
    assert L.dega_hip_aggregate_levels_dev(None, p, 1, 4, 1, nv, 2, two, sizes, None) == E
    assert L.dega_hip_encode_levels_f32_dev(None, p, 1, 4, 1, nv, 2, 100.0, 1, 32, two, sizes, two, two, None) == E
    assert L.dega_hip_encode_levels_job_host(None, C.byref(job), nv, 2, p, two, sizes, two, two, two) == E
    assert L.dega_hip_group_encode_levels(None, C.byref(job), nv, 2, p, two, sizes, two, two, two) == E


# ---- the planner -----------------------------------------------------------------------------------------------------------

def gx_of(Cn, wide):
    units = Cn // 4 if wide and Cn % 4 == 0 else Cn
    return max(1, (units + 255) // 256)


def check_plan(dca, Cn, T, levels, wide=True):
    assert "DEGA_AGG_LEVELS_MIN_WORKGROUPS" not in os.environ  # the knob named in the header replaces the floor asserted below
    pass_of, step_of = dca.aggregate_levels_plan(Cn, T, levels, wide)
    assert len(pass_of) == len(levels) and 1 <= len(step_of) <= len(levels)  # every level in exactly one pass, never more passes than levels
    assert sorted(set(pass_of)) == list(range(len(step_of)))
    for k, N in enumerate(levels):
        step = step_of[pass_of[k]]
        assert step >= 1 and (step % N == 0 or step >= T), (levels, N, step)
    for p, step in enumerate(step_of):
        members = [N for k, N in enumerate(levels) if pass_of[k] == p]
        if len(members) > 1:  # what let them share: their least common multiple leaves enough ranges
            L = min(math.lcm(*[min(N, T) for N in members]), T)
            assert gx_of(Cn, wide) * -(-T // L) >= 512, (levels, members)
            assert -(-T // step) <= 65535
    return pass_of, step_of


def test_plan_of_the_study_levels_is_one_pass(dca):
    pass_of, step_of = check_plan(dca, 65536, 86400, [60, 300, 900, 3600])
    assert pass_of == [0, 0, 0, 0] and step_of[0] % 3600 == 0
    assert gx_of(65536, True) == 64 and 64 * (86400 // 3600) == 1536


def test_plan_separates_levels_without_a_common_step(dca):
    pass_of, step_of = check_plan(dca, 256, 86400, [899, 900, 901])
    assert sorted(pass_of) == [0, 1, 2]
    pass_of, step_of = check_plan(dca, 256, 86400, [2, 60, 900])  # L = 900 would give 96 ranges x 1 workgroup, below 512
    assert pass_of[0] == pass_of[1] != pass_of[2] and len(step_of) == 2
    assert check_plan(dca, 65536, 86400, [2, 3, 4, 5, 6, 10, 12, 60])[0] == [0] * 8  # L = 60: one pass of eight levels


def test_plan_of_one_level_and_of_none(dca):
    assert check_plan(dca, 4096, 3600, [60])[0] == [0]
    assert check_plan(dca, 1, 1, [1])[0] == [0]
    assert dca.aggregate_levels_plan(4096, 3600, []) == ([], [])


def test_plan_does_not_depend_on_the_order_of_the_levels(dca):
    rng = np.random.default_rng(11)
    pool = [1, 2, 3, 7, 60, 120, 300, 899, 900, 901, 3600, 5000, 100000]
    for _ in range(60):
        levels = [int(n) for n in rng.choice(pool, size=int(rng.integers(1, 9)), replace=False)]
        Cn, T = int(rng.choice([8, 256, 300, 4096, 65536])), int(rng.choice([1801, 3600, 86400]))
        wide = bool(rng.integers(0, 2))
        pass_of, step_of = check_plan(dca, Cn, T, levels, wide)
        groups = {frozenset(N for k, N in enumerate(levels) if pass_of[k] == p): step_of[p] for p in range(len(step_of))}
        perm = [int(i) for i in rng.permutation(len(levels))]
        shuffled = [levels[i] for i in perm]
        pass2, step2 = check_plan(dca, Cn, T, shuffled, wide)
        groups2 = {frozenset(N for k, N in enumerate(shuffled) if pass2[k] == p): step2[p] for p in range(len(step2))}
        assert groups == groups2, (levels, shuffled)


def test_plan_with_huge_levels_neither_traps_nor_wraps(dca):
    huge = [2 ** 40 + 1, 2 ** 41 + 3, 2 ** 63 + 5, 2 ** 64 - 1, 2 ** 32 + 1, 7]
    pass_of, step_of = check_plan(dca, 65536, 86400, huge)
    assert pass_of[5] != pass_of[0] and all(s == 86400 for p, s in enumerate(step_of) if p != pass_of[5])  # anything above T counts as T
    check_plan(dca, 65536, 2 ** 33, [2 ** 31 + 1, 2 ** 31 + 3, 3])  # a series longer than 2^32 rows goes level by level
    assert len(dca.aggregate_levels_plan(65536, 2 ** 33, [2, 4])[1]) == 2


def test_plan_refuses_bad_level_lists(dca):
    L = dca.library()
    pass_of, step_of = (C.c_int * 9)(), (C.c_size_t * 9)()
    E = dca.ERROR_INVALID_VALUE
    assert L.dega_hip_aggregate_levels_plan(256, 100, (C.c_size_t * 2)(2, 0), 2, 1, pass_of, step_of) == E  # a level of 0
    assert L.dega_hip_aggregate_levels_plan(256, 100, (C.c_size_t * 2)(60, 60), 2, 1, pass_of, step_of) == E  # the same N twice
    assert L.dega_hip_aggregate_levels_plan(256, 100, (C.c_size_t * 9)(*range(1, 10)), 9, 1, pass_of, step_of) == E  # more than 8
    assert L.dega_hip_aggregate_levels_plan(256, 100, None, 2, 1, pass_of, step_of) == E
    assert L.dega_hip_aggregate_levels_plan(256, 100, (C.c_size_t * 2)(2, 4), 2, 1, None, step_of) == E


# ---- kernel logic under the emulator ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sim():
    S = sim_library("aggregate_levels")
    S.sim_aggregate_levels.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t]
    return S


def sim_levels(S, v, levels, step, Cn=None, ld_out=None, wide=0):
    v = np.ascontiguousarray(v, dtype=np.float32)
    T, ld = v.shape
    Cn = ld if Cn is None else Cn
    K = len(levels)
    ld_out = [Cn] * K if ld_out is None else ld_out
    outs = [np.full((-(-T // N), ld_out[k]), SENTINEL, dtype=np.float32) for k, N in enumerate(levels)]  # what must not be touched stays recognisable
    ret = S.sim_aggregate_levels(v.ctypes.data, Cn, T, ld, (C.c_size_t * K)(*levels), K, (C.c_void_p * K)(*[o.ctypes.data for o in outs]),
                                 (C.c_size_t * K)(*ld_out), wide, step)
    assert ret == 0, (levels, step)
    return outs


def steps_of(levels, T):
    L = math.lcm(*[min(N, T) for N in levels])
    return sorted({min(L, T) if L < T else T, min(2 * L, T) if 2 * L < T else T, T, T + 5})


def test_kernel_source_matches_the_reference_floats(sim, fx):
    """every fixture case of 2, 3, 4 and 8 levels, dword form and (where C allows) 16-byte form, ranges of L, 2 L and >= T rows"""
    seen = set()
    for name, levels in fx.cases():
        v = fx.series(name)
        seen.add(len(levels))
        for wide in ((0, 1) if v.shape[1] % 4 == 0 else (0,)):
            for step in steps_of(levels, v.shape[0]):
                got = sim_levels(sim, v, levels, step, wide=wide)
                for k, N in enumerate(levels):
                    assert same_floats(got[k], fx.sums(name, N)), (name, levels, N, wide, step)
    assert seen == {2, 3, 4, 8}


def test_kernel_source_every_level_count(sim, fx):
    """K = 2 .. 8 (every instantiation the library dispatches to) on one series, ranges that cut and ranges that do not"""
    v = fx.series("n900_plus1")
    pool = [2, 3, 4, 6, 12, 60, 5, 10]
    for K in range(2, 9):
        levels = pool[:K]
        for wide in (0, 1):
            for step in steps_of(levels, v.shape[0]):
                got = sim_levels(sim, v, levels, step, wide=wide)
                for k, N in enumerate(levels):
                    assert same_floats(got[k], sequential(v, N)), (K, N, wide, step)


def test_kernel_source_ragged_wave_and_pitches(sim, fx):
    rng = np.random.default_rng(6)
    # 300 channels: two workgroups in the dword form, a ragged last wave; 45 rows end inside a group of both levels
    v = (np.round(rng.uniform(0, 5000, (45, 300)) * 100) / 100).astype(np.float32)
    for step in (14, 28, 45):
        got = sim_levels(sim, v, [7, 2], step)
        assert same_floats(got[0], sequential(v, 7)) and same_floats(got[1], sequential(v, 2)), step
    # ld > C and a pitch of its own per level: the columns beyond C are neither read into a result nor written
    base = fx.series("n900_plus1")
    T = base.shape[0]
    wide_in = np.full((T, 16), np.float32(np.nan), dtype=np.float32)
    wide_in[:, :8] = base
    for w in (0, 1):
        got = sim_levels(sim, wide_in, [60, 2, 300], 600, Cn=8, ld_out=[12, 8, 20], wide=w)
        for k, N in enumerate([60, 2, 300]):
            assert same_floats(got[k][:, :8], fx.sums("n900_plus1", N)), (w, N)
            assert (got[k][:, 8:] == SENTINEL).all(), (w, N)
    # a level above T: one row, the sum of all, beside a level that cuts
    got = sim_levels(sim, v, [1000, 5], 45)
    assert same_floats(got[0], sequential(v, 1000)) and got[0].shape == (1, 300) and same_floats(got[1], sequential(v, 5))


def test_the_fixture_tells_a_cheat_apart(fx):
    """a coarser level formed from a finer level's sums rounds differently, and the fixture shows it: for the fixture cases
    whose levels divide each other, the nested sum differs from the reference's floats on the series named here"""
    expect = {(2, 60): {"chain_meter", "n60_mult", "n900_plus1", "alternating_n60"}, (60, 120): {"chain_meter", "n60_mult", "n900_plus1", "alternating_n60"},
              (7, 21): {"chain_meter", "n60_mult", "n900_plus1", "alternating_n60"}, (60, 300): {"chain_meter", "n60_mult", "n900_plus1"}}
    found = {pair: set() for pair in expect}
    for name, levels in fx.cases():
        for fine in levels:
            for coarse in levels:
                if coarse > fine > 1 and coarse % fine == 0:
                    nested = sequential(fx.sums(name, fine), coarse // fine)
                    assert nested.shape == fx.sums(name, coarse).shape
                    if (fine, coarse) in expect and not same_floats(nested, fx.sums(name, coarse)):
                        found[(fine, coarse)].add(name)
    for pair, names in expect.items():
        assert names <= found[pair], (pair, names - found[pair])


def test_fixture_equals_the_restatement_from_the_base_series(fx):
    n = 0
    for name, levels in fx.cases():
        for N in levels:
            assert same_floats(sequential(fx.series(name), N), fx.sums(name, N)), (name, N)
            n += 1
    assert n >= 100 and fx.series("meter3601").shape == (3601, 12)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "aggregate_levels.npz")) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "aggregate.npz"))
