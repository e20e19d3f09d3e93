"""The `aggregate` feature (DCLib/src/aggregate.c:9-26) without a GPU: the C ABI's new symbols and argument checks, the
"gaggregate" row of the host plugin table, and the kernel's LOGIC -- the shipped kernel source compiled by g++ under the
thread-per-lane emulator of tests/sim/ against tests/golden/aggregate.npz (the compiled reference's floats).  The parity
tests proper are tests/test_gpu_aggregate.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from __graft_entry__ import load_package
from oracle import orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from agg_common import same_floats, sequential  # noqa: E402
from sim_build import sim_library  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "data-compressor_amd", "host")
GOLDEN = os.path.join(ROOT, "tests", "golden")
CLI = os.path.join(HOST, "dccli_amd")

NEW_SYMBOLS = ("dega_hip_aggregate_rows", "dega_hip_aggregate_dev", "dega_hip_aggregate_host", "dega_hip_encode_agg_f32_dev",
               "dega_hip_encode_agg_job_host", "dega_hip_group_encode_agg")


@pytest.fixture(scope="module")
def dca():
    mod = load_package()
    if not os.path.exists(mod.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return mod


@pytest.fixture(scope="module")
def hostlib(dca):
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    L = C.CDLL(os.path.join(HOST, "libdclib_amd.so"))
    L.GetEncoder.restype = C.c_void_p
    L.GetEncoder.argtypes = [C.c_char_p]
    L.GetNumberOfEncoders.restype = C.c_size_t
    L.EncoderSupportsOption.argtypes = [C.c_char_p, C.c_char_p]
    return L


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "aggregate.npz"))


def float_cases(z):
    return sorted(k[:-2] for k in z.files if k.endswith(".v"))


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
    assert "aggregate.c" in header  # the header cites what the entry points replace, like the others


def test_aggregate_rows(dca):
    f = dca.library().dega_hip_aggregate_rows
    for T, N, want in ((0, 1, 0), (0, 60, 0), (1, 1, 1), (1000, 60, 17), (1001, 60, 17), (1020, 60, 17), (1021, 60, 18), (86400, 900, 96),
                       (86400, 60, 1440), (59, 60, 1), (5, 7, 1), (7, 7, 1), (8, 7, 2), (86400, 1, 86400), (2 ** 40 + 1, 2, 2 ** 39 + 1)):
        assert f(T, N) == want == (T + N - 1) // N, (T, N)
    assert f(1000, 0) == 0 and f(0, 0) == 0


def test_null_context_or_group_is_rejected(dca):
    L = dca.library()
    job = dca.Job(1, 4, 1, 1, 32, dca.SAMPLES_F32, 100.0)
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    E = dca.ERROR_INVALID_VALUE
    assert L.dega_hip_aggregate_dev(None, p, 1, 4, 1, 2, p, 1, None) == E
    assert L.dega_hip_aggregate_host(None, p, 1, 4, 1, 2, p, 1) == E
    assert L.dega_hip_encode_agg_f32_dev(None, p, 1, 4, 1, 2, 100.0, 1, 32, p, 4, p, p, None) == E
    assert L.dega_hip_encode_agg_job_host(None, C.byref(job), 2, p, p, 64, p, p, p) == E
    assert L.dega_hip_group_encode_agg(None, C.byref(job), 2, p, p, 64, p, p, p) == E


# ---- plugin table ----------------------------------------------------------------------------------------------------------

def test_codec_table_lists_gaggregate(hostlib):
    names = (C.c_char_p * hostlib.GetNumberOfEncoders())()
    hostlib.GetEncoderNames(names)
    listed = [n.decode() for n in names]
    assert listed == sorted(listed) and "gaggregate" in listed  # sorted: bsearch depends on it
    assert listed.index("fdega") < listed.index("gaggregate") < listed.index("glzmh")
    for name in listed:  # every row is still found through the prefix comparator (DCLib/src/enc_dec.c:89-98)
        assert hostlib.GetEncoder(name.encode()), name
    assert len({hostlib.GetEncoder(n.encode()) for n in listed}) == len(listed)

    class EncDec(C.Structure):
        _fields_ = [("encoder", C.c_void_p), ("decoder", C.c_void_p)]
    row = EncDec.from_address(hostlib.GetEncoder(b"gaggregate"))
    assert row.encoder and not row.decoder  # encoder only, as DCLib/src/enc_dec.c:52
    assert hostlib.EncoderSupportsOption(b"gaggregate", b"num_values") and hostlib.EncoderSupportsOption(b"gaggregate", b"num_channels")
    assert not hostlib.EncoderSupportsOption(b"gaggregate", b"adaptive")
    assert not hostlib.GetEncoder(b"aggregate")  # the reference's CPU codec is not registered here, and the new name does not extend it


def test_fdega_still_does_not_take_num_values(hostlib):
    """the option's default is 2: were it on the fdega row, every existing `encode fdega` would halve its input"""
    assert not hostlib.EncoderSupportsOption(b"fdega", b"num_values")
    assert not hostlib.EncoderSupportsOption(b"dega", b"num_values")


def test_cli_refuses_to_decode_gaggregate(hostlib, tmp_path):
    src = tmp_path / "in.f32"
    src.write_bytes(np.arange(8, dtype=np.float32).tobytes())
    p = subprocess.run([CLI, str(src), str(tmp_path / "o.bin"), "decode", "gaggregate"], capture_output=True, text=True)
    assert p.returncode == (-4) & 0xFF  # ERROR_INVALID_MODE, what the reference gives for `decode aggregate` (DCCLI/src/params.c:241-246)
    p = subprocess.run([CLI, str(src), str(tmp_path / "o.bin"), "encode", "gaggregate", "adaptive"], capture_output=True, text=True)
    assert p.returncode != 0  # an option the row does not list
    p = subprocess.run([CLI, str(src), str(tmp_path / "o.bin"), "encode", "gaggregate", "num_values=0"], capture_output=True, text=True)
    assert p.returncode != 0 and "Invalid value" in p.stderr  # refused before any GPU is looked for


# ---- kernel logic under the emulator ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sim():
    S = sim_library("aggregate")
    S.sim_aggregate.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_size_t]
    return S


def sim_aggregate(S, v, N, Cn=None, ld_out=None, wide=0, ranges=1):
    v = np.ascontiguousarray(v, dtype=np.float32)
    T, ld = v.shape
    Cn = ld if Cn is None else Cn
    ld_out = Cn if ld_out is None else ld_out
    T_out = (T + N - 1) // N
    a = np.full((T_out, ld_out), np.float32(-12345.0), dtype=np.float32)  # what the kernel must not touch stays recognisable
    assert S.sim_aggregate(v.ctypes.data, Cn, T, ld, N, a.ctypes.data, ld_out, wide, ranges) == 0
    return a


def test_kernel_source_matches_the_reference_floats(sim, golden):
    """every fixture case, dword form and (where C allows) 16-byte form, one range of output rows and several"""
    names = float_cases(golden)
    assert len(names) >= 17
    for name in names:
        v, N, want = golden[name + ".v"], int(golden[name + ".N"]), golden[name + ".a"]
        for wide in ((0, 1) if v.shape[1] % 4 == 0 else (0,)):
            for ranges in (1, 3, 1000):
                got = sim_aggregate(sim, v, N, wide=wide, ranges=ranges)
                assert same_floats(got, want), (name, wide, ranges)


def test_kernel_source_ragged_wave_and_pitches(sim, golden):
    rng = np.random.default_rng(5)
    # 300 channels: two workgroups in the dword form, a ragged last wave; 7 does not divide 45
    v = (np.round(rng.uniform(0, 5000, (45, 300)) * 100) / 100).astype(np.float32)
    assert same_floats(sim_aggregate(sim, v, 7, ranges=4), sequential(v, 7))
    # ld > C and ld_out != ld: the columns beyond C are neither read into a result nor written
    wide_in = np.full((62, 80), np.float32(np.nan), dtype=np.float32)
    wide_in[:, :72] = golden["n7_minus1.v"]
    for w in (0, 1):
        got = sim_aggregate(sim, wide_in, 7, Cn=72, ld_out=76, wide=w, ranges=2)
        assert same_floats(got[:, :72], golden["n7_minus1.a"]), w
        assert (got[:, 72:] == np.float32(-12345.0)).all(), w
    # num_values > T: one row, the sum of all
    assert same_floats(sim_aggregate(sim, v, 1000), sequential(v, 1000)) and sequential(v, 1000).shape == (1, 300)


def test_sequential_restatement_tells_orders_apart(golden):
    """the restatement the other tests lean on equals the fixture everywhere, and a pairwise sum does not: the fixture can
    tell a reassociating kernel from a correct one"""
    differs = 0
    for name in float_cases(golden):
        v, N, want = golden[name + ".v"], int(golden[name + ".N"]), golden[name + ".a"]
        assert same_floats(sequential(v, N), want), name
        with np.errstate(all="ignore"):
            differs += 0 if same_floats(np.add.reduceat(v, np.arange(0, v.shape[0], N), axis=0), want) else 1
    assert differs > 0
    z = golden["special_n1.v"], golden["special_n1.a"]
    assert np.signbit(z[0][:, 0]).all() and not np.signbit(z[1][:, 0]).any()  # num_values = 1 is no copy: -0.0f comes out as +0.0f


def test_restatement_matches_the_compiled_reference_on_random_shapes():
    if not orc.have_ref():
        pytest.skip("oracle/_ref/libdcref.so is built where the reference's sources are; elsewhere the fixture stands for it")
    rng = np.random.default_rng(77)
    for _ in range(40):
        T, N = int(rng.integers(1, 400)), int(rng.choice([1, 2, 3, 7, 60, 900, int(rng.integers(1, 50))]))
        col = (rng.uniform(-1, 1, T) * 10.0 ** rng.integers(-3, 9, T)).astype(np.float32)
        ret, b, n, _ = orc.ref_run_chain(col.tobytes(), T * 32, ["encode aggregate num_values=%d" % N])
        assert ret == 0 and n == 32 * ((T + N - 1) // N)
        assert same_floats(sequential(col.reshape(-1, 1), N)[:, 0], np.frombuffer(b, dtype=np.float32)), (T, N)
