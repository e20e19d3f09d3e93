"""The LZMH restatement (oracle/lzmh_oracle.c) against the fixtures made from the compiled reference
(tests/golden/lzmh.json, lzmh.npz, lzmh_random.json) and, where oracle/_ref exists, against the compiled reference itself."""
import gzip
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fixtures():
    with open(os.path.join(GOLDEN, "lzmh.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, "lzmh.npz"))


def test_lzmh_testfile_golden(fixtures):
    meta = fixtures[0]["testfile"]
    with gzip.open(os.path.join(GOLDEN, "input.txt.gz"), "rb") as f:
        raw = f.read()
    ret, b, n = orc.stage("lzmh", True, raw, 8 * len(raw))
    assert ret == 0
    data = orc.file_bytes(b, n)
    assert len(data) == meta["file_bytes"] == 270896
    assert (n // 8, n % 8) == (meta["wrote_bytes"], meta["wrote_bits"])
    assert hashlib.sha256(data).hexdigest() == meta["sha256"]
    assert meta["sha256"].startswith("c493269c") and meta["roundtrip_identical"]
    ret, d, dn = orc.stage("lzmh", False, b, n)
    assert ret == 0 and dn == 8 * len(raw) and d == raw


def test_lzmh_small_goldens(fixtures):
    meta, z = fixtures
    names = sorted(k[:-3] for k in z.files if k.endswith(".in"))
    assert len(names) >= 20
    for name in names:
        data = z[name + ".in"].tobytes()
        ret, b, n = orc.stage("lzmh", True, data, 8 * len(data))
        assert ret == 0 and n == int(z[name + ".bits"][0]), name
        assert b[: (n + 7) // 8] == z[name + ".stream"].tobytes(), name
        ret, d, dn = orc.stage("lzmh", False, b, n)
        assert ret == 0 and d[: dn // 8] == z[name + ".dec"].tobytes(), name
        assert (d[: dn // 8] == data) == meta[name]["decodes_to_input"], name
    # the reference's quirks are part of the fixtures: exactly one ring of input encodes to nothing, and the decoder
    # turns an empty stream into one zero byte
    assert meta["digits_403"]["bits"] == 0 and meta["digits_0"]["decoded_bytes"] == 1


def test_lzmh_rejects_partial_byte():
    assert orc.stage("lzmh", True, b"\xff\x80", 9)[0] == orc.ERROR_LIBRARY_CALL


def sha(b):
    return hashlib.sha256(b).hexdigest()


def random_inputs():
    """The seeded random byte strings of the comparison with the compiled reference: (data, 40 garbage bytes) per case."""
    rng = np.random.default_rng(3)
    for it in range(300):
        kind = it % 5
        L = int(rng.integers(0, 1500)) if it % 7 else [0, 1, 2, 3, 402, 403, 404, 405, 806][it % 9]
        if kind == 0:
            data = bytes(rng.integers(0, 256, L, dtype=np.uint8))
        elif kind == 1:
            data = ("".join("%.2f\n" % v for v in rng.uniform(0, 400, L // 6 + 1)))[:L].encode()
        elif kind == 2:
            data = bytes(rng.integers(48, 58, L, dtype=np.uint8))
        elif kind == 3:
            data = bytes(rng.integers(0, 3, L, dtype=np.uint8))
        else:
            data = (b"abcabcabd" * (L // 9 + 1))[:L]
        yield data, bytes(rng.integers(0, 256, 40, dtype=np.uint8))


def long_inputs():
    rng = np.random.default_rng(42)
    return [bytes(rng.integers(48, 58, 1_500_000, dtype=np.uint8)), bytes(600_000)]


def reference_record(data, garbage=None):
    """The compiled reference (oracle/_ref) on one input: [status, bits, sha256] of `encode lzmh`, the same of
    `decode lzmh` of that stream, and [status, bits] of `decode lzmh` of the garbage (the reference reads never-written
    list symbols there, lzmh.c:395, :434, so only the status and the length are defined)."""
    r = orc.ref_run_chain(data, 8 * len(data), ["encode lzmh"])
    dr = orc.ref_run_chain(r[1], r[2], ["decode lzmh"])
    rec = [[r[0], r[2], sha(r[1])], [dr[0], dr[2], sha(dr[1])]]
    if garbage is not None:
        gr = orc.ref_run_chain(garbage, 8 * len(garbage), ["decode lzmh"])
        rec.append([gr[0], gr[2]])
    return rec


@pytest.fixture(scope="module")
def recorded():
    """The compiled reference's results on random_inputs() and long_inputs() (tests/golden/lzmh_random.json, recorded by
    make_golden.py); where oracle/_ref is built, every record is also checked against the live reference."""
    with open(os.path.join(GOLDEN, "lzmh_random.json")) as f:
        return json.load(f)


def test_lzmh_restatement_equals_compiled_reference_on_random_inputs(recorded):
    want = recorded["random_inputs"]
    cases = list(random_inputs())
    assert len(want) == len(cases) == 300
    for it, ((data, g), rec) in enumerate(zip(cases, want)):
        if orc.have_ref():
            assert reference_record(data, g) == rec, it
        a = orc.stage("lzmh", True, data, 8 * len(data))
        assert [a[0], a[2], sha(a[1])] == rec[0], (it, len(data))
        d = orc.stage("lzmh", False, a[1], a[2])
        assert [d[0], d[2], sha(d[1])] == rec[1], (it, len(data))
        d = orc.stage("lzmh", False, g, 8 * len(g))
        assert [d[0], d[2]] == rec[2], it


def test_lzmh_restatement_equals_compiled_reference_on_long_inputs(recorded):
    """Count saturation at 65 535 (lzmh.c:304) and back-to-back 274-byte matches: beyond what the short fixtures reach."""
    want = recorded["long_inputs"]
    assert len(want) == 2
    for data, rec in zip(long_inputs(), want):
        if orc.have_ref():
            assert reference_record(data) == rec
        a = orc.stage("lzmh", True, data, 8 * len(data))
        assert [a[0], a[2], sha(a[1])] == rec[0]
        d = orc.stage("lzmh", False, a[1], a[2])
        assert [d[0], d[2], sha(d[1])] == rec[1] and d[1] == data
