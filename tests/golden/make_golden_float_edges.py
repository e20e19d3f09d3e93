#!/usr/bin/env python3
"""Generates tests/golden/float_edges.npz from the COMPILED REFERENCE LIBRARY in process (oracle/_ref/libdcref.so through
orc.ref_run_chain, as the other generators do).  Build container only:

    make -C oracle && python tests/golden/make_golden_float_edges.py

The corpus, the channels and the integer series are those of tests/float_edges_common.py (seeded; the fixture stores a
checksum of what the reference was given).  `encode normalize` runs on every value alone, so that every value has a verdict
of its own -- the values that the restatement takes for in range first as one stream, which the reference either accepts as
a whole or, if it does not, value by value like the rest.  `decode normalize` runs on integers(vs).  The whole chain
`encode normalize # encode diff # encode seg # encode bac [adaptive]` and its inverse run on a thin sample of the channel
sets, and `decode csv # encode normalize # ...` on the texts of TEXT_LINES.  The layout is EdgeFixture's (data only).
The same run gives the same bytes.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import orc  # noqa: E402
import float_edges_common as fe  # noqa: E402
import csv_read_common as crc  # noqa: E402


def options(vs, factor):
    return " normalization_factor=%r valuesize=%d" % (float(factor), vs)


def ref_normalize_each(bits, factor, vs):
    """(failed bool [n], fields uint64 [n]) of `encode normalize` on every value alone"""
    stage = ["encode normalize" + options(vs, factor)]
    failed = np.zeros(bits.size, dtype=bool)
    fields = np.zeros(bits.size, dtype=np.uint64)
    ok, _ = fe.normalize(bits, factor, vs)
    alone = np.flatnonzero(~ok)
    accepted = np.flatnonzero(ok)
    ret, b, n, _ = orc.ref_run_chain(bits[accepted].tobytes(), 32 * accepted.size, stage)
    if ret == 0 and n == vs * accepted.size:
        fields[accepted] = fe.unpack_fields(b, n, vs)
    else:
        alone = np.arange(bits.size)
    for i in alone:
        ret, b, n, _ = orc.ref_run_chain(bits[i: i + 1].tobytes(), 32, stage)
        failed[i] = ret != 0
        if ret == 0:
            assert n == vs
            fields[i] = fe.unpack_fields(b, n, vs)[0]
        else:
            assert ret == fe.INVALID, ret
    return failed, fields


def ref_denormalize(u, factor, vs):
    data, n = fe.pack_fields(u, vs)
    ret, b, nb, _ = orc.ref_run_chain(data, n, ["decode normalize" + options(vs, factor)])
    assert ret == 0 and nb == 32 * u.size, (ret, nb)
    return np.frombuffer(b, dtype=np.uint32).copy()


def chain_stages(vs, factor, ad):
    opt = " valuesize=%d" % vs
    bac = "bac" + (" adaptive" if ad else "")
    enc = ["encode normalize" + options(vs, factor), "encode diff" + opt, "encode seg" + opt, "encode " + bac]
    dec = ["decode " + bac, "decode seg" + opt, "decode diff" + opt, "decode normalize" + options(vs, factor)]
    return enc, dec


def streams_array(streams):
    out = np.zeros((len(streams), max([len(s) for s in streams] + [1])), dtype=np.uint8)
    for i, s in enumerate(streams):
        out[i, : len(s)] = np.frombuffer(s, dtype=np.uint8)
    return out


def main():
    assert orc.have_ref(), "oracle/_ref/libdcref.so is not built (make -C oracle)"
    out = {}
    differ = []
    for vs, factor in fe.KEYS:
        k = fe.key(vs, factor)
        bits, cls = fe.values(vs, factor)
        ok, n = fe.normalize(bits, factor, vs)
        failed, fields = ref_normalize_each(bits, factor, vs)
        out[k + ".in"] = fe.crc(bits)
        out[k + ".status"] = np.packbits(failed ^ ~ok)
        out[k + ".int"] = fields ^ n
        for i in np.flatnonzero((failed ^ ~ok) | (fields != n))[:3]:
            differ.append((k, "normalize", fe.CLASSES[cls[i]], hex(int(bits[i])), bool(failed[i]), hex(int(fields[i])), bool(ok[i]), hex(int(n[i]))))
        u = fe.integers(vs)
        den, want = ref_denormalize(u, factor, vs), fe.denormalize(u, factor, vs)
        same = fe.same_float_bits(den, want)
        out[k + ".den.in"] = fe.crc(u)
        out[k + ".den"] = np.where(same, 0, den ^ want).astype(np.uint32)
        for i in np.flatnonzero(~same)[:3]:
            differ.append((k, "denormalize", hex(int(u[i])), hex(int(den[i])), hex(int(want[i]))))
        if factor in (100.0, 1.0):
            lit = np.flatnonzero((cls == fe.CLASSES.index("bounds")) | (cls == fe.CLASSES.index("specials")))
            out[k + ".lit.in"] = bits[lit]
            out[k + ".lit.status"] = np.where(failed[lit], fe.INVALID, 0).astype(np.int8)
            out[k + ".lit.int"] = fields[lit]

    for vs, factor in fe.FUSED_IN_FIXTURE:
        v, _ = fe.channels(vs, factor)
        idx = np.arange(0, v.shape[1], 15)
        for ad in (1, 0):
            enc, dec = chain_stages(vs, factor, ad)
            err, nbits, streams, back = [], [], [], np.zeros((v.shape[0], idx.size), dtype=np.uint32)
            for j, c in enumerate(idx):
                col = np.ascontiguousarray(v[:, c])
                ret, b, nb, _ = orc.ref_run_chain(col.tobytes(), 32 * col.size, enc)
                err.append(ret)
                nbits.append(nb if ret == 0 else 0)
                streams.append(b if ret == 0 else b"")
                if ret == 0:
                    r2, fb, fn, _ = orc.ref_run_chain(b, nb, dec)
                    assert r2 == 0 and fn == 32 * col.size, (vs, factor, ad, c, r2, fn)
                    _, fields = fe.normalize(col, factor, vs)
                    want = fe.denormalize(fields, factor, vs)
                    got = np.frombuffer(fb, dtype=np.uint32)
                    back[:, j] = np.where(fe.same_float_bits(got, want), 0, got ^ want)
            k = "%s.%s.chain" % (fe.key(vs, factor), "ad" if ad else "st")
            out[k + ".idx"] = idx.astype(np.int32)
            out[k + ".err"] = np.array(err, dtype=np.int32)
            out[k + ".bits"] = np.array(nbits, dtype=np.uint64)
            out[k + ".stream"] = streams_array(streams)
            out[k + ".back"] = back
            assert (np.array(err) == 0).any() and (np.array(err) != 0).any(), (vs, factor, ad)

    texts = [crc.lines_text(lines) for lines in fe.TEXT_LINES]
    for vs in fe.TEXT_SIZES:
        for ad in (1, 0):
            err, nbits, streams = [], [], []
            for t in texts:
                ret, b, nb, _ = orc.ref_run_chain(t, 8 * len(t), fe.text_chain_stages(vs, ad))
                err.append(ret)
                nbits.append(nb if ret == 0 else 0)
                streams.append(b if ret == 0 else b"")
            k = "text.n%d.%s" % (vs, "ad" if ad else "st")
            out[k + ".err"] = np.array(err, dtype=np.int32)
            out[k + ".bits"] = np.array(nbits, dtype=np.uint64)
            out[k + ".stream"] = streams_array(streams)

    fe.save_npz(fe.FIXTURE, out)
    size = os.path.getsize(fe.FIXTURE)
    print("%s: %d arrays, %d bytes" % (fe.FIXTURE, len(out), size))
    print("%d places where the reference and the restatement differ%s" % (len(differ), ":" if differ else ""))
    for d in differ:
        print("  ", d)
    assert size <= max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.endswith(".npz") and f != "float_edges.npz")


if __name__ == "__main__":
    main()
