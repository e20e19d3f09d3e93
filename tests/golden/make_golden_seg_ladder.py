#!/usr/bin/env python3
"""Generates tests/golden/seg_ladder.npz from the COMPILED REFERENCE LIBRARY in process (oracle/_ref/libdcref.so through
orc.ref_run_chain, as the other generators do).  Build container only:

    make -C oracle && python tests/golden/make_golden_seg_ladder.py

The series are those of tests/seg_ladder_common.py (closed form and seeded; the fixture stores a checksum of what the
reference was given): at each of its value sizes the channels of golden_channels() -- one of every accepted kind and two
refused ones -- through `encode diff valuesize=n # encode seg valuesize=n # encode bac [adaptive]` and, where that is
accepted, back through the three decodes.  Data only, few and compact arrays (S value sizes, models in the order adaptive,
static, K channels):
  sizes [S], channels [K], input_sha256 [S][32]   SHA-256 of the uint64 samples [T][K] the reference was given
  err int32 [S][2][K], bits uint64 [S][2][K]      statuses and bit lengths
  vs<n>.stream uint8 [K][cap]                     the adaptive model's streams, zero padded
  static_sha256 uint8 [S][K][32]                  SHA-256 of the static model's streams (they are twice as long)
  lossy int64 [n][3], lossy_dec uint64 [n][T64]   (index of the value size, model, index of the channel) of every accepted
                                                  channel whose decoded fields are NOT the ones that went in, and those
                                                  fields: value size 64, the differences of magnitude 2^63.  For every other
                                                  accepted channel the decoded fields were the input, whose checksum stands
                                                  for them.
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import orc  # noqa: E402
import hostile_common as hc  # noqa: E402
import seg_ladder_common as sl  # noqa: E402


def digest(data):
    return np.frombuffer(hashlib.sha256(data).digest(), dtype=np.uint8)


def main():
    chans = sl.golden_channels()
    S, K = len(sl.SIZES), len(chans)
    out = {"sizes": np.array(sl.SIZES, dtype=np.int64), "channels": np.array(chans, dtype=np.int64)}
    out["input_sha256"] = np.zeros((S, 32), dtype=np.uint8)
    out["err"] = np.zeros((S, 2, K), dtype=np.int32)
    out["bits"] = np.zeros((S, 2, K), dtype=np.uint64)
    out["static_sha256"] = np.zeros((S, K, 32), dtype=np.uint8)
    lossy, lossy_dec = [], []
    for s, vs in enumerate(sl.SIZES):
        corp = sl.corpus(vs)
        opt = " valuesize=%d" % vs
        out["input_sha256"][s] = digest(np.ascontiguousarray(corp.x[:, chans]).tobytes())
        for m, ad in enumerate((1, 0)):
            bac = "bac adaptive" if ad else "bac"
            streams = []
            for i, c in enumerate(chans):
                data, n = hc.pack_be(corp.x[:, c], vs)
                ret, b, nb, _ = orc.ref_run_chain(data, n, ["encode diff" + opt, "encode seg" + opt, "encode " + bac])
                out["err"][s, m, i] = ret
                streams.append(b if ret == 0 else b"")
                if ret == 0:
                    out["bits"][s, m, i] = nb
                    rd, d, dn, _ = orc.ref_run_chain(b, nb, ["decode " + bac, "decode seg" + opt, "decode diff" + opt])
                    assert rd == 0 and dn == n, (vs, ad, c, rd, dn)
                    dec = hc.unpack_be(d, dn, vs)
                    if (dec != corp.x[:, c]).any():
                        lossy.append((s, m, i))
                        lossy_dec.append(dec)
            if ad:
                arr = np.zeros((K, max(1, max(len(b) for b in streams))), dtype=np.uint8)
                for i, b in enumerate(streams):
                    arr[i, : len(b)] = np.frombuffer(b, dtype=np.uint8)
                out["vs%d.stream" % vs] = arr
            else:
                for i, b in enumerate(streams):
                    out["static_sha256"][s, i] = digest(b)
        print("vs %d: T %d, statuses %s" % (vs, corp.T, out["err"][s, 0].tolist()))
    assert all(sl.SIZES[s] == 64 for s, _, _ in lossy)
    out["lossy"] = np.array(lossy, dtype=np.int64).reshape(-1, 3)
    out["lossy_dec"] = np.array(lossy_dec, dtype=np.uint64).reshape(len(lossy), -1)
    print("lossy (size, model, channel):", [(sl.SIZES[s], m, chans[i]) for s, m, i in lossy])
    path = os.path.join(HERE, "seg_ladder.npz")
    np.savez_compressed(path, **out)
    print("seg_ladder.npz: %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
