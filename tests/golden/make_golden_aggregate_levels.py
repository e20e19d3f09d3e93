#!/usr/bin/env python3
"""Generates tests/golden/aggregate_levels.npz from the COMPILED REFERENCE LIBRARY in process (oracle/_ref/libdcref.so
through orc.ref_run_chain), like make_golden_aggregate.py.  Build container only:

    make -C oracle && python tests/golden/make_golden_aggregate_levels.py

The granularity study runs `encode aggregate num_values=N` once per level over the SAME readings; the fixture holds what
the reference writes for every (series, N) that a level set below needs.  Data only:
  set<i>.levels   int64 [K]      one level set, in the order a caller would give it
  set<i>.series   str [..]       the series that set is checked on
  <series>.v      float32 [T][C] only for series that tests/golden/aggregate.npz does not already hold under that name
  <series>.N<N>.a float32 [ceil(T/N)][C]   what `encode aggregate num_values=N` writes for every channel
and for the (series, N) that go on into the coder, per (valuesize, adaptive) in CHAIN_CONFIGS:
  <series>.N<N>.vs<V>.<ad|st>.stream / .bits / .err    `encode aggregate # encode normalize # encode diff # encode seg #
                                                       encode bac [adaptive]` as in aggregate.npz
  <series>.factor  float32       normalization_factor of those chains

The generator asserts that a strict left-to-right float32 loop over the BASE series reproduces the reference on every
case, and that a coarser level formed from a finer level's sums does NOT (on the series and pairs listed in NESTED):
otherwise the fixture could not tell a kernel that chains its levels from a correct one.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from oracle import orc  # noqa: E402
from make_golden_aggregate import CHAIN_CONFIGS, meter, ref_aggregate, ref_chain, same_floats, sequential  # noqa: E402

TINY = ("chain_meter", "alternating_n60", "special_n2")  # every set
SMALL = TINY + ("n900_plus1",)
LONG = SMALL + ("meter3601",)
ALL = LONG + ("n60_mult",)  # (the wide and the long series: only the sets whose fine levels keep the file small)
SETS = (((2, 60), SMALL + ("n60_mult",)), ((60, 300), ALL), ((7, 3, 21), SMALL), ((7, 21), ("n60_mult",)), ((60, 300, 900, 3600), ALL), ((1, 2, 900), TINY),
        ((7, 60), LONG), ((899, 900, 901), LONG), ((2, 3, 4, 5, 6, 10, 12, 60), TINY), ((60, 120), ALL), ((2, 5000), SMALL))
NESTED = {(2, 60): ("chain_meter", "n60_mult", "n900_plus1", "alternating_n60"), (60, 120): ("chain_meter", "n60_mult", "n900_plus1", "alternating_n60"),
          (7, 21): ("chain_meter", "n60_mult", "n900_plus1", "alternating_n60"), (60, 300): ("chain_meter", "n60_mult", "n900_plus1")}
CHAINS = {"chain_meter": (1.0, (2, 60, 300, 900)), "meter3601": (1.0, (60, 300, 900, 3600))}


def main():
    assert orc.have_ref(), "oracle/_ref/libdcref.so is not built (make -C oracle)"
    base = np.load(os.path.join(HERE, "aggregate.npz"))
    rng = np.random.default_rng(20152)
    series = {name: base[name + ".v"] for name in ALL if name + ".v" in base.files}
    series["meter3601"] = meter(rng, 3601, 12, top=50.0)
    out = {"meter3601.v": series["meter3601"]}
    for i, (levels, names) in enumerate(SETS):
        out["set%d.levels" % i] = np.array(levels, dtype=np.int64)
        out["set%d.series" % i] = np.array(names)
        for name in names:
            for N in levels:
                key = "%s.N%d.a" % (name, N)
                if key in out:
                    continue
                v = series[name]
                a = ref_aggregate(v, N)
                assert same_floats(sequential(v, N), a), "a strict sequential float32 sum does not reproduce the reference on " + key
                out[key] = a
    for (fine, coarse), names in NESTED.items():
        for name in names:
            nested = sequential(out["%s.N%d.a" % (name, fine)], coarse // fine)
            assert not same_floats(nested, out["%s.N%d.a" % (name, coarse)]), "level %d from level %d is not told apart on %s" % (coarse, fine, name)
    for name, (factor, levels) in CHAINS.items():
        out[name + ".factor"] = np.float32(factor)
        for N in levels:
            assert "%s.N%d.a" % (name, N) in out
            for vs, ad in CHAIN_CONFIGS:
                s, b, e = ref_chain(series[name], N, factor, vs, ad)
                key = "%s.N%d.vs%d.%s." % (name, N, vs, "ad" if ad else "st")
                out[key + "stream"], out[key + "bits"], out[key + "err"] = s, b, e
    path = os.path.join(HERE, "aggregate_levels.npz")
    np.savez_compressed(path, **out)
    print("%s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))
    assert os.path.getsize(path) < os.path.getsize(os.path.join(HERE, "aggregate.npz"))


if __name__ == "__main__":
    main()
