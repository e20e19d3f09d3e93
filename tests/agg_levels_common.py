"""Shared by tests/test_aggregate_levels_host.py and tests/test_gpu_aggregate_levels.py: reading
tests/golden/aggregate_levels.npz (the compiled reference's floats and streams, one run of `encode aggregate
num_values=N` per level; see tests/golden/make_golden_aggregate_levels.py)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHAIN_CONFIGS = ((32, 1), (32, 0), (16, 1), (16, 0))


class Fixture:
    def __init__(self):
        self.z = np.load(os.path.join(GOLDEN, "aggregate_levels.npz"))
        self.base = np.load(os.path.join(GOLDEN, "aggregate.npz"))

    def series(self, name):
        return self.z[name + ".v"] if name + ".v" in self.z.files else self.base[name + ".v"]

    def sums(self, name, N):
        return self.z["%s.N%d.a" % (name, N)]

    def cases(self):
        """(series name, levels) of every fixture case"""
        i = 0
        while "set%d.levels" % i in self.z.files:
            levels = [int(n) for n in self.z["set%d.levels" % i]]
            for name in self.z["set%d.series" % i]:
                yield str(name), levels
            i += 1

    def chains(self):
        """(series name, factor, [N ...]) of the series that go on into the coder"""
        for key in self.z.files:
            if key.endswith(".factor"):
                name = key[:-7]
                Ns = sorted({int(k.split(".")[1][1:]) for k in self.z.files if k.startswith(name + ".N") and k.endswith(".vs32.ad.bits")})
                yield name, float(self.z[key]), Ns

    def chain(self, name, N, vs, ad):
        key = "%s.N%d.vs%d.%s." % (name, N, vs, "ad" if ad else "st")
        return self.z[key + "stream"], self.z[key + "bits"], self.z[key + "err"]
