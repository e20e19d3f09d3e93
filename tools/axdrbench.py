#!/usr/bin/env python3
"""Times the A-XDR kernels on a resident batch and writes profiles/axdr_bench.txt.

    python tools/axdrbench.py [--channels 65536] [--samples 86400] [--runs 20] [--warmup 3] [--sizes 8,16,24,32,64]

Per value size: dega_hip_axdr_encode_dev (pack) and dega_hip_axdr_decode_dev (unpack) on float32 readings, and IN THE SAME
JOB, run by run in turn with them, the 4-byte dega_hip_to_channel_major_dev of the same image: the kernel with the same access
pattern, which at value size 32 moves exactly the pack kernel's bytes (8 per sample), so it is the yardstick.  hipEvents on
the launches' stream (torch.cuda.Event is one), warm-up runs, medians with fastest, 90th percentile and slowest; the
transposition's own run-to-run spread, the ratios, and the fraction of the HBM peak (8 TB/s).
Every output is verified before anything is timed: the round trip against the library's normalize / denormalize kernels on
the whole image (value sizes up to 32), and a few channels against the oracle's `encode normalize` byte for byte."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.aggbench import event_ms, spread  # noqa: E402

HBM_PEAK_TBS = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=65536)
    ap.add_argument("--samples", type=int, default=86400)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="8,16,24,32,64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "axdr_bench.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from __graft_entry__ import load_package
    from oracle import orc
    dca = load_package()
    ctx = dca.Context(0)
    Cn, T = args.channels, args.samples
    lines, results = [], {}

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("resident: %d channels x %d float32 readings (%.1f GB); %d timed runs per candidate, in turn, %d warm-up runs; hipEvents"
        % (Cn, T, Cn * T * 4 / 1e9, args.runs, args.warmup))
    walk = ctx.synth(Cn, T, seed=1234, S=50)
    v = torch.empty((T, Cn), dtype=torch.float32, device="cuda")
    x_ct = torch.empty((Cn, T), dtype=torch.float32, device="cuda")
    back = torch.empty((T, Cn), dtype=torch.float32, device="cuda")
    for vs in [int(s) for s in args.sizes.split(",")]:
        top = min((1 << (vs - 1)) - 2, 60000)  # centi-units that Normalize accepts at this value size
        for t0 in range(0, T, 4096):
            v[t0:t0 + 4096] = (walk[t0:t0 + 4096] % top).to(torch.float32) / 100.0
        cap = dca.axdr_bytes(T, vs)
        slabs = torch.zeros((Cn, cap), dtype=torch.uint8, device="cuda")
        # verified first
        _, bits, err = ctx.axdr_encode(v, vs, out=slabs)
        _, count, derr = ctx.axdr_decode(slabs, bits, T, vs, out=back)
        torch.cuda.synchronize()
        assert int((err != 0).sum()) == 0 and int((derr != 0).sum()) == 0 and bool((bits == T * vs).all()) and bool((count == T).all())
        if vs <= 32:
            x, nerr = ctx.normalize(v, valuesize=vs)
            assert int((nerr != 0).sum()) == 0 and torch.equal(ctx.denormalize(x, valuesize=vs).view(torch.int32), back.view(torch.int32)), "round trip"
            del x
        for c in (0, 1, 63, 64, Cn // 2 + 5, Cn - 1):
            r, data, n = orc.stage("normalize", True, v[:, c].contiguous().cpu().numpy().tobytes(), 32 * T, valuesize=vs)
            assert r == 0 and n == T * vs and slabs[c, : (n + 7) // 8].cpu().numpy().tobytes() == data[: (n + 7) // 8], ("oracle", vs, c)
        cands = {
            "to_channel_major, 4-byte (the yardstick)": lambda: ctx.to_channel_major(v, out=x_ct),
            "pack   vs %2d" % vs: lambda: ctx.axdr_encode(v, vs, out=slabs),
            "unpack vs %2d" % vs: lambda: ctx.axdr_decode(slabs, bits, T, vs, out=back),
        }
        for _ in range(args.warmup):
            for fn in cands.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in cands}
        for _ in range(args.runs):
            for k, fn in cands.items():
                ms[k].append(event_ms(fn))
        got = {k: spread(m) for k, m in ms.items()}
        say("value size %d: %d bytes a slab, %.1f GB of streams" % (vs, cap, Cn * cap / 1e9))
        yard = None
        res = {}
        for k, sp in got.items():
            moved = Cn * T * (8.0 if yard is None else 4.0 + vs / 8.0)
            tbs = moved / (sp["median_ms"] * 1e-3) / 1e12
            extra = ""
            if yard is None:
                yard = sp
                extra = "  spread (slowest - fastest) / median %.3f" % ((sp["slowest_ms"] - sp["fastest_ms"]) / sp["median_ms"])
            else:
                extra = "  %.3f of the transposition's time, %.3f of its time per byte" % (sp["median_ms"] / yard["median_ms"],
                                                                                          sp["median_ms"] / yard["median_ms"] * 8.0 / (4.0 + vs / 8.0))
            say("  %-42s median %8.3f ms (fastest %8.3f, p90 %8.3f, slowest %8.3f)  %.2f TB/s, %.2f of the HBM peak%s"
                % (k, sp["median_ms"], sp["fastest_ms"], sp["p90_ms"], sp["slowest_ms"], tbs, tbs / HBM_PEAK_TBS, extra))
            res[k.strip()] = dict(sp, tbs=round(tbs, 3), of_peak=round(tbs / HBM_PEAK_TBS, 3), of_yardstick=round(sp["median_ms"] / yard["median_ms"], 3))
        results["vs%d" % vs] = res
        del slabs, cands
        torch.cuda.empty_cache()
    say(json.dumps(results))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
