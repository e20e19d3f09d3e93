#!/usr/bin/env python3
"""Times the counted entry points (ragged batches: a count per channel) against their uniform twins on one batch of float32
readings resident on the device, and writes profiles/ragged_bench.txt.

    python tools/raggedbench.py [--channels 65536] [--samples 86400] [--levels 60 300 900 3600] [--runs 20] [--warmup 3]

Three distributions of the counts: all equal to T; uniform in [0.9 T, T]; one channel in 64 at T / 2 (one early lane per
wave), the others at T.  Per distribution:
  (a) dega_hip_aggregate_levels_var_dev against dega_hip_aggregate_levels_dev at the level set,
  (b) dega_hip_encode_f32_var_dev against dega_hip_encode_f32_dev (adaptive, valuesize 32),
  (c) dega_hip_csv_write_var_dev against dega_hip_csv_write_dev (two decimals),
  (d) dega_hip_encode_var_dev against dega_hip_encode_dev on the same readings normalized to int32 (adaptive, valuesize 32),
  (e) the counted host job against the uniform one (encode_job with and without count=) on --job-channels x --job-samples of
      those int32 samples in pageable host memory: wall clock around the whole call, the two alternating.
--parts picks among float (a, b), csv (c), int (d), job (e); default: all of them.
The uniform twin always runs over all T rows -- it has no other way to take the batch -- so for the ragged distributions it
does MORE work than the counted call; the like-for-like comparison is the first distribution.
hipEvents on the stream the launches use (torch.cuda.Event is one), warm-up runs, then the two candidates alternating run
by run in one session; medians with the fastest, the 90th percentile and the slowest run.  Outputs are verified before
anything is timed: with all counts equal to T the counted call must return the uniform call's bits, lengths and statuses
for every channel and its bytes for a sample of them; with ragged counts a sample of channels is compared with the uniform
call on that channel alone, cut to its count."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.aggbench import COPY_TBS, event_ms, readings, spread  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=65536)
    ap.add_argument("--samples", type=int, default=86400)
    ap.add_argument("--levels", type=int, nargs="+", default=[60, 300, 900, 3600])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bytes-per-value", type=int, default=9, help="text stride = samples x this (meter readings need about 8)")
    ap.add_argument("--parts", nargs="+", default=["float", "csv", "int", "job"], choices=["float", "csv", "int", "job"])
    ap.add_argument("--job-channels", type=int, default=8192)
    ap.add_argument("--job-samples", type=int, default=10800)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_bench.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from __graft_entry__ import load_package
    dca = load_package()
    L = dca.library()
    ctx = dca.Context(0)
    Cn, T, Ns = args.channels, args.samples, args.levels
    K = len(Ns)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    v = readings(ctx, Cn, T)
    s = ctx._stream()
    rng = np.random.default_rng(64)
    half = np.full(Cn, T, dtype=np.int64)
    lane = rng.integers(0, 64, (Cn + 63) // 64) + 64 * np.arange((Cn + 63) // 64)
    half[lane[lane < Cn]] = T // 2
    dists = [("all T", np.full(Cn, T, dtype=np.int64)), ("uniform in [0.9 T, T]", rng.integers(T - T // 10, T + 1, Cn).astype(np.int64)),
             ("one in 64 at T / 2", half)]
    sample = [int(c) for c in np.unique(np.concatenate([lane[:4], rng.integers(0, Cn, 8), [0, Cn - 1]]).clip(0, Cn - 1))]
    say("ragged batches, %d channels x %d float32 readings resident, levels %s; %d timed runs per candidate, alternating, %d warm-up runs; hipEvents"
        % (Cn, T, Ns, args.runs, args.warmup))

    rows = [L.dega_hip_aggregate_rows(T, N) for N in Ns]
    nv = (C.c_size_t * K)(*Ns)
    lds = (C.c_size_t * K)(*[Cn] * K)
    ptrs = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    a_uni = [torch.zeros((r, Cn), dtype=torch.float32, device="cuda") for r in rows]
    a_var = [torch.zeros((r, Cn), dtype=torch.float32, device="cuda") for r in rows]
    oc = [torch.zeros(Cn, dtype=torch.int64, device="cuda") for _ in range(K)]
    aerr = torch.zeros(Cn, dtype=torch.int32, device="cuda")
    cap = (4 * T + 64 + 3) & ~3
    e_uni = (torch.zeros((Cn, cap), dtype=torch.uint8, device="cuda"), torch.zeros(Cn, dtype=torch.int64, device="cuda"), torch.zeros(Cn, dtype=torch.int32, device="cuda"))
    e_var = (torch.zeros((Cn, cap), dtype=torch.uint8, device="cuda"), torch.zeros(Cn, dtype=torch.int64, device="cuda"), torch.zeros(Cn, dtype=torch.int32, device="cuda"))
    results = {"channels": Cn, "samples": T, "levels": Ns, "runs": args.runs, "warmup": args.warmup, "distributions": []}

    def alternate(uni, var):
        for _ in range(args.warmup):
            uni()
            var()
        torch.cuda.synchronize()
        u, w = [], []
        for _ in range(args.runs):
            u.append(event_ms(uni))
            w.append(event_ms(var))
        return spread(u), spread(w)

    def report(what, u, w, extra=""):
        say("  %-26s uniform median %9.3f ms (fastest %9.3f, p90 %9.3f, slowest %9.3f) | counted median %9.3f ms (fastest %9.3f, p90 %9.3f, slowest %9.3f) | counted / uniform %.3f%s"
            % (what, u["median_ms"], u["fastest_ms"], u["p90_ms"], u["slowest_ms"], w["median_ms"], w["fastest_ms"], w["p90_ms"], w["slowest_ms"],
               w["median_ms"] / u["median_ms"], extra))

    def int_parts(name, count, res):
        """(d) and (e): integer samples, on the device and through the host job"""
        import time
        cd = torch.from_numpy(count).cuda()
        equal = bool((count == T).all())
        if "int" in args.parts:
            x, nerr = ctx.normalize(v, 100.0, 32)
            torch.cuda.synchronize()
            assert int((nerr != 0).sum().item()) == 0
            i_uni = (torch.zeros((Cn, cap), dtype=torch.uint8, device="cuda"), torch.zeros(Cn, dtype=torch.int64, device="cuda"), torch.zeros(Cn, dtype=torch.int32, device="cuda"))
            i_var = (torch.zeros((Cn, cap), dtype=torch.uint8, device="cuda"), torch.zeros(Cn, dtype=torch.int64, device="cuda"), torch.zeros(Cn, dtype=torch.int32, device="cuda"))

            def int_uni():
                assert L.dega_hip_encode_dev(ctx._h, x.data_ptr(), Cn, T, Cn, 1, 32, i_uni[0].data_ptr(), cap, i_uni[1].data_ptr(), i_uni[2].data_ptr(), s) == 0

            def int_var():
                assert L.dega_hip_encode_var_dev(ctx._h, x.data_ptr(), Cn, T, Cn, cd.data_ptr(), 1, 32, dca.SAMPLES_I32, i_var[0].data_ptr(), cap, i_var[1].data_ptr(),
                                                 i_var[2].data_ptr(), s) == 0
            int_uni()
            int_var()
            torch.cuda.synchronize()
            assert int((i_var[2] != 0).sum().item()) == 0 and int((i_uni[2] != 0).sum().item()) == 0
            if equal:
                assert torch.equal(i_uni[1], i_var[1])
            for c in sample:
                n = int(count[c])
                o, b, e = ctx.encode(x[:n, c : c + 1].contiguous(), 1)
                torch.cuda.synchronize()
                nb = (int(b[0].item()) + 7) // 8
                assert int(b[0].item()) == int(i_var[1][c].item()) and torch.equal(o[0, :nb], i_var[0][c, :nb]), c
            u, w = alternate(int_uni, int_var)
            report("encode int32 (32, adaptive)", u, w, "; counted: %.1f Gsamples/s of the samples below the counts" % (float(count.sum()) / (w["median_ms"] * 1e-3) / 1e9))
            res["encode_i32"] = {"uniform": u, "counted": w}
            del i_uni, i_var, x
        if "job" in args.parts:
            jc, jt = min(args.job_channels, Cn), min(args.job_samples, T)
            xh = ctx.normalize(v[:jt, :jc].contiguous(), 100.0, 32)[0].cpu().numpy()
            jcount = np.minimum(count[:jc] * jt // T, jt).astype(np.uint64)  # the same distribution at the job's length

            def wall(f):
                t0 = time.perf_counter()
                r = f()
                return (time.perf_counter() - t0) * 1e3, r
            job_uni = lambda: ctx.encode_job(xh)  # noqa: E731
            job_var = lambda: ctx.encode_job(xh, count=jcount)  # noqa: E731
            ru, rw = job_uni(), job_var()
            assert int((rw[3] != 0).sum()) == 0
            if equal:
                assert all(a.tobytes() == b.tobytes() for a, b in zip(ru, rw))
            for _ in range(args.warmup):
                job_uni()
                job_var()
            tu, tw = [], []
            for _ in range(args.runs):
                tu.append(wall(job_uni)[0])
                tw.append(wall(job_var)[0])
            u, w = spread(tu), spread(tw)
            report("encode_job int32 %dx%d" % (jc, jt), u, w, "; wall clock, pageable; counted: %.2f Gsamples/s of the samples below the counts"
                   % (float(jcount.sum()) / (w["median_ms"] * 1e-3) / 1e9))
            res["encode_job_i32"] = {"uniform": u, "counted": w, "channels": jc, "samples": jt}

    for name, count in dists:
        cd = torch.from_numpy(count).cuda()
        res = {"counts": name, "mean_count": float(count.mean()), "min_count": int(count.min())}
        say("counts %s: mean %.1f, smallest %d" % (name, count.mean(), count.min()))
        equal = bool((count == T).all())
        int_parts(name, count, res)
        if "float" not in args.parts:
            results["distributions"].append(res)
            continue

        # ---- (a) aggregate ----
        def agg_uni():
            assert L.dega_hip_aggregate_levels_dev(ctx._h, v.data_ptr(), Cn, T, Cn, nv, K, ptrs(a_uni), lds, s) == 0

        def agg_var():
            assert L.dega_hip_aggregate_levels_var_dev(ctx._h, v.data_ptr(), Cn, T, Cn, cd.data_ptr(), nv, K, ptrs(a_var), lds, ptrs(oc), aerr.data_ptr(), s) == 0
        agg_uni()
        agg_var()
        torch.cuda.synchronize()
        assert int((aerr != 0).sum().item()) == 0
        for k, N in enumerate(Ns):
            assert bool((oc[k] == (cd + (N - 1)) // N).all()), N
            if equal:
                assert torch.equal(a_uni[k].view(torch.int32), a_var[k].view(torch.int32)), N
            for c in sample:
                n = int(count[c])
                alone = ctx.aggregate(v[:n, c : c + 1].contiguous(), N)
                torch.cuda.synchronize()
                assert torch.equal(alone[:, 0].contiguous().view(torch.int32), a_var[k][: alone.shape[0], c].contiguous().view(torch.int32)), (N, c)
        u, w = alternate(agg_uni, agg_var)
        moved_uni = 4.0 * Cn * (T + sum(rows))
        moved_var = 4.0 * (float(count.sum()) + sum(float((-(-count // N)).sum()) for N in Ns))
        report("aggregate, %d levels" % K, u, w, "; counted: %.0f GB/s of the rows below the counts read + sums written (%.2f of the %.2f TB/s copy figure); uniform: %.0f GB/s"
               % (moved_var / (w["median_ms"] * 1e-3) / 1e9, moved_var / (w["median_ms"] * 1e-3) / 1e12 / COPY_TBS, COPY_TBS, moved_uni / (u["median_ms"] * 1e-3) / 1e9))
        res["aggregate"] = {"uniform": u, "counted": w}

        # ---- (b) the DEGA float entry ----
        def enc_uni():
            assert L.dega_hip_encode_f32_dev(ctx._h, v.data_ptr(), Cn, T, Cn, 100.0, 1, 32, e_uni[0].data_ptr(), cap, e_uni[1].data_ptr(), e_uni[2].data_ptr(), s) == 0

        def enc_var():
            assert L.dega_hip_encode_f32_var_dev(ctx._h, v.data_ptr(), Cn, T, Cn, cd.data_ptr(), 100.0, 1, 32, e_var[0].data_ptr(), cap, e_var[1].data_ptr(),
                                                 e_var[2].data_ptr(), s) == 0
        enc_uni()
        enc_var()
        torch.cuda.synchronize()
        assert int((e_var[2] != 0).sum().item()) == 0 and int((e_uni[2] != 0).sum().item()) == 0
        if equal:
            assert torch.equal(e_uni[1], e_var[1])
        for c in sample:
            n = int(count[c])
            o, b, e = ctx.encode_f32(v[:n, c : c + 1].contiguous(), 100.0, 1)
            torch.cuda.synchronize()
            nb = (int(b[0].item()) + 7) // 8
            assert int(b[0].item()) == int(e_var[1][c].item()) and torch.equal(o[0, :nb], e_var[0][c, :nb]), c
        u, w = alternate(enc_uni, enc_var)
        report("encode_f32 (32, adaptive)", u, w, "; counted: %.1f Gsamples/s of the samples below the counts" % (float(count.sum()) / (w["median_ms"] * 1e-3) / 1e9))
        res["encode_f32"] = {"uniform": u, "counted": w, "stream_bytes_counted": int(((e_var[1] + 7) // 8).sum().item())}
        results["distributions"].append(res)

    # ---- (c) the writer: its text needs the room the encoder's slabs had ----
    del e_uni, e_var, a_uni, a_var
    torch.cuda.empty_cache()
    if "csv" not in args.parts:
        dists = []
    stride = (T * args.bytes_per_value + 16 + 15) // 16 * 16
    t_uni = (torch.zeros((Cn, stride), dtype=torch.uint8, device="cuda"), torch.zeros(Cn, dtype=torch.int64, device="cuda"), torch.zeros(Cn, dtype=torch.int32, device="cuda"))
    t_var = (torch.zeros((Cn, stride), dtype=torch.uint8, device="cuda"), torch.zeros(Cn, dtype=torch.int64, device="cuda"), torch.zeros(Cn, dtype=torch.int32, device="cuda"))
    for (name, count), res in zip(dists, results["distributions"]):
        cd = torch.from_numpy(count).cuda()
        equal = bool((count == T).all())

        def csv_uni():
            assert L.dega_hip_csv_write_dev(ctx._h, v.data_ptr(), Cn, T, Cn, 2, 1, 44, t_uni[0].data_ptr(), stride, t_uni[1].data_ptr(), t_uni[2].data_ptr(), s) == 0

        def csv_var():
            assert L.dega_hip_csv_write_var_dev(ctx._h, v.data_ptr(), Cn, T, Cn, cd.data_ptr(), 2, 1, 44, t_var[0].data_ptr(), stride, t_var[1].data_ptr(),
                                                t_var[2].data_ptr(), s) == 0
        csv_uni()
        csv_var()
        torch.cuda.synchronize()
        assert int((t_var[2] != 0).sum().item()) == 0 and int((t_uni[2] != 0).sum().item()) == 0
        if equal:
            assert torch.equal(t_uni[1], t_var[1])
        for c in sample:
            n = int(count[c])
            text, lens, err = ctx.csv_write(v[:n, c : c + 1].contiguous(), stride=stride)
            torch.cuda.synchronize()
            m = int(lens[0].item())
            assert m == int(t_var[1][c].item()) and torch.equal(text[0, :m], t_var[0][c, :m]), c
        u, w = alternate(csv_uni, csv_var)
        say("counts %s:" % name)
        report("csv_write (2 decimals)", u, w, "; counted: %.1f Gvalues/s" % (float(count.sum()) / (w["median_ms"] * 1e-3) / 1e9))
        res["csv_write"] = {"uniform": u, "counted": w, "text_bytes_counted": int(t_var[1].sum().item())}
    say(json.dumps(results))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
