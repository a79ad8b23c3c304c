#!/usr/bin/env python3
"""WHERE (RJ_NODE_SELECT) next to the one equivalent plan the library could run before the node
existed: the semi join of the table against a one-row filter side.

One relation of 100 M rows, Page-packed and resident in HBM, result Page images left in HBM (as
bench.py): an INT32 key and an INT64 payload.  `SELECT key, payload WHERE key = c` runs as
  select   Scan -> RJ_NODE_SELECT [key == c]                (k_select, then two k_gather)
  semi     Scan SEMI Scan({c})                               (k_filter_bcast: the broadcast path)
at selectivities 0.01, 0.5 and 1.0 (the fraction of rows whose key is c).  Both produce the same rows.
The two plans are timed with interleaved repetitions in one process (select, semi, select, ...), and the
whole measurement is repeated in several fresh processes: the spread between the processes' medians
is the yardstick for "not slower".  One line per (process, selectivity), then a table over the
processes with, for the node, the algorithmic bytes (4 B key read + 4 s B ids written,
then per output column 4 s B of ids read and width x s read and written) / best time / 8 TB/s.

    python scripts/select_bench.py [--steps 7] [--warmup 2] [--rows 100000000] [--procs 3]
    rocprofv3 --kernel-trace --stats --output-format csv -- python3 scripts/select_bench.py --child --selectivity 1.0
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "radix-join_amd"))

SELECTIVITIES = (0.01, 0.5, 1.0)
PEAK_BYTES_PER_S = 8e12
C_KEY = 7


def child(rows, steps, warmup, only=None):
    import torch

    from pyrj import capi
    from pyrj import plan as pl
    from pyrj import workloads as wl

    I32, I64 = pl.INT32, pl.INT64
    sel = pl.Plan()
    s = sel.new_scan_node(0, [(0, I32), (1, I64)])
    sel.root = sel.new_select_node(s, [("EQ", 0, C_KEY)], [(0, I32), (1, I64)])
    semi = pl.Plan()
    t = semi.new_scan_node(0, [(0, I32), (1, I64)])
    f = semi.new_scan_node(1, [(0, I32)])
    semi.root = semi.new_semi_join_node(False, t, f, 0, 0, [(0, I32), (1, I64)])  # the right child filters

    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    ctx = capi.Context(device=0)
    d = ctx.device_info()
    print(json.dumps({"device": d["name"], "arch": d["arch"], "compute_units": d["compute_units"]}), flush=True)
    F = wl.adopt(ctx, [torch.full((1,), C_KEY, device=dev, dtype=torch.int32)])
    for sv in SELECTIVITIES if only is None else (only,):
        gen.manual_seed(23)
        k = torch.randint(1000, 2**30, (rows,), device=dev, generator=gen, dtype=torch.int32)
        k[torch.rand(rows, device=dev, generator=gen) < sv] = C_KEY
        v = torch.randint(-(2**40), 2**40, (rows,), device=dev, generator=gen, dtype=torch.int64)
        T = wl.adopt(ctx, [k, v])
        del k, v
        torch.cuda.empty_cache()
        times = {"select": [], "semi": []}
        out = {}
        for i in range(warmup + steps):
            for name, plan, tables in (("select", sel, [T]), ("semi", semi, [T, F])):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = ctx.execute_resident(plan, tables)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                out[name] = res.num_rows
                res.free()
                if i >= warmup:
                    times[name].append(dt)
        assert out["select"] == out["semi"], out
        print(json.dumps({"selectivity": sv, "rows": rows, "out_rows": out["select"],
                          **{f"{n}_best_ms": round(min(ts), 3) for n, ts in times.items()},
                          **{f"{n}_median_ms": round(statistics.median(ts), 3) for n, ts in times.items()}}), flush=True)
        T.release()
        torch.cuda.empty_cache()
    F.release()
    ctx.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--selectivity", type=float, help="with --child: this selectivity only (a profiler's run)")
    a = ap.parse_args()
    if a.child:
        return child(a.rows, a.steps, a.warmup, a.selectivity)
    print(f"# rows={a.rows} steps={a.steps} warmup={a.warmup} processes={a.procs}", flush=True)
    runs = {sv: [] for sv in SELECTIVITIES}
    for p in range(a.procs):  # one fresh process after the other; the first failure ends the run
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--rows", str(a.rows), "--steps", str(a.steps),
                            "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            print(r.stdout + r.stderr, flush=True)
            sys.exit(f"process {p} ended with status {r.returncode}")
        for line in r.stdout.splitlines():
            rec = json.loads(line)
            print(f"process {p}: {line}", flush=True)
            if "selectivity" in rec:
                runs[rec["selectivity"]].append(rec)
    print("\n| selectivity | out rows | select best / median ms (per process) | semi best / median ms (per process) | "
          "process spread of the medians: select, semi | select / semi (medians of the process medians) | node: algorithmic GB, "
          "fraction of 8 TB/s at best |")
    print("|---|---|---|---|---|---|---|")
    for sv, recs in runs.items():
        col = lambda key: [r[key] for r in recs]
        pairs = lambda n: ", ".join(f"{b:.2f} / {m:.2f}" for b, m in zip(col(f"{n}_best_ms"), col(f"{n}_median_ms")))
        spread = lambda n: max(col(f"{n}_median_ms")) - min(col(f"{n}_median_ms"))
        ms, mf = statistics.median(col("select_median_ms")), statistics.median(col("semi_median_ms"))
        s_out = recs[0]["out_rows"] / recs[0]["rows"]
        algo = recs[0]["rows"] * (4.0 + 4.0 * s_out + (4.0 + 2 * 4.0) * s_out + (4.0 + 2 * 8.0) * s_out)
        best = min(col("select_best_ms"))
        print(f"| {sv} | {recs[0]['out_rows']} | {pairs('select')} | {pairs('semi')} | {spread('select'):.2f} ms, {spread('semi'):.2f} ms | "
              f"{ms / mf:.3f} ({ms - mf:+.2f} ms) | {algo / 1e9:.2f} GB, {algo / (best * 1e-3) / PEAK_BYTES_PER_S:.3f} |")


if __name__ == "__main__":
    main()
