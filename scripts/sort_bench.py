#!/usr/bin/env python3
"""ORDER BY (RJ_NODE_SORT) over one relation of 100 M rows, Page-packed and resident in HBM, result
Page images left in HBM (as bench.py): a sort key and an INT64 payload, `SELECT key, payload ORDER BY
key`, as Scan -> RJ_NODE_SORT.

  full32    INT32 keys over the whole range                       4 passes
  small32   INT32 keys in [0, 200)                                1 pass  (the skip rule)
  full64    INT64 keys over the whole range                       8 passes
  two-key   ORDER BY small32, full32                              4 + 1 passes
  limit10   full32 with LIMIT 10                                  4 passes, 10 rows gathered

Per case: wall time of rj_execute_resident (best / median over the steps), the k_sort_scatter launches
(the launch log), and from one more execution on a profiling context (rj_profile_read: the dispatch
timestamps of every kernel) the time of the sort kernels and the achieved bytes/s of k_sort_scatter:
per pass and row it reads the key (4 or 8 B) and, from the second pass on, the row id (4 B), and writes
the row id and, unless the pass is the column's last, the key.  The yardstick beside that figure is the
hashed partition pass (pass1_scatter, 4.2-4.6 TB/s, profiles/r03_zz_config3_final.md), which may write
a digit's rows in any order.

    python scripts/sort_bench.py [--steps 5] [--warmup 1] [--rows 100000000]
    rocprofv3 --kernel-trace --stats --output-format csv -- python3 scripts/sort_bench.py --only full32 --steps 2
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "radix-join_amd"))

CASES = ("full32", "small32", "full64", "two-key", "limit10")


def scatter_bytes(rows, columns):
    """columns: [(key bytes, passes)] in the order they are sorted (last key first) -> bytes k_sort_scatter moves"""
    total, first = 0, True
    for width, passes in columns:
        for q in range(passes):
            total += rows * (width + (0 if first else 4) + 4 + (width if q + 1 < passes else 0))
            first = False
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--only", choices=CASES, help="this case only, no profiling context (a profiler's run)")
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("sort_bench.py needs a GPU: it measures the HIP path only")
    from pyrj import capi
    from pyrj import plan as pl
    from pyrj import workloads as wl

    I32, I64 = pl.INT32, pl.INT64
    rows = a.rows
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(29)
    ctx = capi.Context(device=0)
    pctx = None if a.only else capi.Context(device=0, profile=2)  # 2: every launch is timed
    d = ctx.device_info()
    print(json.dumps({"device": d["name"], "arch": d["arch"], "compute_units": d["compute_units"], "rows": rows}), flush=True)

    def plan_of(types, keys, limit=None):
        p = pl.Plan()
        s = p.new_scan_node(0, list(enumerate(types)))
        p.root = p.new_sort_node(s, keys, [(keys[0][0], types[keys[0][0]]), (len(types) - 1, I64)], limit)
        return p

    v = torch.randint(-(2**40), 2**40, (rows,), device=dev, generator=gen, dtype=torch.int64)
    k32 = torch.randint(-(2**31), 2**31, (rows,), device=dev, generator=gen, dtype=torch.int32)
    small = torch.randint(0, 200, (rows,), device=dev, generator=gen, dtype=torch.int32)
    k64 = torch.randint(-(2**63), 2**63 - 1, (rows,), device=dev, generator=gen, dtype=torch.int64)
    # case -> (columns, plan, [(key bytes, passes)] in sorting order)
    setups = {
        "full32": ([k32, v], plan_of([I32, I64], [(0, 0)]), [(4, 4)]),
        "small32": ([small, v], plan_of([I32, I64], [(0, 0)]), [(4, 1)]),
        "full64": ([k64, v], plan_of([I64, I64], [(0, 0)]), [(8, 8)]),
        "two-key": ([small, k32, v], plan_of([I32, I32, I64], [(0, 0), (1, 0)]), [(4, 4), (4, 1)]),
        "limit10": ([k32, v], plan_of([I32, I64], [(0, 0)], limit=10), [(4, 4)]),
    }
    for name in CASES if a.only is None else (a.only,):
        cols, plan, columns = setups[name]
        T = wl.adopt(ctx, cols)
        times, out_rows = [], 0
        ctx.launch_log(True)
        for i in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = ctx.execute_resident(plan, [T])
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            out_rows = res.num_rows
            res.free()
            if i >= a.warmup:
                times.append(dt)
        ran = ctx.launches()
        ctx.launch_log(False)
        T.release()
        runs = a.warmup + a.steps
        passes = sum(n for k, n in ran.items() if "k_sort_scatter" in k) // runs
        rec = {"case": name, "out_rows": out_rows, "best_ms": round(min(times), 3), "median_ms": round(statistics.median(times), 3),
               "scatter_passes": passes, "expected_passes": sum(p for _, p in columns)}
        if pctx is not None:
            P = wl.adopt(pctx, cols)
            pctx.execute_resident(plan, [P]).free()
            pctx.profile_reset()
            pctx.execute_resident(plan, [P]).free()
            torch.cuda.synchronize()
            prof = {r["name"]: r for r in pctx.profile()}
            P.release()
            for kname in ("sort_encode", "sort_count", "sort_scan", "sort_scatter", "gather"):
                if kname in prof:
                    rec[f"{kname}_ms"] = round(prof[kname]["total_ms"], 3)
            if prof.get("sort_scatter", {}).get("total_ms"):
                moved = scatter_bytes(rows, columns)
                rec["scatter_GB"] = round(moved / 1e9, 2)
                rec["scatter_TB_per_s"] = round(moved / (prof["sort_scatter"]["total_ms"] * 1e-3) / 1e12, 3)
        print(json.dumps(rec), flush=True)
        torch.cuda.empty_cache()
    if pctx is not None:
        pctx.destroy()
    ctx.destroy()


if __name__ == "__main__":
    main()
