#!/usr/bin/env python3
"""ROWS frames and LAG of RJ_NODE_WINDOW next to the default-frame node they extend.

One relation of 16 M rows, Page-packed and resident in HBM, result Page images left in HBM (as
bench.py): an INT32 partition key p with rows / 1000 uniform values (partitions of about 1 000 rows),
an INT32 order key o over the whole range, an INT64 value v.  Every case is ONE window node OVER
(PARTITION BY p ORDER BY o) that passes p, o and v through and adds one function:

  default_sum     SUM(v) under the default frame: the node without the frame layer, the yardstick
  rows_sum_6      SUM(v)  ROWS BETWEEN 6 PRECEDING AND CURRENT ROW
  rows_min_6      MIN(v)  ROWS BETWEEN 6 PRECEDING AND CURRENT ROW
  rows_min_1000   MIN(v)  ROWS BETWEEN 1000 PRECEDING AND CURRENT ROW
  lag_1           LAG(v, 1)
  two_frames      SUM(v) and MIN(v) under 6 PRECEDING and under 29 PRECEDING: four functions, one ordering

The cases are timed in turns (case 1, case 2, ... case 1, case 2, ...), so that what else the machine
does hits all of them alike.  One JSON line per case: wall time of rj_execute_resident (best, median,
worst over the steps), the median's difference to default_sum, and from one more execution on a
profiling context (level 2: the dispatch timestamps of every kernel) the time per kernel family.

    python scripts/frame_bench.py [--steps 10] [--warmup 2] [--rows 16000000]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "radix-join_amd"))

FRAME_KERNELS = ("frame_pick", "frame_ntile", "frame_sum", "frame_leaves", "frame_levels", "frame_extreme")
WIN_KERNELS = ("win_marks", "win_carry", "win_ranks", "win_tails", "win_tail_carry", "win_scan", "win_column")
OTHER_KERNELS = ("group_heads", "sort_encode", "sort_count", "sort_scan", "sort_scatter", "gather", "finish_pages", "encode_nullable")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=16_000_000)
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("frame_bench.py needs a GPU: it measures the HIP path only")
    from pyrj import capi
    from pyrj import plan as pl
    from pyrj import workloads as wl

    I32, I64 = pl.INT32, pl.INT64
    rows = a.rows
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(41)
    ctx = capi.Context(device=0)
    pctx = capi.Context(device=0, profile=2)  # 2: every launch is timed
    d = ctx.device_info()
    print(json.dumps({"device": d["name"], "arch": d["arch"], "compute_units": d["compute_units"], "rows": rows,
                      "partitions": max(1, rows // 1000), "steps": a.steps, "warmup": a.warmup}), flush=True)
    TYPES = [I32, I32, I64]
    CASES = {
        "default_sum": [(pl.WIN_SUM, 2, I64)],
        "rows_sum_6": [(pl.WIN_ROWS_SUM, 2, I64, -6, 0)],
        "rows_min_6": [(pl.WIN_ROWS_MIN, 2, I64, -6, 0)],
        "rows_min_1000": [(pl.WIN_ROWS_MIN, 2, I64, -1000, 0)],
        "lag_1": [(pl.WIN_LAG, 2, I64, 1, 0)],
        "two_frames": [(pl.WIN_ROWS_SUM, 2, I64, -6, 0), (pl.WIN_ROWS_SUM, 2, I64, -29, 0), (pl.WIN_ROWS_MIN, 2, I64, -6, 0),
                       (pl.WIN_ROWS_MIN, 2, I64, -29, 0)],
    }

    def window_plan(funcs):
        p = pl.Plan()
        sc = p.new_scan_node(0, list(enumerate(TYPES)))
        p.root = p.new_window_node(sc, [(0, 0)], [(1, 0)], [(pl.WIN_COL, c, TYPES[c]) for c in range(3)] + funcs)
        return p

    def adopt(c, cols):
        pages = [wl.pack_pages_gpu64(t) if t.element_size() == 8 else wl.pack_pages_gpu(t) for t in cols]
        torch.cuda.synchronize()
        return c.adopt_device(cols[0].numel(), TYPES, [p.data_ptr() for p in pages], [p.shape[0] for p in pages], keep=pages)

    def once(c, plan, tables):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = c.execute_resident(plan, tables)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        assert res.num_rows == rows
        res.free()
        return dt

    def kernels(plan, P):
        """kernel family -> ms of ONE execution on the profiling context"""
        pctx.execute_resident(plan, [P]).free()
        pctx.profile_reset()
        pctx.execute_resident(plan, [P]).free()
        torch.cuda.synchronize()
        return {r["name"]: round(r["total_ms"], 3) for r in pctx.profile()}

    cols = [torch.randint(0, max(1, rows // 1000), (rows,), device=dev, generator=gen, dtype=torch.int32),
            torch.randint(-(2**31), 2**31, (rows,), device=dev, generator=gen, dtype=torch.int32),
            torch.randint(-(2**40), 2**40, (rows,), device=dev, generator=gen, dtype=torch.int64)]
    T, P = adopt(ctx, cols), adopt(pctx, cols)
    plans = {name: window_plan(funcs) for name, funcs in CASES.items()}
    times = {name: [] for name in CASES}
    for step in range(a.warmup + a.steps):
        for name, plan in plans.items():
            dt = once(ctx, plan, [T])
            if step >= a.warmup:
                times[name].append(dt)
    base = statistics.median(times["default_sum"])
    for name, plan in plans.items():
        t = times[name]
        rec = {"case": name, "best_ms": round(min(t), 3), "median_ms": round(statistics.median(t), 3), "worst_ms": round(max(t), 3),
               "median_minus_default_sum_ms": round(statistics.median(t) - base, 3)}
        prof = kernels(plan, P)
        rec["kernels_ms"] = {k: prof[k] for k in FRAME_KERNELS + WIN_KERNELS + OTHER_KERNELS if k in prof}
        rec["frame_kernels_total_ms"] = round(sum(prof.get(k, 0.0) for k in FRAME_KERNELS), 3)
        rec["win_kernels_total_ms"] = round(sum(prof.get(k, 0.0) for k in WIN_KERNELS), 3)
        print(json.dumps(rec), flush=True)
    T.release()
    P.release()
    pctx.destroy()
    ctx.destroy()


if __name__ == "__main__":
    main()
