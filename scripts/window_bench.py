#!/usr/bin/env python3
"""Window functions (RJ_NODE_WINDOW) next to the sort they contain.

One relation of 100 M rows, Page-packed and resident in HBM, result Page images left in HBM (as
bench.py): an INT32 partition key p with 10^4 uniform values, an INT32 order key o over the whole
range, an INT64 value v.  Every case passes the key columns it uses and v through.  One JSON line per
case: wall time of rj_execute_resident (best / median over the steps) of the window node and, in the
same process, of its yardstick, and from one more execution of each on a profiling context (level 2:
the dispatch timestamps of every kernel) the time per kernel family.

  ranks     ROW_NUMBER, RANK, DENSE_RANK OVER (PARTITION BY p ORDER BY o)
  running   the same keys: COUNT(*), SUM(v), MIN(v), MAX(v), running (the default frame)
  totals    OVER (PARTITION BY p): the same aggregates, the partition's total on every row
  nokey     OVER (): SUM(v).  The contract's frame without an order key is the whole partition, so every
            row gets the total; the rows stay in the scan's order and nothing is sorted
  yardstick: RJ_NODE_SORT at the root over the same keys with the same passed-through columns — the
            price of ordering and gathering, which the window node pays too.  window - sort is what
            the k_win_* kernels (and k_group_heads) cost.
  The aggregate cases also run RJ_NODE_GROUP BY p with SUM / MIN / MAX of v on the profiling context:
  its k_group_reduce is what one reduction of the same column through the same kind of permutation takes.

    python scripts/window_bench.py [--steps 5] [--warmup 1] [--rows 100000000] [--only NAME]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "radix-join_amd"))

CASES = ("ranks", "running", "totals", "nokey")
WIN_KERNELS = ("win_one_head", "win_marks", "win_carry", "win_ranks", "win_tails", "win_tail_carry", "win_scan", "win_column")
OTHER_KERNELS = ("group_heads", "sort_encode", "sort_count", "sort_scan", "sort_scatter", "gather", "finish_pages", "encode_nullable")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--only", choices=CASES, help="this case only, no profiling context (a profiler's run)")
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("window_bench.py needs a GPU: it measures the HIP path only")
    from pyrj import capi
    from pyrj import plan as pl
    from pyrj import workloads as wl

    I32, I64 = pl.INT32, pl.INT64
    rows = a.rows
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(37)
    ctx = capi.Context(device=0)
    pctx = None if a.only else capi.Context(device=0, profile=2)  # 2: every launch is timed
    d = ctx.device_info()
    print(json.dumps({"device": d["name"], "arch": d["arch"], "compute_units": d["compute_units"], "rows": rows,
                      "steps": a.steps, "warmup": a.warmup}), flush=True)
    TYPES = [I32, I32, I64]
    RANKS = [(pl.WIN_ROW_NUMBER, 0, I64), (pl.WIN_RANK, 0, I64), (pl.WIN_DENSE_RANK, 0, I64)]
    AGGS = [(pl.WIN_COUNT_STAR, 0, I64), (pl.WIN_SUM, 2, I64), (pl.WIN_MIN, 2, I64), (pl.WIN_MAX, 2, I64)]
    SHAPES = {  # partition keys, order keys, functions
        "ranks": ([(0, 0)], [(1, 0)], RANKS),
        "running": ([(0, 0)], [(1, 0)], AGGS),
        "totals": ([(0, 0)], [], AGGS),
        "nokey": ([], [], [(pl.WIN_SUM, 2, I64)]),
    }

    def scan(p):
        return p.new_scan_node(0, list(enumerate(TYPES)))

    def passed(part, order):
        return sorted({c for c, _ in part + order} | {2})

    def window_plan(part, order, funcs):
        p = pl.Plan()
        p.root = p.new_window_node(scan(p), part, order, [(pl.WIN_COL, c, TYPES[c]) for c in passed(part, order)] + funcs)
        return p

    def sort_plan(part, order):
        p = pl.Plan()
        p.root = p.new_sort_node(scan(p), part + order, [(c, TYPES[c]) for c in passed(part, order)])
        return p

    def group_plan():
        p = pl.Plan()
        p.root = p.new_group_node(scan(p), [(0, 0)], [(pl.AGG_KEY, 0, I32), (pl.AGG_SUM, 2, I64), (pl.AGG_MIN, 2, I64), (pl.AGG_MAX, 2, I64)])
        return p

    def adopt(c, cols):
        pages = [wl.pack_pages_gpu64(t) if t.element_size() == 8 else wl.pack_pages_gpu(t) for t in cols]
        torch.cuda.synchronize()
        return c.adopt_device(cols[0].numel(), TYPES, [p.data_ptr() for p in pages], [p.shape[0] for p in pages], keep=pages)

    def timed(c, plan, tables):
        times, out_rows = [], 0
        for i in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = c.execute_resident(plan, tables)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            out_rows = res.num_rows
            res.free()
            if i >= a.warmup:
                times.append(dt)
        return round(min(times), 3), round(statistics.median(times), 3), out_rows

    def kernels(plan, P):
        """kernel family -> ms of ONE execution on the profiling context"""
        pctx.execute_resident(plan, [P]).free()
        pctx.profile_reset()
        pctx.execute_resident(plan, [P]).free()
        torch.cuda.synchronize()
        return {r["name"]: round(r["total_ms"], 3) for r in pctx.profile()}

    cols = [torch.randint(0, 10_000, (rows,), device=dev, generator=gen, dtype=torch.int32),
            torch.randint(-(2**31), 2**31, (rows,), device=dev, generator=gen, dtype=torch.int32),
            torch.randint(-(2**40), 2**40, (rows,), device=dev, generator=gen, dtype=torch.int64)]
    T = adopt(ctx, cols)
    P = adopt(pctx, cols) if pctx is not None else None
    for name in CASES if a.only is None else (a.only,):
        part, order, funcs = SHAPES[name]
        rec = {"case": name}
        wplan, splan = window_plan(part, order, funcs), sort_plan(part, order)
        rec["window_best_ms"], rec["window_median_ms"], out_rows = timed(ctx, wplan, [T])
        assert out_rows == rows
        rec["sort_best_ms"], rec["sort_median_ms"], _ = timed(ctx, splan, [T])
        rec["window_minus_sort_ms"] = round(rec["window_best_ms"] - rec["sort_best_ms"], 3)
        if pctx is not None:
            prof = kernels(wplan, P)
            rec["window_kernels_ms"] = {k: prof[k] for k in WIN_KERNELS + OTHER_KERNELS if k in prof}
            rec["win_kernels_total_ms"] = round(sum(prof.get(k, 0.0) for k in WIN_KERNELS), 3)
            sprof = kernels(splan, P)
            rec["sort_kernels_ms"] = {k: t for k, t in sprof.items() if k in OTHER_KERNELS}
            if name in ("running", "totals"):
                gprof = kernels(group_plan(), P)
                rec["group_reduce_same_column_ms"] = gprof.get("group_reduce")
                rec["group_heads_one_key_ms"] = gprof.get("group_heads")
        print(json.dumps(rec), flush=True)
    T.release()
    if P is not None:
        P.release()
        pctx.destroy()
    ctx.destroy()


if __name__ == "__main__":
    main()
