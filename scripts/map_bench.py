#!/usr/bin/env python3
"""Computed columns (RJ_NODE_MAP): what k_map costs per row and per op.

One relation of 100 M rows, Page-packed and resident in HBM, result Page images left in HBM (as
bench.py): an INT32 key k with 10^4 uniform values, INT64 columns a, b, c, an FP64 column f.  One JSON
line per case: wall time of rj_execute_resident (best / median over the steps) and, from one more
execution on a profiling context (level 2: the dispatch timestamps of every kernel), the time per
kernel family; for k_map its algorithmic bytes (the columns it reads once + the arrays it writes) and
the bytes per second they make.

  abc        a * b + c -> INT64: 3 reads + 1 write = 32 bytes per row
  f_abc      f * f + f over the FP64 column: 1 read + 1 write = 16 bytes per row (three loads of one column)
  ops1       NEG(a): one operator over one column, 16 bytes per row
  ops32      NEG applied 32 times: the same bytes; (ops32 - ops1) / 31 is the interpreter's cost per op
  nullable   x * b + c where x is a NULLABLE column (dense values + validity bytes, made by a MAP below:
             CASE WHEN a % 8 = 0 THEN NULL ELSE a END); the figures are the upper MAP's alone (the profile
             of the lower MAP alone is subtracted): 3 reads + 1 validity read + 1 write + 1 validity write
             = 34 bytes per row
  sum_group  SUM(a * b) GROUP BY k as MAP + GROUP, next to the GROUP over a stored column

    python scripts/map_bench.py [--steps 5] [--warmup 1] [--rows 100000000]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "radix-join_amd"))

KERNELS = ("map", "gather", "finish_pages", "encode_nullable", "group_heads", "group_scan", "group_reduce", "group_keys", "group_column",
           "sort_encode", "sort_count", "sort_scan", "sort_scatter")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", type=int, default=100_000_000)
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("map_bench.py needs a GPU: it measures the HIP path only")
    from pyrj import capi
    from pyrj import plan as pl
    from pyrj import workloads as wl

    I32, I64, F64 = pl.INT32, pl.INT64, pl.FP64
    O = ("OUT",)
    rows = a.rows
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(41)
    ctx = capi.Context(device=0)
    pctx = capi.Context(device=0, profile=2)  # 2: every launch is timed
    d = ctx.device_info()
    print(json.dumps({"device": d["name"], "arch": d["arch"], "compute_units": d["compute_units"], "rows": rows,
                      "steps": a.steps, "warmup": a.warmup}), flush=True)
    TYPES = [I32, I64, I64, I64, F64]  # k, a, b, c, f

    def scan(p):
        return p.new_scan_node(0, list(enumerate(TYPES)))

    def map_plan(prog, outs, below=None):
        p = pl.Plan()
        child = scan(p) if below is None else below(p)
        p.root = p.new_map_node(child, prog, outs)
        return p

    def timed(c, plan, tables):
        times = []
        for i in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = c.execute_resident(plan, tables)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            assert res.num_rows == rows or plan.nodes[plan.root].data.__class__ is pl.GroupNode
            res.free()
            if i >= a.warmup:
                times.append(dt)
        return round(min(times), 3), round(statistics.median(times), 3)

    def kernels(plan, P):
        """kernel family -> ms of ONE execution on the profiling context"""
        pctx.execute_resident(plan, [P]).free()
        pctx.profile_reset()
        pctx.execute_resident(plan, [P]).free()
        torch.cuda.synchronize()
        return {r["name"]: round(r["total_ms"], 3) for r in pctx.profile()}

    cols = [torch.randint(0, 10_000, (rows,), device=dev, generator=gen, dtype=torch.int32)]
    cols += [torch.randint(-(2**40), 2**40, (rows,), device=dev, generator=gen, dtype=torch.int64) for _ in range(3)]
    cols.append(torch.randn((rows,), device=dev, generator=gen, dtype=torch.float64).view(torch.int64))
    pages = [wl.pack_pages_gpu64(t) if t.element_size() == 8 else wl.pack_pages_gpu(t) for t in cols]
    torch.cuda.synchronize()
    del cols
    adopt = lambda c: c.adopt_device(rows, TYPES, [p.data_ptr() for p in pages], [p.shape[0] for p in pages], keep=pages)
    T, P = adopt(ctx), adopt(pctx)

    def report(name, plan, map_bytes_per_row, minus=None):
        rec = {"case": name}
        rec["best_ms"], rec["median_ms"] = timed(ctx, plan, [T])
        prof = kernels(plan, P)
        rec["kernels_ms"] = {k: prof[k] for k in KERNELS if k in prof}
        map_ms = prof.get("map", 0.0) - (minus or 0.0)
        rec["k_map_ms"] = round(map_ms, 3)
        if map_bytes_per_row and map_ms > 0:
            rec["k_map_bytes_per_row"] = map_bytes_per_row
            rec["k_map_TB_per_s"] = round(map_bytes_per_row * rows / (map_ms * 1e-3) / 1e12, 3)
        print(json.dumps(rec), flush=True)
        return rec

    report("abc", map_plan([("COL", 1), ("COL", 2), ("MUL",), ("COL", 3), ("ADD",), O], [("EXPR", 0, I64)]), 32)
    report("f_abc", map_plan([("COL", 4), ("COL", 4), ("MUL",), ("COL", 4), ("ADD",), O], [("EXPR", 0, F64)]), 16)
    r1 = report("ops1", map_plan([("COL", 1), ("NEG",), O], [("EXPR", 0, I64)]), 16)
    r32 = report("ops32", map_plan([("COL", 1)] + [("NEG",)] * 32 + [O], [("EXPR", 0, I64)]), 16)
    print(json.dumps({"case": "per_op", "k_map_ms_per_op": round((r32["k_map_ms"] - r1["k_map_ms"]) / 31, 4),
                      "ns_per_row_and_op": round((r32["k_map_ms"] - r1["k_map_ms"]) / 31 * 1e6 / rows, 5)}), flush=True)
    lower_prog = [("COL", 1), ("INT", 8), ("MOD",), ("INT", 0), ("EQ",), ("NULL", I64), ("COL", 1), ("CASE",), O]
    lower_outs = [("EXPR", 0, I64), ("COL", 2, I64), ("COL", 3, I64)]
    lower = lambda p: p.new_map_node(scan(p), lower_prog, lower_outs)
    low = kernels(map_plan(lower_prog, lower_outs), P).get("map", 0.0)
    report("nullable", map_plan([("COL", 0), ("COL", 1), ("MUL",), ("COL", 2), ("ADD",), O], [("EXPR", 0, I64)], below=lower), 34, minus=low)

    g = pl.Plan()
    m = g.new_map_node(scan(g), [("COL", 1), ("COL", 2), ("MUL",), O], [("COL", 0, I32), ("EXPR", 0, I64)])
    g.root = g.new_group_node(m, [(0, 0)], [(pl.AGG_KEY, 0, I32), (pl.AGG_SUM, 1, I64)])
    report("sum_group", g, 24)
    s = pl.Plan()
    s.root = s.new_group_node(scan(s), [(0, 0)], [(pl.AGG_KEY, 0, I32), (pl.AGG_SUM, 1, I64)])
    report("sum_group_stored_column", s, 0)
    T.release()
    P.release()
    pctx.destroy()
    ctx.destroy()


if __name__ == "__main__":
    main()
