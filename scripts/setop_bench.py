#!/usr/bin/env python3
"""UNION / INTERSECT / EXCEPT [ALL] (RJ_NODE_SETOP), next to what they can be measured against.

Two relations, Page-packed and resident in HBM, result Page images left in HBM (as bench.py).  One JSON
line per case: wall time of rj_execute_resident (best / median / spread over the steps), and from one more
execution on a profiling context (level 2: the dispatch timestamps of every kernel) the time per kernel.

  union-all   UNION ALL of two INT32 columns of --rows rows each
              yardstick: a device-to-device copy of the same bytes (both columns into one buffer), timed in
              this process the same way; the ratio node / copy
  i32-few / i32-many / mixed-few / mixed-many
              the six operations on 2 x --rows / 2 rows: one INT32 column, or (INT32, INT64, FP64) columns,
              with 1000 distinct rows or with about as many distinct rows as a side has rows; per operation
              the share of the sort's kernels and k_group_heads, and the share of the k_setop_* kernels, in
              the sum of all kernel times
  intersect-vs-semi
              INTERSECT on one INT32 column without NULLs (1000 and --rows / 2 distinct values) next to the
              plan that was expressible before the node: RJ_NODE_GROUP (DISTINCT) over RJ_NODE_SEMI

    python scripts/setop_bench.py [--steps 5] [--warmup 1] [--rows 100000000] [--only NAME]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "radix-join_amd"))

CASES = ("union-all", "i32-few", "i32-many", "mixed-few", "mixed-many", "intersect-vs-semi")
OP_NAMES = ("union_all", "union", "intersect", "intersect_all", "except", "except_all")
SORT_SIDE = ("sort_encode", "sort_count", "sort_scan", "sort_scatter", "group_heads")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--only", choices=CASES, help="this case only")
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("setop_bench.py needs a GPU: it measures the HIP path only")
    from pyrj import capi
    from pyrj import plan as pl
    from pyrj import workloads as wl

    I32, I64, F64 = pl.INT32, pl.INT64, pl.FP64
    rows, half = a.rows, a.rows // 2
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(47)
    ctx = capi.Context(device=0)
    pctx = capi.Context(device=0, profile=2)  # 2: every launch is timed
    d = ctx.device_info()
    print(json.dumps({"device": d["name"], "arch": d["arch"], "compute_units": d["compute_units"], "rows": rows,
                      "steps": a.steps, "warmup": a.warmup}), flush=True)

    def adopt(c, cols, types):
        """device tensors -> Page images -> a resident table (a double's pages are an INT64's: 8 bytes a value)"""
        pages = [wl.pack_pages_gpu64(t.view(torch.int64)) if t.element_size() == 8 else wl.pack_pages_gpu(t) for t in cols]
        torch.cuda.synchronize()
        return c.adopt_device(cols[0].numel(), types, [p.data_ptr() for p in pages], [p.shape[0] for p in pages], keep=pages)

    def stats(times):
        return {"best_ms": round(min(times), 3), "median_ms": round(statistics.median(times), 3), "max_ms": round(max(times), 3)}

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
        return dict(stats(times), rows=out_rows)

    def kernels(plan, tables):
        """kernel -> ms of ONE execution on the profiling context"""
        pctx.execute_resident(plan, tables).free()
        pctx.profile_reset()
        pctx.execute_resident(plan, tables).free()
        torch.cuda.synchronize()
        return {r["name"]: round(r["total_ms"], 3) for r in pctx.profile()}

    def setop_plan(op, types):
        p = pl.Plan()
        l, r = p.new_scan_node(0, list(enumerate(types))), p.new_scan_node(1, list(enumerate(types)))
        p.root = p.new_setop_node(op, l, r, [(c, c, t) for c, t in enumerate(types)])
        return p

    def side(n, distinct, mixed):
        k = torch.randint(0, distinct, (n,), device=dev, generator=gen, dtype=torch.int32)
        if not mixed:
            return [k], [I32]
        return [k, k.to(torch.int64) * 4_000_000_007 - 12345, k.to(torch.float64) * 0.5 - 3.0], [I32, I64, F64]

    for name in CASES if a.only is None else (a.only,):
        if name == "union-all":
            cols = [torch.randint(-(2**31), 2**31, (rows,), device=dev, generator=gen, dtype=torch.int64).to(torch.int32) for _ in range(2)]
            L, R = adopt(ctx, cols[:1], [I32]), adopt(ctx, cols[1:], [I32])
            plan = setop_plan(pl.SET_UNION_ALL, [I32])
            rec = {"case": name, "node": timed(ctx, plan, [L, R])}
            dst, times = torch.empty(2 * rows, device=dev, dtype=torch.int32), []
            for i in range(a.warmup + a.steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dst[:rows].copy_(cols[0])
                dst[rows:].copy_(cols[1])
                torch.cuda.synchronize()
                if i >= a.warmup:
                    times.append((time.perf_counter() - t0) * 1e3)
            rec["d2d_copy"] = stats(times)
            rec["bytes_read_and_written"] = 2 * rows * 4 * 2
            rec["ratio_node_over_copy"] = round(rec["node"]["best_ms"] / rec["d2d_copy"]["best_ms"], 3)
            L.release(), R.release()
            PL, PR = adopt(pctx, cols[:1], [I32]), adopt(pctx, cols[1:], [I32])
            rec["kernels_ms"] = kernels(plan, [PL, PR])
            PL.release(), PR.release()
            print(json.dumps(rec), flush=True)
            del cols, dst
        elif name == "intersect-vs-semi":
            for distinct in (1000, half):
                lc, types = side(half, distinct, False)
                rc, _ = side(half, distinct, False)
                L, R = adopt(ctx, lc, types), adopt(ctx, rc, types)
                p = pl.Plan()
                l, r = p.new_scan_node(0, [(0, I32)]), p.new_scan_node(1, [(0, I32)])
                s = p.new_semi_join_node(False, l, r, 0, 0, [(0, I32)])
                p.root = p.new_group_node(s, [(0, 0)], [(pl.AGG_KEY, 0, I32)])
                rec = {"case": name, "distinct": distinct, "intersect": timed(ctx, setop_plan(pl.SET_INTERSECT, types), [L, R]),
                       "group_over_semi": timed(ctx, p, [L, R])}
                assert rec["intersect"]["rows"] == rec["group_over_semi"]["rows"], rec
                rec["ratio_intersect_over_group_semi"] = round(rec["intersect"]["best_ms"] / rec["group_over_semi"]["best_ms"], 3)
                L.release(), R.release()
                print(json.dumps(rec), flush=True)
                del lc, rc
        else:
            mixed, distinct = name.startswith("mixed"), (1000 if name.endswith("few") else half)
            lc, types = side(half, distinct, mixed)
            rc, _ = side(half, distinct, mixed)
            L, R = adopt(ctx, lc, types), adopt(ctx, rc, types)
            PL, PR = adopt(pctx, lc, types), adopt(pctx, rc, types)
            for op, op_name in enumerate(OP_NAMES):
                plan = setop_plan(op, types)
                rec = dict({"case": name, "op": op_name, "distinct": distinct}, **timed(ctx, plan, [L, R]))
                prof = kernels(plan, [PL, PR])
                total = sum(prof.values())
                rec["kernels_ms"] = prof
                rec["kernels_total_ms"] = round(total, 3)
                rec["share_sort_and_group_heads"] = round(sum(t for k, t in prof.items() if k in SORT_SIDE) / total, 3) if total else None
                rec["share_setop"] = round(sum(t for k, t in prof.items() if k.startswith("setop_")) / total, 3) if total else None
                print(json.dumps(rec), flush=True)
            for t in (L, R, PL, PR):
                t.release()
            del lc, rc
        torch.cuda.empty_cache()
    pctx.destroy()
    ctx.destroy()


if __name__ == "__main__":
    main()
