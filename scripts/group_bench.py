#!/usr/bin/env python3
"""GROUP BY with any keys, or none (RJ_NODE_GROUP), next to the nodes it can be measured against.

One relation of 100 M rows, Page-packed and resident in HBM, result Page images left in HBM (as
bench.py).  Every case runs the node, computing its key(s), COUNT(*), SUM, MIN and MAX of one INT64
value, and in the same process the yardstick named below.  One JSON line per case: wall time of
rj_execute_resident (best / median over the steps) of every plan, and from one more execution on a
profiling context (level 2: the dispatch timestamps of every kernel) the time per kernel family.

  scalar    no key: SELECT COUNT(*), SUM(v), MIN(v), MAX(v)
            yardstick: RJ_NODE_SELECT over the same column with a predicate that keeps no row (k_select
            reads the column once and writes nothing)
  g10 / g1e4 / g1e7   one INT32 key with that many uniform groups
  two-key   GROUP BY a, b: a in [0, 200), b over the whole INT32 range
  f64       one FP64 key, 10^6 distinct values
            yardstick of the keyed cases: RJ_NODE_SORT on the same keys with LIMIT 1 — the sort alone —;
            node minus sort is what the grouping kernels cost, given as their bytes over that time:
            per row k_group_heads gathers each key (4 B row id + the key) and k_group_reduce the value
            (4 B row id + 8 B); per group 8 B per accumulator and the keys
            single-key cases also: RJ_NODE_AGG (the hashed node) on the same input, and the ratio

    python scripts/group_bench.py [--steps 5] [--warmup 1] [--rows 100000000] [--only NAME]
    rocprofv3 --kernel-trace --stats --output-format csv -- python3 scripts/group_bench.py --only scalar --steps 2
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "radix-join_amd"))

CASES = ("scalar", "g10", "g1e4", "g1e7", "two-key", "f64")
GROUP_KERNELS = ("group_heads", "group_scan", "group_keys", "group_init", "group_reduce", "group_column")
SORT_KERNELS = ("sort_encode", "sort_count", "sort_scan", "sort_scatter")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--only", choices=CASES, help="this case only, no profiling context (a profiler's run)")
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("group_bench.py needs a GPU: it measures the HIP path only")
    from pyrj import capi
    from pyrj import plan as pl
    from pyrj import workloads as wl

    I32, I64, F64 = pl.INT32, pl.INT64, pl.FP64
    KEY, STAR, SUM, MIN, MAX = pl.AGG_KEY, pl.AGG_COUNT_STAR, pl.AGG_SUM, pl.AGG_MIN, pl.AGG_MAX
    rows = a.rows
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(31)
    ctx = capi.Context(device=0)
    pctx = None if a.only else capi.Context(device=0, profile=2)  # 2: every launch is timed
    d = ctx.device_info()
    print(json.dumps({"device": d["name"], "arch": d["arch"], "compute_units": d["compute_units"], "rows": rows,
                      "steps": a.steps, "warmup": a.warmup}), flush=True)

    def scan(p, types):
        return p.new_scan_node(0, list(enumerate(types)))

    def group_plan(types, keys):
        p = pl.Plan()
        v = len(types) - 1
        outs = [(KEY, c, types[c]) for c, _ in keys] + [(STAR, 0, I64), (SUM, v, I64), (MIN, v, I64), (MAX, v, I64)]
        p.root = p.new_group_node(scan(p, types), keys, outs)
        return p

    def sort_plan(types, keys):
        p = pl.Plan()
        p.root = p.new_sort_node(scan(p, types), keys, [(keys[0][0], types[keys[0][0]]), (len(types) - 1, I64)], limit=1)
        return p

    def agg_plan(types):
        p = pl.Plan()
        p.root = p.new_agg_node(scan(p, types), 0, [(KEY, 0, types[0]), (STAR, 0, I64), (SUM, 1, I64), (MIN, 1, I64), (MAX, 1, I64)])
        return p

    def select_none_plan(types):
        p = pl.Plan()
        v = len(types) - 1
        p.root = p.new_select_node(scan(p, types), [("LT", v, -(2**62))], [(v, I64)])   # the values are within +-2^40
        return p

    def adopt(c, cols, types):
        """device tensors -> Page images -> a resident table (a double's pages are an INT64's: 8 bytes a value)"""
        pages = [wl.pack_pages_gpu64(t.view(torch.int64)) if t.element_size() == 8 else wl.pack_pages_gpu(t) for t in cols]
        torch.cuda.synchronize()
        return c.adopt_device(cols[0].numel(), types, [p.data_ptr() for p in pages], [p.shape[0] for p in pages], keep=pages)

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

    def kernels(plan, cols, types):
        """kernel family -> ms of ONE execution on the profiling context"""
        P = adopt(pctx, cols, types)
        pctx.execute_resident(plan, [P]).free()
        pctx.profile_reset()
        pctx.execute_resident(plan, [P]).free()
        torch.cuda.synchronize()
        prof = {r["name"]: round(r["total_ms"], 3) for r in pctx.profile()}
        P.release()
        return prof

    v = torch.randint(-(2**40), 2**40, (rows,), device=dev, generator=gen, dtype=torch.int64)

    def key_columns(name):
        if name == "scalar":
            return [], []
        if name == "two-key":
            return [torch.randint(0, 200, (rows,), device=dev, generator=gen, dtype=torch.int32),
                    torch.randint(-(2**31), 2**31, (rows,), device=dev, generator=gen, dtype=torch.int32)], [I32, I32]
        if name == "f64":
            return [torch.randint(-500_000, 500_000, (rows,), device=dev, generator=gen, dtype=torch.int64).to(torch.float64) * 0.25], [F64]
        groups = {"g10": 10, "g1e4": 10_000, "g1e7": 10_000_000}[name]
        return [torch.randint(0, groups, (rows,), device=dev, generator=gen, dtype=torch.int32)], [I32]

    for name in CASES if a.only is None else (a.only,):
        kcols, ktypes = key_columns(name)
        cols, types = kcols + [v], ktypes + [I64]
        keys = [(c, 0) for c in range(len(kcols))]
        T = adopt(ctx, cols, types)
        rec = {"case": name}
        gplan = group_plan(types, keys)
        rec["group_best_ms"], rec["group_median_ms"], rec["groups"] = timed(ctx, gplan, [T])
        if name == "scalar":
            yard, yname = select_none_plan(types), "select_none"
        else:
            yard, yname = sort_plan(types, keys), "sort_limit1"
        rec[f"{yname}_best_ms"], rec[f"{yname}_median_ms"], _ = timed(ctx, yard, [T])
        rec[f"ratio_group_over_{yname}"] = round(rec["group_best_ms"] / rec[f"{yname}_best_ms"], 3)
        if name in ("g10", "g1e4", "g1e7"):
            rec["agg_best_ms"], rec["agg_median_ms"], agg_rows = timed(ctx, agg_plan(types), [T])
            assert agg_rows == rec["groups"], (agg_rows, rec["groups"])
            rec["ratio_group_over_agg"] = round(rec["group_best_ms"] / rec["agg_best_ms"], 3)
        T.release()
        if name != "scalar":
            # what the grouping kernels move: per row the keys and the value, each behind a 4-byte row id; per group the outputs
            kbytes = sum(4 if t == I32 else 8 for t in ktypes)
            moved = rows * (4 * len(ktypes) + kbytes + 4 + 8) + rec["groups"] * (8 * 5 + kbytes)
            extra_ms = rec["group_best_ms"] - rec["sort_limit1_best_ms"]
            rec["group_minus_sort_ms"] = round(extra_ms, 3)
            rec["grouping_bytes_per_row"] = round(moved / rows, 1)
            rec["grouping_TB_per_s"] = round(moved / (extra_ms * 1e-3) / 1e12, 3) if extra_ms > 0 else None
        if pctx is not None:
            prof = kernels(gplan, cols, types)
            rec["group_kernels_ms"] = {k: prof[k] for k in GROUP_KERNELS + SORT_KERNELS if k in prof}
            rec["group_kernels_total_ms"] = round(sum(prof.get(k, 0.0) for k in GROUP_KERNELS), 3)
            yprof = kernels(yard, cols, types)
            rec[f"{yname}_kernels_ms"] = {k: t for k, t in yprof.items() if k in SORT_KERNELS + ("select", "gather")}
        print(json.dumps(rec), flush=True)
        del kcols, cols
        torch.cuda.empty_cache()
    if pctx is not None:
        pctx.destroy()
    ctx.destroy()


if __name__ == "__main__":
    main()
