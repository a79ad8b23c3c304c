#!/usr/bin/env python3
"""The exactly rounded FP64 sum of RJ_NODE_GROUP (RJ_AGG_FSUM) next to the integer SUM of the same node.

One relation of 100 M rows, Page-packed and resident in HBM, result Page images left in HBM (as bench.py
and scripts/group_bench.py, whose shapes these are).  Every case runs three plans over the same keys:

  fsum-band   KEY, FSUM(x), COUNT(x) of an FP64 column in a narrow exponent band (prices: uniform in
              [0, 1000)) — every lane of a wave adds to the same three chunks
  fsum-wide   ... of an FP64 column of random signs, exponents (the whole finite range) and significands
  sum-i64     KEY, SUM(v), COUNT(v) of an INT64 column: the yardstick (k_group_reduce; the parent commit's
              figures for it are in profiles/group_bench.log)

  scalar / g10 / g1e4 / g1e7   no key, or one INT32 key with that many uniform groups

One JSON line per case: wall time of rj_execute_resident (best / median over the steps) of every plan, and
from one more execution on a profiling context (level 2: the dispatch timestamps of every kernel) the time
of the fsum_* kernels and of group_reduce.

    python scripts/fsum_bench.py [--steps 5] [--warmup 1] [--rows 100000000] [--only NAME]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "radix-join_amd"))

CASES = ("scalar", "g10", "g1e4", "g1e7")
FSUM_KERNELS = ("fsum_slots", "fsum_zero", "fsum_reduce", "fsum_finish")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--only", choices=CASES, help="this case only")
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("fsum_bench.py needs a GPU: it measures the HIP path only")
    from pyrj import capi
    from pyrj import plan as pl
    from pyrj import workloads as wl

    I32, I64, F64 = pl.INT32, pl.INT64, pl.FP64
    rows = a.rows
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(31)
    ctx = capi.Context(device=0)
    pctx = capi.Context(device=0, profile=2)  # 2: every launch is timed
    d = ctx.device_info()
    print(json.dumps({"device": d["name"], "arch": d["arch"], "compute_units": d["compute_units"], "rows": rows,
                      "steps": a.steps, "warmup": a.warmup}), flush=True)

    def plan(types, keyed, func, col, rt):
        p = pl.Plan()
        sc = p.new_scan_node(0, list(enumerate(types)))
        outs = ([(pl.AGG_KEY, 0, I32)] if keyed else []) + [(func, col, rt), (pl.AGG_COUNT, col, I64)]
        p.root = p.new_group_node(sc, [(0, 0)] if keyed else [], outs)
        return p

    def adopt(c, cols, types):
        pages = [wl.pack_pages_gpu64(t.view(torch.int64)) if t.element_size() == 8 else wl.pack_pages_gpu(t) for t in cols]
        torch.cuda.synchronize()
        return c.adopt_device(cols[0].numel(), types, [p.data_ptr() for p in pages], [p.shape[0] for p in pages], keep=pages)

    def timed(c, p, tables):
        times, out_rows = [], 0
        for i in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = c.execute_resident(p, tables)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            out_rows = res.num_rows
            res.free()
            if i >= a.warmup:
                times.append(dt)
        return round(min(times), 3), round(statistics.median(times), 3), out_rows

    def kernels(p, P):
        """kernel family -> ms of ONE execution on the profiling context"""
        pctx.execute_resident(p, [P]).free()
        pctx.profile_reset()
        pctx.execute_resident(p, [P]).free()
        torch.cuda.synchronize()
        return {r["name"]: round(r["total_ms"], 3) for r in pctx.profile()}

    band = torch.rand((rows,), device=dev, generator=gen, dtype=torch.float64) * 1000.0
    wide = (torch.randint(1, 2047, (rows,), device=dev, generator=gen, dtype=torch.int64) << 52) \
        | torch.randint(0, 2**52, (rows,), device=dev, generator=gen, dtype=torch.int64) \
        | (torch.randint(0, 2, (rows,), device=dev, generator=gen, dtype=torch.int64) << 63)
    wide = wide.view(torch.float64)
    ints = torch.randint(-(2**40), 2**40, (rows,), device=dev, generator=gen, dtype=torch.int64)
    types = [I32, F64, F64, I64]

    for name in CASES if a.only is None else (a.only,):
        groups = {"scalar": 1, "g10": 10, "g1e4": 10_000, "g1e7": 10_000_000}[name]
        key = torch.randint(0, groups, (rows,), device=dev, generator=gen, dtype=torch.int32)
        cols = [key, band, wide, ints]
        T, P = adopt(ctx, cols, types), adopt(pctx, cols, types)
        keyed = name != "scalar"
        rec = {"case": name}
        for tag, func, col, rt in (("fsum_band", pl.AGG_FSUM, 1, F64), ("fsum_wide", pl.AGG_FSUM, 2, F64), ("sum_i64", pl.AGG_SUM, 3, I64)):
            p = plan(types, keyed, func, col, rt)
            rec[f"{tag}_best_ms"], rec[f"{tag}_median_ms"], rec["groups"] = timed(ctx, p, [T])
            prof = kernels(p, P)
            rec[f"{tag}_kernels_ms"] = {k: prof[k] for k in FSUM_KERNELS + ("group_reduce",) if k in prof}
            if func == pl.AGG_FSUM:
                rec[f"{tag}_fsum_total_ms"] = round(sum(prof.get(k, 0.0) for k in FSUM_KERNELS), 3)
        reduce_ms = rec["sum_i64_kernels_ms"]["group_reduce"]
        for tag in ("fsum_band", "fsum_wide"):
            rec[f"ratio_{tag}_over_group_reduce"] = round(rec[f"{tag}_fsum_total_ms"] / reduce_ms, 2)
        T.release()
        P.release()
        print(json.dumps(rec), flush=True)
        del key, cols
        torch.cuda.empty_cache()
    pctx.destroy()
    ctx.destroy()


if __name__ == "__main__":
    main()
