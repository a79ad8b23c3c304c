#!/usr/bin/env python3
"""GROUP BY (RJ_NODE_AGG) next to the inner self-join of the same relation.

One relation of 100 M rows, Page-packed and resident in HBM, result Page images left in HBM (as
bench.py): an INT32 key and an INT64 value.  The node computes key, COUNT(*), SUM, MIN, MAX of the
value.  Group shapes: 10, 10^4 and 10^7 uniform groups, and Zipf-0.9 keys over 10^7 values.
Each shape runs, in one process, as the aggregation and as the inner self-join R JOIN R on the key
with the value carried on both sides (same key, same carry; it partitions two sides where the node
partitions one).  A self-join whose result exceeds what one relation may hold (2^32 rows: 10 and 10^4
groups, Zipf) is refused by the library; the line then says so, and the self-join of a relation
with 100 M UNIQUE keys — the least work a self-join of that size can be — stands in as yardstick.
One line per case: best / median ms of the timed steps, G input rows/s, and for the node the
algorithmic bytes / best time / 8 TB/s.  The bytes follow the node's bit plan: 12-byte
tuples, 4 B for the first histogram, 24 B per radix pass, 12 B to read the partitions, 36 B per group;
the pass count is derived from the row count as the executor does and printed next to the figure.

    python scripts/agg_bench.py [--steps 5] [--warmup 2] [--rows 100000000] [--only NAME]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "radix-join_amd"))

import torch  # noqa: E402

from pyrj import capi  # noqa: E402
from pyrj import plan as pl  # noqa: E402
from pyrj import workloads as wl  # noqa: E402

I32, I64 = pl.INT32, pl.INT64
SHAPES = {"g10": 10, "g1e4": 10_000, "g1e7": 10_000_000, "zipf": 10_000_000, "unique": 0}
PEAK_BYTES_PER_S = 8e12
AGG_TARGET, PT_MAXBITS = 384, 9  # rj_device.hpp: mean tuples per partition, radix bits per pass


def radix_passes(rows):
    """Passes of the node's automatic bit plan (Exec::agg_bits, radix_plan())."""
    bits = min(max((max(-(-rows // AGG_TARGET), 1) - 1).bit_length(), 1), 21)
    return -(-bits // PT_MAXBITS)


def agg_plan():
    p = pl.Plan()
    s = p.new_scan_node(0, [(0, I32), (1, I64)])
    p.root = p.new_agg_node(s, 0, [(pl.AGG_KEY, 0, I32), (pl.AGG_COUNT_STAR, 0, I64), (pl.AGG_SUM, 1, I64),
                                   (pl.AGG_MIN, 1, I64), (pl.AGG_MAX, 1, I64)])
    return p


def join_plan():
    p = pl.Plan()
    a = p.new_scan_node(0, [(0, I32), (1, I64)])
    b = p.new_scan_node(0, [(0, I32), (1, I64)])
    p.root = p.new_join_node(True, a, b, 0, 0, [(0, I32), (1, I64), (3, I64)])
    return p


def timed(ctx, plan, tables, steps, warmup):
    times, rows = [], 0
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = ctx.execute_resident(plan, tables)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        rows = res.num_rows
        res.free()
        if i >= warmup:
            times.append(dt)
    return min(times), statistics.median(times), rows


def run_shape(name, n, steps, warmup):
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(17)
    if name == "zipf":
        k = wl.zipf_keys(SHAPES[name], n, 0.9, dev, gen).to(torch.int32)
    elif name == "unique":
        k = torch.randperm(n, device=dev, generator=gen).to(torch.int32)
    else:
        k = torch.randint(0, SHAPES[name], (n,), device=dev, generator=gen, dtype=torch.int32)
    v = torch.randint(-(2**40), 2**40, (n,), device=dev, generator=gen, dtype=torch.int64)
    ctx = capi.Context(device=0)
    R = wl.adopt(ctx, [k, v])
    del k, v
    torch.cuda.empty_cache()
    if name != "unique":
        best, med, groups = timed(ctx, agg_plan(), [R], steps, warmup)
        passes = radix_passes(n)
        algo = (4.0 + 24.0 * passes + 12.0) * n + 36.0 * groups
        print(f"{name:6s} agg   rows={n} groups={groups} best_ms={best:.2f} median_ms={med:.2f} "
              f"G_rows_per_s={n / best / 1e6:.2f} radix_passes={passes} algorithmic_GB={algo / 1e9:.2f} "
              f"fraction_of_8TBps={algo / (best * 1e-3) / PEAK_BYTES_PER_S:.3f}", flush=True)
    try:
        jb, jm, jrows = timed(ctx, join_plan(), [R], steps, warmup)
        print(f"{name:6s} self-join rows={n} out_rows={jrows} best_ms={jb:.2f} median_ms={jm:.2f}", flush=True)
        if name != "unique":
            print(f"{name:6s} ratio agg/self-join: best={best / jb:.3f} median={med / jm:.3f}", flush=True)
    except capi.RjError as e:
        print(f"{name:6s} self-join refused: {e}", flush=True)
        jb = None
    R.release()
    ctx.destroy()
    torch.cuda.empty_cache()
    return (best if name != "unique" else None), jb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--only", choices=list(SHAPES))
    a = ap.parse_args()
    info = capi.Context(device=0)
    d = info.device_info()
    info.destroy()
    print(f"# {d['name']} ({d['arch']}, {d['compute_units']} CUs); rows={a.rows} steps={a.steps} warmup={a.warmup}", flush=True)
    aggs, uniq = {}, None
    for name in SHAPES:
        if a.only in (None, name):
            ab, jb = run_shape(name, a.rows, a.steps, a.warmup)
            if name == "unique":
                uniq = jb
            else:
                aggs[name] = ab
    if uniq:
        for name, ab in aggs.items():
            print(f"{name:6s} ratio agg/unique-key self-join (best): {ab / uniq:.3f}", flush=True)


if __name__ == "__main__":
    main()
