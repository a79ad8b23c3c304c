#!/usr/bin/env python3
"""Semi / anti joins against the inner join that outputs the same preserved columns.

Two shapes, Page-packed inputs resident in HBM, result Page images left in HBM (as bench.py):
  part   100 M filter keys (a permutation: unique) against 100 M preserved rows (uniform keys over
         twice the filter domain: half of them have a partner) with an INT32 payload — partitioned;
  bcast  4096 unique filter keys against 1 B preserved rows (uniform over 8192 values) — broadcast.
Each shape runs as SEMI, as ANTI and as INNER = Join(filter, preserved) outputting the preserved key
and payload; over a unique-key filter side INNER returns exactly the SEMI rows, after the same
partitioning.  One line per case: best / median ms of the timed steps and G preserved tuples/s
(preserved rows / best time).  The row counts are checked: SEMI == INNER, SEMI + ANTI == preserved.

    python scripts/filter_join_bench.py [--steps 5] [--warmup 2] [--only part|bcast]
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

I32 = pl.INT32
SHAPES = {
    "part": dict(n_filter=100_000_000, n_preserved=100_000_000, domain=200_000_000),
    "bcast": dict(n_filter=4096, n_preserved=1_000_000_000, domain=8192),
}


def plan_of(kind):
    """Scan(filter){key} x Scan(preserved){key, payload}; the filter side is the left (built) one."""
    p = pl.Plan()
    f = p.new_scan_node(0, [(0, I32)])
    s = p.new_scan_node(1, [(0, I32), (1, I32)])
    outs = [(1, I32), (2, I32)]  # the preserved key and payload
    if kind == "semi":
        p.root = p.new_semi_join_node(True, f, s, 0, 0, outs)
    elif kind == "anti":
        p.root = p.new_anti_join_node(True, f, s, 0, 0, outs)
    else:
        p.root = p.new_join_node(True, f, s, 0, 0, outs)
    return p


def run_shape(name, steps, warmup):
    sh = SHAPES[name]
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    fk = torch.randperm(sh["domain"], device=dev, generator=gen)[: sh["n_filter"]].to(torch.int32)
    pk = torch.randint(0, sh["domain"], (sh["n_preserved"],), device=dev, generator=gen, dtype=torch.int32)
    pp = torch.arange(sh["n_preserved"], device=dev, dtype=torch.int32)
    ctx = capi.Context(device=0)
    F = wl.adopt(ctx, [fk])
    P = wl.adopt(ctx, [pk, pp])
    del fk, pk, pp
    torch.cuda.empty_cache()
    rows = {}
    for kind in ("semi", "anti", "inner"):
        plan = plan_of(kind)
        times = []
        for i in range(warmup + steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = ctx.execute_resident(plan, [F, P])
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            rows[kind] = res.num_rows
            res.free()
            if i >= warmup:
                times.append(dt)
        best = min(times)
        print(f"{name:5s} {kind:5s} filter={sh['n_filter']} preserved={sh['n_preserved']} out_rows={rows[kind]} "
              f"best_ms={best:.2f} median_ms={statistics.median(times):.2f} "
              f"G_preserved_tuples_per_s={sh['n_preserved'] / best / 1e6:.2f}", flush=True)
    assert rows["semi"] == rows["inner"], rows
    assert rows["semi"] + rows["anti"] == sh["n_preserved"], rows
    F.release()
    P.release()
    ctx.destroy()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=list(SHAPES))
    a = ap.parse_args()
    info = capi.Context(device=0)
    d = info.device_info()
    info.destroy()
    print(f"# {d['name']} ({d['arch']}, {d['compute_units']} CUs); steps={a.steps} warmup={a.warmup}", flush=True)
    for name in SHAPES:
        if a.only in (None, name):
            run_shape(name, a.steps, a.warmup)


if __name__ == "__main__":
    main()
