#!/usr/bin/env python3
"""Outer join against the two queries whose union it is: the inner join and the anti join.

The shapes of scripts/filter_join_bench.py, Page-packed inputs resident in HBM, result Page images
left in HBM (as bench.py), every side with an INT32 key and an INT32 payload:
  part   100 M optional keys (a permutation: unique) against 100 M preserved rows (uniform keys over
         twice the optional domain: half of them have a partner) — partitioned;
  bcast  4096 unique optional keys against 1 B preserved rows (uniform over 8192 values) — broadcast.
Each shape runs, in one process, as OUTER (preserved key + payload, optional payload), as INNER with
the same output list and as ANTI (preserved key + payload).  One line per case: best / median ms of
the timed steps and G preserved tuples/s (preserved rows / best time); then the two ratios the
outer join is judged by: OUTER / (INNER + ANTI) and OUTER / INNER, best and median.  The row counts
are checked: OUTER == INNER + ANTI == preserved rows (the optional keys are unique).

    python scripts/outer_join_bench.py [--steps 5] [--warmup 2] [--only part|bcast]
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
    "part": dict(n_optional=100_000_000, n_preserved=100_000_000, domain=200_000_000),
    "bcast": dict(n_optional=4096, n_preserved=1_000_000_000, domain=8192),
}


def plan_of(kind):
    """Scan(optional){key, payload} x Scan(preserved){key, payload}; the optional side is the left
    (built) one: `optional RIGHT JOIN preserved`."""
    p = pl.Plan()
    o = p.new_scan_node(0, [(0, I32), (1, I32)])
    s = p.new_scan_node(1, [(0, I32), (1, I32)])
    outs = [(2, I32), (3, I32), (1, I32)]  # the preserved key and payload, the optional payload
    if kind == "outer":
        p.root = p.new_outer_join_node(True, o, s, 0, 0, outs)
    elif kind == "anti":
        p.root = p.new_anti_join_node(True, o, s, 0, 0, outs[:2])
    else:
        p.root = p.new_join_node(True, o, s, 0, 0, outs)
    return p


def run_shape(name, steps, warmup):
    sh = SHAPES[name]
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    ok = torch.randperm(sh["domain"], device=dev, generator=gen)[: sh["n_optional"]].to(torch.int32)
    op = torch.arange(sh["n_optional"], device=dev, dtype=torch.int32)
    pk = torch.randint(0, sh["domain"], (sh["n_preserved"],), device=dev, generator=gen, dtype=torch.int32)
    pp = torch.arange(sh["n_preserved"], device=dev, dtype=torch.int32)
    ctx = capi.Context(device=0)
    O = wl.adopt(ctx, [ok, op])
    P = wl.adopt(ctx, [pk, pp])
    del ok, op, pk, pp
    torch.cuda.empty_cache()
    rows, best, med = {}, {}, {}
    for kind in ("outer", "inner", "anti"):
        plan = plan_of(kind)
        times = []
        for i in range(warmup + steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = ctx.execute_resident(plan, [O, P])
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            rows[kind] = res.num_rows
            res.free()
            if i >= warmup:
                times.append(dt)
        best[kind], med[kind] = min(times), statistics.median(times)
        print(f"{name:5s} {kind:5s} optional={sh['n_optional']} preserved={sh['n_preserved']} out_rows={rows[kind]} "
              f"best_ms={best[kind]:.2f} median_ms={med[kind]:.2f} "
              f"G_preserved_tuples_per_s={sh['n_preserved'] / best[kind] / 1e6:.2f}", flush=True)
    for what, t in (("best", best), ("median", med)):
        print(f"{name:5s} ratio {what}: outer/(inner+anti)={t['outer'] / (t['inner'] + t['anti']):.3f} "
              f"outer/inner={t['outer'] / t['inner']:.3f}", flush=True)
    assert rows["outer"] == rows["inner"] + rows["anti"] == sh["n_preserved"], rows
    O.release()
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
