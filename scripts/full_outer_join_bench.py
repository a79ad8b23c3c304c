#!/usr/bin/env python3
"""Full outer join against what a caller had to run before the node existed: the outer join of the
same inputs plus the anti join of the built side against the probed side.

The shapes of scripts/outer_join_bench.py, Page-packed inputs resident in HBM, result Page images
left in HBM (as bench.py), every side with an INT32 key and an INT32 payload:
  part   100 M built keys (unique, drawn from twice their number) against 100 M probed rows (uniform
         over the same domain): about 60 % of the built rows and half of the probed rows stay
         without a partner — partitioned;
  bcast  4096 built keys (unique, drawn from 16384 values) against 1 B probed rows (uniform over the
         lower 8192 values): half of the built rows stay without a partner — broadcast.
Each shape runs, in one process, as FULL (probed key + payload, built payload), as OUTER with the
same output list and as ANTI the other way round (built side preserved, its payload out).  One line
per case: best / median ms of the timed steps; then the ratio the node is judged by,
FULL / (OUTER + ANTI), best and median.  The row counts are checked: FULL == OUTER + ANTI.

    python scripts/full_outer_join_bench.py [--steps 7] [--warmup 2] [--only part|bcast]
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
    "part": dict(n_optional=100_000_000, n_preserved=100_000_000, domain=200_000_000, probe_domain=200_000_000),
    "bcast": dict(n_optional=4096, n_preserved=1_000_000_000, domain=16384, probe_domain=8192),
}


def plan_of(kind):
    """Scan(built){key, payload} x Scan(probed){key, payload}; the built side is the left one."""
    p = pl.Plan()
    o = p.new_scan_node(0, [(0, I32), (1, I32)])
    s = p.new_scan_node(1, [(0, I32), (1, I32)])
    outs = [(2, I32), (3, I32), (1, I32)]  # the probed key and payload, the built payload
    if kind == "full":
        p.root = p.new_full_outer_join_node(True, o, s, 0, 0, outs)
    elif kind == "outer":
        p.root = p.new_outer_join_node(True, o, s, 0, 0, outs)
    else:  # the built rows without a partner: the probed side filters
        p.root = p.new_anti_join_node(False, o, s, 0, 0, [(1, I32)])
    return p


def run_shape(name, steps, warmup):
    sh = SHAPES[name]
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    ok = torch.randperm(sh["domain"], device=dev, generator=gen)[: sh["n_optional"]].to(torch.int32)
    op = torch.arange(sh["n_optional"], device=dev, dtype=torch.int32)
    pk = torch.randint(0, sh["probe_domain"], (sh["n_preserved"],), device=dev, generator=gen, dtype=torch.int32)
    pp = torch.arange(sh["n_preserved"], device=dev, dtype=torch.int32)
    ctx = capi.Context(device=0)
    O = wl.adopt(ctx, [ok, op])
    P = wl.adopt(ctx, [pk, pp])
    del ok, op, pk, pp
    torch.cuda.empty_cache()
    rows, best, med = {}, {}, {}
    for kind in ("full", "outer", "anti"):
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
        print(f"{name:5s} {kind:5s} built={sh['n_optional']} probed={sh['n_preserved']} out_rows={rows[kind]} "
              f"best_ms={best[kind]:.2f} median_ms={med[kind]:.2f} "
              f"G_probed_tuples_per_s={sh['n_preserved'] / best[kind] / 1e6:.2f}", flush=True)
    for what, t in (("best", best), ("median", med)):
        print(f"{name:5s} ratio {what}: full/(outer+anti)={t['full'] / (t['outer'] + t['anti']):.3f} "
              f"full/outer={t['full'] / t['outer']:.3f}", flush=True)
    assert rows["full"] == rows["outer"] + rows["anti"] and rows["outer"] == sh["n_preserved"], rows
    O.release()
    P.release()
    ctx.destroy()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
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
