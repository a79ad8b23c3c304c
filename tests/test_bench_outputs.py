"""bench.py's plain run and --dump-outputs: the result line's fields, the number of timed steps,
and the sampled join result it writes (rows named by their probe row, whatever order the device
wrote them in)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
from pyrj import workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pages(v, rows_per_page):
    n = v.numel()
    p = torch.zeros(((n + rows_per_page - 1) // rows_per_page, rows_per_page), dtype=v.dtype)
    p.view(-1)[:n] = v
    return p


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d) if f.endswith(".npy")}


@pytest.mark.parametrize("payload64", [True, False])
def test_dump_outputs_names_rows_by_probe_row(tmp_path, monkeypatch, payload64):
    """A PK-FK join result in shuffled row order, cut into pages the way the library writes them:
    the dump holds, for a seeded sample of probe rows, the key and both payloads of the output row
    that carries it, in float64, whatever the row order."""
    n = 50_021
    g = torch.Generator().manual_seed(5)
    rk = torch.randperm(n, generator=g).to(torch.int32)
    sk = torch.randint(0, n, (n,), generator=g).to(torch.int32)
    mul = wl.PAY_MUL if payload64 else 1
    rp = (torch.arange(n) * mul).to(torch.int64 if payload64 else torch.int32)
    rel = wl.Relations("t", n, n, 0, 1, rk, rp, sk, rp.clone(), payload64)
    row_of_key = torch.empty(n, dtype=torch.int64)
    row_of_key[rk.long()] = torch.arange(n)
    order = torch.randperm(n, generator=g)
    key = sk[order]
    rf = wl.ROWS64 if payload64 else wl.ROWS32
    cols = [_pages(key, wl.ROWS32), _pages(rp[row_of_key[key.long()]], rf), _pages(rel.sp[order], rf)]

    class Res:
        num_rows = n

    monkeypatch.setattr(wl, "result_column", lambda res, c, n_rows: (cols[c], None))
    bench.dump_outputs(Res(), rel, str(tmp_path / "a"), sample_rows=4000, chunk_pages=3)
    d = _load(tmp_path / "a")
    assert set(d) == {"num_rows", "probe_row", "matches", "key", "build_payload", "probe_payload"}
    assert all(a.dtype == np.float64 for a in d.values())
    assert d["num_rows"].tolist() == [n]
    pr = d["probe_row"].astype(np.int64)
    assert pr.shape == (4000,) and (np.diff(pr) > 0).all()
    assert (d["matches"] == 1).all()
    assert (d["key"] == sk.numpy()[pr]).all()
    assert (d["probe_payload"] == pr * mul).all()
    assert (d["build_payload"] == row_of_key.numpy()[sk.numpy()[pr]] * mul).all()
    # another row order of the same result: the same files
    order2 = torch.randperm(n, generator=g)
    key2 = sk[order2]
    cols[:] = [_pages(key2, wl.ROWS32), _pages(rp[row_of_key[key2.long()]], rf), _pages(rel.sp[order2], rf)]
    bench.dump_outputs(Res(), rel, str(tmp_path / "b"), sample_rows=4000, chunk_pages=5)
    d2 = _load(tmp_path / "b")
    for k in d:
        assert np.array_equal(d[k], d2[k]), k


@pytest.mark.gpu
def test_plain_bench_run_and_its_outputs(tmp_path):
    """A plain run times exactly --steps steps, reports ms_per_step, carries none of the --full
    fields, and dumps the last step's result, which matches the seeded inputs."""
    rows = 1_000_000
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--rows", str(rows), "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert line["metric"] == "probe_tuples_per_sec" and line["unit"] == "tuples/s" and line["higher_is_better"] is True
    assert line["dtype"] == "int32" and line["steps"] == 3 and line["warmup"] == 1
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(rows / (line["ms_per_step"] * 1e-3), rel=1e-6)
    assert not {"configs", "plan_ms", "ingest", "cpu_baseline"} & set(line)
    d = _load(out)
    assert sum(a.nbytes for a in d.values()) <= 64 << 20
    assert d["num_rows"].tolist() == [rows]
    assert (d["matches"] == 1).all()
    rel = wl.make_relations("config3", torch.device("cuda"), rows=rows)
    pr = torch.from_numpy(d["probe_row"].astype(np.int64)).cuda()
    key = rel.sk[pr].long()
    assert np.array_equal(d["key"], key.cpu().numpy().astype(np.float64))
    assert np.array_equal(d["probe_payload"], (pr * wl.PAY_MUL).cpu().numpy().astype(np.float64))
    brow = torch.from_numpy(d["build_payload"].astype(np.int64) // wl.PAY_MUL).cuda()
    assert bool((rel.rk[brow].long() == key).all())
