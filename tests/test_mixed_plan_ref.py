"""The mixed-kind plan generator (tests/_plangen.py) and the two references for its plans, on the CPU.

  * tests/_bruteref.py (row at a time, written from include/rj.h) and tests/_aggref.py (numpy; what
    tests/test_gpu_fuzz_mixed.py compares the device with) agree on every generated plan, as sorted
    row multisets — mid plans on the first MID_CAP rows of every base table, which keeps the plan and
    every node's role and leaves pure Python a size it can walk;
  * plans of scans and inner joins alone also agree with the pinned C oracle;
  * no relation of any plan exceeds _plangen.MAX_ROWS rows, so the device tests skip no seed;
  * the generator really mixes: the counts below are conditions on it, not measurements.
Everything is generated from seeds: there are no fixtures."""
import collections
import functools

import pytest

import _aggref
import _bruteref
import _oracle
import _plangen
import test_gpu_outer_join as og
from pyrj import plan as pl

SMALL, MID = range(300), range(20)
MID_CAP = 1500
NON_SCAN = _plangen.KINDS + ("agg",)


@functools.lru_cache(maxsize=None)
def plan_of(size, seed):
    return _plangen.mixed_plan(seed, size=size)


@functools.lru_cache(maxsize=None)
def kinds_of(size, seed):
    p = plan_of(size, seed)
    return [_plangen.kind_of(p.nodes[i]) for i in _plangen.reachable(p)]


def same_rows(a, b, what):
    assert a.num_rows == b.num_rows, (what, a.num_rows, b.num_rows)
    assert [c.type for c in a.columns] == [c.type for c in b.columns], what
    assert pl.canonical_rows(a) == pl.canonical_rows(b), what


def test_constants_are_the_kernels():
    assert (_plangen.JN_RMAX, _plangen.JN_HEAVY) == (og.JN_RMAX, og.JN_HEAVY)


def test_same_seed_same_plan():
    for size, seed in (("small", 7), ("mid", 3)):
        a, b = plan_of(size, seed), _plangen.mixed_plan(seed, size=size)
        assert a is not b and a.root == b.root and len(a.nodes) == len(b.nodes)
        assert [(type(x.data), x.data.__dict__, x.output_attrs) for x in a.nodes] == [(type(x.data), x.data.__dict__, x.output_attrs) for x in b.nodes]
        for ta, tb in zip(a.inputs, b.inputs):
            assert ta.num_rows == tb.num_rows and all((ca.pages == cb.pages).all() for ca, cb in zip(ta.columns, tb.columns))


@pytest.mark.parametrize("seed", SMALL)
def test_references_agree(seed):
    p = plan_of("small", seed)
    same_rows(_bruteref.execute(p), _aggref.execute(p), seed)


@pytest.mark.parametrize("seed", MID)
def test_references_agree_on_capped_mid_plans(seed):
    p = _plangen.capped(plan_of("mid", seed), MID_CAP)
    same_rows(_bruteref.execute(p), _aggref.execute(p), seed)


def test_oracle_agrees_on_plans_of_inner_joins():
    seeds = [s for s in SMALL if set(kinds_of("small", s)) <= {"scan", "join"}]
    assert len(seeds) >= 3, seeds
    for s in seeds:
        p = plan_of("small", s)
        same_rows(_oracle.execute(p), _aggref.execute(p), s)
        same_rows(_oracle.execute(p), _bruteref.execute(p), s)


@pytest.mark.parametrize("size,seeds", [("small", SMALL), ("mid", MID)], ids=["small", "mid"])
def test_no_relation_is_too_large(size, seeds):
    for s in seeds:
        rows = _plangen.relation_rows(plan_of(size, s))
        assert max(rows.values()) <= _plangen.MAX_ROWS, (s, rows)


def test_mid_tables_and_hot_keys():
    """2-3 tables of 5 000 ... 80 000 rows, at most one of at most JN_RMAX rows; in about a third of
    the seeds one value owns more than JN_HEAVY rows of a column of the largest table."""
    hot = 0
    for s in MID:
        p = plan_of("mid", s)
        n = [t.num_rows for t in p.inputs]
        assert 2 <= len(n) <= 3 and sum(x <= _plangen.JN_RMAX for x in n) <= 1, n
        assert all(x <= _plangen.JN_RMAX or 5_000 <= x <= 80_000 for x in n), n
        big = p.inputs[n.index(max(n))]
        for c, col in zip(big.columns, pl.decode_table(big)):
            if c.type != pl.VARCHAR and collections.Counter(col[0][col[1]].tolist()).most_common(1)[0][1] > _plangen.JN_HEAVY:
                hot += 1
                break
    assert 4 <= hot <= 10, hot


def test_mid_plans_reach_both_forms_of_every_join_kind():
    """What tests/test_gpu_fuzz_mixed.py then sees in the launch log, predicted from the row counts."""
    forms = collections.Counter()
    for s in MID:
        forms.update(_plangen.probe_forms(plan_of("mid", s)))
    for kind in ("join", "outer", "full"):
        assert forms[kind, "bcast"] and forms[kind, "part"], (kind, forms)
    assert forms["semi", "bcast"] + forms["anti", "bcast"] and forms["semi", "part"] + forms["anti", "part"], forms
    assert sum("agg" in kinds_of("mid", s) for s in MID) >= 3


def test_the_generator_really_mixes():
    roots, pairs = collections.Counter(), collections.Counter()
    three = varchar = mismatch = empty = 0
    for s in SMALL:
        p = plan_of("small", s)
        nodes = _plangen.reachable(p)
        roots[_plangen.kind_of(p.nodes[p.root])] += 1
        for i in nodes:
            for c in _plangen.children(p.nodes[i]):
                pairs[_plangen.kind_of(p.nodes[i]), _plangen.kind_of(p.nodes[c])] += 1
        three += len(set(kinds_of("small", s)) - {"scan"}) >= 3
        varchar += pl.VARCHAR in _plangen.out_types(p.nodes[p.root])
        mismatch += any(_plangen.mismatched(p, i) for i in nodes if i != p.root)
        empty += any(t.num_rows == 0 for t in p.inputs)
    for k in NON_SCAN:
        assert roots[k] >= 10, (k, roots)
    # (an aggregation has one child, so it is nobody's second child: the pairs count either child)
    for parent in NON_SCAN:
        for child in NON_SCAN:
            assert pairs[parent, child] >= 3, (parent, child, pairs[parent, child])
    assert three >= 20 and varchar >= 10 and mismatch >= 10 and empty >= 10, (three, varchar, mismatch, empty)


def test_agg_nodes_respect_the_carry_limit_in_the_worst_case():
    """Every generated AGG node fits rj.h's carry words with each aggregated column counted as
    nullable, unless its child is a scan (then the base column's NULLs decide)."""
    seen = 0
    for size, seeds in (("small", SMALL), ("mid", MID)):
        for s in seeds:
            p = plan_of(size, s)
            for i in _plangen.reachable(p):
                n = p.nodes[i]
                if _plangen.kind_of(n) != "agg":
                    continue
                child = p.nodes[n.data.child]
                ct = _plangen.out_types(child)
                assert ct[n.data.key_attr] in _plangen.AGGABLE
                cols = sorted({pl.agg_col(x) for x, _ in n.output_attrs if pl.agg_func(x) >= pl.AGG_COUNT})
                assert all(ct[c] in _plangen.AGGABLE for c in cols)
                for x, t in n.output_attrs:
                    f = pl.agg_func(x)
                    assert t == _aggref.result_type(f, ct[pl.agg_col(x)] if f != pl.AGG_COUNT_STAR else None, ct[n.data.key_attr])
                assert sum(pl.agg_func(x) == pl.AGG_KEY for x, _ in n.output_attrs) <= 2
                if _plangen.kind_of(child) == "scan":
                    t = p.inputs[child.data.base_table_id]
                    dec = pl.decode_table(t)
                    nullable = [not dec[child.output_attrs[c][0]][1].all() for c in cols]
                else:
                    nullable = [True] * len(cols)
                assert _plangen.agg_carry_fits(ct[n.data.key_attr], [(ct[c], nl) for c, nl in zip(cols, nullable)]), (size, s, i)
                seen += 1
    assert seen >= 100
