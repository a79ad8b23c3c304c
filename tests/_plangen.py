"""Seeded generator of valid plans that mix all six node kinds of include/rj.h: inner, semi, anti,
outer and full outer joins and aggregations over scans (test infrastructure for
tests/test_mixed_plan_ref.py and tests/test_gpu_fuzz_mixed.py).

mixed_plan(seed, size=...) -> pl.Plan; the same seed gives the same plan.  The tables are those of
tests/test_gpu_fuzz.py's random_plan (its random_column / random_table are mirrored here, so that
file's plans stay what they are): 2-5 base tables of INT32 / INT64 / FP64 / VARCHAR columns, NULL
fractions from {0, 0.05, 0.3}, NaN and +-inf in FP64 columns, negative and wide keys, empty and
zero-page tables, the occasional table whose key column has another type.  size="mid" makes 2-3
tables of 5 000 ... 80 000 rows (one of them may hold at most JN_RMAX rows), and in about a third of
the seeds one key value owns more than JN_HEAVY rows of the largest table.

The tree: two relations are picked at random and combined by a binary node of a random kind with a
random build side, until one is left (left deep and bushy shapes both occur); with some probability a
relation (a scan's or a node's result) is wrapped in an aggregation first, and the root is at times.

Only plans the library documents as supported come out, so every device error is a test failure:
  * join keys are INT32 / INT64 / FP64, usually of one type on both sides, deliberately not in a few
    percent of the nodes (rj.h defines that result for every kind);
  * SEMI / ANTI name preserved columns only; OUTER no VARCHAR column of the optional side; FULL no
    VARCHAR column at all;
  * AGG keys are INT32 / INT64, COUNT / SUM / MIN / MAX go over INT32 / INT64 columns, the declared
    types follow _aggref.result_type, RJ_AGG_KEY appears 0, 1 or 2 times, and the distinct aggregated
    columns respect the carry limit with every one of them counted as nullable (the executor asks
    "has the column a validity array", which depends on what the child happened to produce) —
    except over a scan, for base columns that were generated without NULLs.

The generator evaluates every node with the numpy reference while it builds the plan (it needs the
children's types and widths anyway) and redraws a node from a deterministic sub-seed when its result
exceeds MAX_ROWS rows, so no caller has to skip a seed for its size."""
from __future__ import annotations

import numpy as np

import _aggref
import _filterref
import _fullref
from pyrj import plan as pl

I32, I64, F64, VC = pl.INT32, pl.INT64, pl.FP64, pl.VARCHAR
KEYABLE = (I32, I64, F64)
AGGABLE = (I32, I64)
MAX_ROWS = 400_000
JN_RMAX, JN_HEAVY = 4096, 65536  # csrc/rj_device.hpp, as tests/test_gpu_outer_join.py names them
KINDS = ("join", "semi", "anti", "outer", "full")
KIND_NAMES = ("scan",) + KINDS + ("agg",)


# ------------------------------------------------------------------ tables
def random_column(rng, dtype, n, key_domain, wide, hot=0):
    """test_gpu_fuzz.random_column, which also tells the NULL fraction it drew.  hot > 0: that many
    rows hold one value."""
    nulls = rng.choice([0.0, 0.0, 0.0, 0.05, 0.3])
    valid = rng.random(n) >= nulls
    if n <= key_domain and rng.random() < 0.5:
        base = rng.permutation(key_domain)[:n]
    else:
        base = rng.integers(0, key_domain, n)
    if hot:
        base[rng.permutation(n)[:hot]] = key_domain // 3
    if dtype == I32:
        return (I32, base.astype(np.int32) - (key_domain // 2 if wide else 0), valid), nulls
    if dtype == I64:
        return (I64, base.astype(np.int64) * (2**33 + 7 if wide else 1), valid), nulls
    if dtype == F64:
        vals = base.astype(np.float64) / 4
        if n > 3 and rng.random() < 0.3:
            vals[:3] = [np.nan, np.inf, -np.inf]
        return (F64, vals, valid), nulls
    strs = [None if not v else (b"s%d" % int(x)) * int(1 + x % 3) for v, x in zip(valid, rng.integers(0, key_domain, n))]
    if n > 2 and rng.random() < 0.15:
        strs[1] = b"L" * int(rng.integers(8186, 20000))  # long-string pages
    return (VC, strs), nulls


def random_table(rng, key_type, key_domain, wide, n, hot=0):
    """-> (table, column types, NULL fraction of every column); the first column of key_type is the
    one a hot value goes to."""
    ncols = int(rng.integers(1, 5))
    types = [key_type] + [int(rng.choice([I32, I64, F64, VC])) for _ in range(ncols - 1)]
    rng.shuffle(types)
    if key_type not in types:
        types[0] = key_type
    types = [int(t) for t in types]
    cols, nulls = [], []
    for ci, dt in enumerate(types):
        c, nl = random_column(rng, dt, n, key_domain, wide, hot if ci == types.index(key_type) else 0)
        cols.append(c)
        nulls.append(float(nl))
    t = pl.make_table(cols)
    if n == 0 and rng.random() < 0.5:
        t = pl.ColumnarTable(0, [pl.Column(dt) for dt in types])  # typed columns, zero pages
    return t, types, nulls


def _table_rows(rng, size, n_tables):
    """-> (rows of every table, hot rows of every table)"""
    if size == "small":
        return [int(rng.choice([0, 1, 5, 60, 500, 1200], p=[0.02, 0.03, 0.05, 0.3, 0.4, 0.2])) for _ in range(n_tables)], [0] * n_tables
    rows = [int(rng.integers(5_000, 80_001)) for _ in range(n_tables)]
    hot = [0] * n_tables
    if rng.random() < 0.7:  # both sides of the broadcast cut
        rows[int(rng.integers(0, n_tables))] = int(rng.choice([1, 700, JN_RMAX - 1, JN_RMAX]))
    if rng.random() < 0.34:  # one key value above JN_HEAVY rows of the largest table
        big = int(np.argmax(rows))
        rows[big] = int(rng.integers(JN_HEAVY + 5_000, 80_001))
        hot[big] = int(rng.integers(JN_HEAVY + 1, rows[big] - 2_000))
    return rows, hot


# ------------------------------------------------------------------ one node over evaluated children
class Rel:
    """A relation while the plan grows: its node, its kind, the evaluated columns, and per column
    whether it is known to have no validity array on the device (a scan of a NULL-free column)."""

    def __init__(self, node, kind, n, cols, nullfree):
        self.node, self.kind, self.n, self.cols, self.nullfree = node, kind, n, cols, nullfree

    @property
    def types(self):
        return [c[0] for c in self.cols]


def join_result(kind, build_left, left, right, la, ra, outs):
    """(rows, columns) of a binary node over two evaluated relations, by the functions
    _fullref.evaluate is made of."""
    both = left + right
    lw = len(left)
    bld, prb = (left, right) if build_left else (right, left)
    bk, pk = (left[la], right[ra]) if build_left else (right[ra], left[la])
    take, cat, null = _fullref._take, _fullref._concat, _fullref._null
    if kind in ("semi", "anti"):
        rows = _filterref.filter_rows(bk, pk, kind == "anti")
        return int(rows.shape[0]), [take(both[i], rows) for i in outs]
    brow, prow, lone_p, lone_b = _fullref.full_parts(bk, pk)
    built = lambda i: (i < lw) == build_left  # noqa: E731
    if kind == "join":
        return int(brow.shape[0]), [take(both[i], brow if built(i) else prow) for i in outs]
    if kind == "outer":
        return int(prow.shape[0] + lone_p.shape[0]), [
            cat(take(both[i], brow), null(both[i][0], lone_p.shape[0])) if built(i) else cat(take(both[i], prow), take(both[i], lone_p))
            for i in outs]
    assert kind == "full"
    out = []
    for i in outs:
        dt = both[i][0]
        if built(i):
            parts = [take(both[i], brow), null(dt, lone_p.shape[0]), take(both[i], lone_b)]
        else:
            parts = [take(both[i], prow), take(both[i], lone_p), null(dt, lone_b.shape[0])]
        out.append(cat(cat(parts[0], parts[1]), parts[2]))
    return int(prow.shape[0] + lone_p.shape[0] + lone_b.shape[0]), out


def agg_carry_fits(key_type, cols):
    """The carry limit of rj.h's RJ_NODE_AGG.  cols: (type, nullable) of the distinct aggregated
    columns."""
    if not cols or (len(cols) == 1 and not cols[0][1]):
        return True
    words = sum(1 if t == I32 else 2 for t, _ in cols) + int(any(nl for _, nl in cols))
    n64 = sum(t == I64 for t, _ in cols)
    return 2 <= words <= (3 if key_type == I32 else 2) and n64 <= 1 and (n64 == 0 or words == 3)


class _Gen:
    def __init__(self, seed, size):
        assert size in ("small", "mid")
        self.seed, self.size = int(seed), size
        self.tag = 0 if size == "small" else 1
        self.plan = pl.Plan()
        self.step = 0

    def sub_rng(self, attempt):
        return np.random.default_rng([self.seed, self.tag, self.step, attempt])

    # -- tables and scans
    def tables(self):
        rng = np.random.default_rng([self.seed, self.tag])
        self.key_type = int(rng.choice(KEYABLE, p=[0.6, 0.25, 0.15]))
        n_tables = int(rng.integers(2, 6)) if self.size == "small" else int(rng.choice([2, 3], p=[0.3, 0.7]))
        key_domain = int(rng.choice([300, 1500])) if self.size == "small" else int(rng.choice([20_000, 100_000]))
        wide = bool(rng.random() < 0.3)
        rows, hot = _table_rows(rng, self.size, n_tables)
        rels = []
        for ti in range(n_tables):
            kt = self.key_type if rng.random() < 0.96 else int(rng.choice(KEYABLE))
            t, types, nulls = random_table(rng, kt, key_domain, wide, rows[ti], hot[ti])
            self.plan.new_input(t)
            k = int(rng.integers(1, len(types) + 1))
            cols = [int(c) for c in rng.choice(len(types), size=k, replace=True)]
            if not any(types[c] == kt for c in cols):
                cols.append(types.index(kt))
            node = self.plan.new_scan_node(ti, [(c, types[c]) for c in cols])
            rels.append(Rel(node, "scan", t.num_rows, _filterref._scan(self.plan, self.plan.nodes[node]),
                            [nulls[c] == 0.0 for c in cols]))
        return rels

    # -- aggregation over one relation
    def agg(self, rng, rel):
        """-> Rel of an AGG node over rel, or None when rel has no INT32 / INT64 column."""
        types = rel.types
        keyc = [c for c, t in enumerate(types) if t in AGGABLE]
        if not keyc:
            return None
        pref = [c for c in keyc if types[c] == self.key_type]
        key = int(rng.choice(pref if pref and rng.random() < 0.8 else keyc))
        kt = types[key]
        chosen = []
        for _ in range(6):  # a random set of distinct aggregated columns that fits the carry words
            k = int(rng.choice([0, 1, 2, 3], p=[0.15, 0.45, 0.3, 0.1]))
            cand = [int(c) for c in rng.permutation(keyc)[:k]]
            if agg_carry_fits(kt, [(types[c], not rel.nullfree[c]) for c in cand]):
                chosen = cand
                break
        outs = []
        for c in chosen:
            funcs = [f for f in (pl.AGG_COUNT, pl.AGG_SUM, pl.AGG_MIN, pl.AGG_MAX) if rng.random() < 0.5]
            for f in funcs or [int(rng.choice([pl.AGG_COUNT, pl.AGG_SUM, pl.AGG_MIN, pl.AGG_MAX]))]:
                outs.append((f, c, _aggref.result_type(f, types[c], kt)))
        if rng.random() < 0.6:
            outs.append((pl.AGG_COUNT_STAR, 0, I64))
        n_key = int(rng.choice([0, 1, 2], p=[0.15, 0.6, 0.25]))
        if not outs and n_key == 0:
            n_key = 1
        outs += [(pl.AGG_KEY, key, kt)] * n_key
        outs = [outs[i] for i in rng.permutation(len(outs))]
        n, cols = _aggref.aggregate(rel.cols, key, outs)
        node = self.plan.new_agg_node(rel.node, key, outs)
        return Rel(node, "agg", n, cols, [False] * len(cols))

    # -- one binary node
    def pick_keys(self, rng, lt, rt):
        """Usually two columns of one type, the plan's key type when both children have it; in a few
        percent of the nodes deliberately (and where the children share no keyable type, perforce)
        columns of two types."""
        common = sorted({t for t in lt if t in KEYABLE} & {t for t in rt if t in KEYABLE})
        if common and rng.random() < 0.96:
            kt = self.key_type if self.key_type in common and rng.random() < 0.93 else int(rng.choice(common))
            return (int(rng.choice([c for c, t in enumerate(lt) if t == kt])),
                    int(rng.choice([c for c, t in enumerate(rt) if t == kt])))
        la = int(rng.choice([c for c, t in enumerate(lt) if t in KEYABLE]))
        other = [c for c, t in enumerate(rt) if t in KEYABLE and t != lt[la]]
        return la, int(rng.choice(other or [c for c, t in enumerate(rt) if t in KEYABLE]))

    def binary(self, rng, left, right, safe):
        """-> (kind, build_left, la, ra, outs, n, cols): one drawn node and its evaluated result."""
        lt, rt = left.types, right.types
        la, ra = self.pick_keys(rng, lt, rt)
        kind = str(rng.choice(("semi", "anti") if safe else KINDS))
        build_left = bool(rng.random() < 0.5)
        both = lt + rt
        lw = len(lt)
        built = lambda c: (c < lw) == build_left  # noqa: E731
        if kind in ("semi", "anti"):
            cand = [c for c in range(len(both)) if not built(c)]
        elif kind == "outer":
            cand = [c for c in range(len(both)) if not (built(c) and both[c] == VC)]
        elif kind == "full":
            cand = [c for c in range(len(both)) if both[c] != VC]
        else:
            cand = list(range(len(both)))
        k = int(rng.integers(1, min(6, len(cand)) + 1))
        outs = [int(c) for c in rng.choice(cand, size=k, replace=True)]  # duplicates, any order
        vcs = [c for c in cand if both[c] == VC]
        if vcs and rng.random() < 0.5:
            outs.insert(int(rng.integers(0, len(outs) + 1)), int(rng.choice(vcs)))
        if not any(both[c] == self.key_type for c in outs):  # keep a column of the plan's key type for the parents
            keys = [c for c in cand if both[c] == self.key_type]
            if keys:
                outs.append(int(rng.choice(keys)))
        if not any(both[c] in KEYABLE for c in outs):  # a parent needs a column to join on
            keys = [c for c in (la, lw + ra) if c in cand]
            outs.append(keys[0] if keys else int(rng.choice([c for c in cand if both[c] in KEYABLE])))
        n, cols = join_result(kind, build_left, left.cols, right.cols, la, ra, outs)
        return kind, build_left, la, ra, outs, n, cols

    def combine(self, rels):
        """Replace two of rels by a binary node over them."""
        self.step += 1
        attempt = 0
        while True:
            rng = self.sub_rng(attempt)
            i, j = (int(x) for x in rng.choice(len(rels), size=2, replace=False))  # either may be the left child
            left, right = rels[i], rels[j]
            # a semi / anti join never holds more rows than its preserved child: the redraws end
            kind, build_left, la, ra, outs, n, cols = self.binary(rng, left, right, safe=attempt >= 6)
            if n <= MAX_ROWS:
                break
            attempt += 1
        p = self.plan
        both = left.types + right.types
        mk = {"join": p.new_join_node, "semi": p.new_semi_join_node, "anti": p.new_anti_join_node,
              "outer": p.new_outer_join_node, "full": p.new_full_outer_join_node}[kind]
        node = mk(build_left, left.node, right.node, la, ra, [(c, both[c]) for c in outs])
        rest = [r for k, r in enumerate(rels) if k not in (i, j)]
        return rest + [Rel(node, kind, n, cols, [False] * len(cols))]

    def maybe_agg(self, rels, p):
        self.step += 1
        rng = self.sub_rng(0)
        if rng.random() < p:
            k = int(rng.integers(0, len(rels)))
            a = self.agg(rng, rels[k])
            if a is not None:
                rels[k] = a

    def build(self):
        rels = self.tables()
        while len(rels) > 1:
            self.maybe_agg(rels, 0.3)
            rels = self.combine(rels)
        self.maybe_agg(rels, 0.25)  # ... and at the root
        self.plan.root = rels[0].node
        return self.plan


def mixed_plan(seed, *, size="small") -> pl.Plan:
    return _Gen(seed, size).build()


# ------------------------------------------------------------------ what a plan holds
def kind_of(node):
    d = node.data
    if isinstance(d, pl.ScanNode):
        return "scan"
    if isinstance(d, pl.AggNode):
        return "agg"
    if isinstance(d, pl.FilterJoinNode):
        return "semi" if d.kind == pl.NODE_SEMI else "anti"
    return {pl.JoinNode: "join", pl.OuterJoinNode: "outer", pl.FullOuterJoinNode: "full"}[type(d)]


def children(node):
    d = node.data
    if isinstance(d, pl.ScanNode):
        return []
    return [d.child] if isinstance(d, pl.AggNode) else [d.left, d.right]


def out_types(node):
    return [t for _, t in node.output_attrs]


def reachable(plan, idx=None):
    """Node indices of the tree under idx (default the root), parents first."""
    idx = plan.root if idx is None else idx
    out = [idx]
    for c in children(plan.nodes[idx]):
        out += reachable(plan, c)
    return out


def mismatched(plan, idx):
    """Is node idx a binary node whose two key columns have different types?"""
    n = plan.nodes[idx]
    if kind_of(n) in ("scan", "agg"):
        return False
    d = n.data
    return out_types(plan.nodes[d.left])[d.left_attr] != out_types(plan.nodes[d.right])[d.right_attr]


def relation_rows(plan):
    """{node index: rows} of every node of the tree, by the numpy reference."""
    return {i: _aggref.evaluate(plan, i)[0] for i in reachable(plan)}


def capped(plan, rows):
    """The same plan over the first `rows` rows of every base table."""
    p = pl.Plan()
    p.nodes, p.root = plan.nodes, plan.root
    for t in plan.inputs:
        n = min(rows, t.num_rows)
        cols = []
        for c, col in zip(t.columns, pl.decode_table(t)):
            cols.append((c.type, col[:n]) if c.type == VC else (c.type, col[0][:n], col[1][:n]))
        p.new_input(pl.make_table(cols) if n else pl.ColumnarTable(0, [pl.Column(c.type) for c in t.columns]))
    return p


def probe_forms(plan, rows=None):
    """What the executor does with every binary node, from the children's row counts (rows:
    relation_rows(plan)) -> [(kind, "none" | "bcast" | "part")], by rj_exec.hip's rules: a node whose
    result needs no probe launches nothing (an empty preserved / probed child; for the inner and the
    semi join also an empty build side or keys of two types); a build side of at most JN_RMAX rows,
    an empty one and keys of two types take the broadcast kernels; FULL builds an empty child
    whatever build_left says.  (No forced radix bits.)"""
    rows = rows or relation_rows(plan)
    out = []
    for i in reachable(plan):
        kind = kind_of(plan.nodes[i])
        if kind in ("scan", "agg"):
            continue
        d = plan.nodes[i].data
        ln, rn = rows[d.left], rows[d.right]
        build_left = d.build_left
        if kind == "full" and (rn if build_left else ln) == 0:
            build_left = not build_left
        nb, npr = (ln, rn) if build_left else (rn, ln)
        mis = mismatched(plan, i)
        if npr == 0 or (kind in ("join", "semi") and (nb == 0 or mis)):
            out.append((kind, "none"))
        else:
            out.append((kind, "bcast" if nb <= JN_RMAX or mis else "part"))
    return out
