"""Legal re-paginations of one logical column.

pyrj.pages packs a column the way the reference's ColumnInserter does: full pages, one short page at the
end.  The page format (tests/_pagecheck.py) allows much more, and other producers emit it: short pages
anywhere, pages with nr == 0, pages that hold more rows than a page without NULLs can, one all-NULL page
of 65 504 rows, long-string chains between any of these.  This module cuts a logical column into pages at
row counts the caller chooses, so that a test can feed the SAME column in many layouts and expect the
same result.

  cut_fixed / cut_varchar   `cuts` = rows per page, 0 = a page with nr == 0.  Every page is made by
                            pyrj.pages.pack_* on the slice, which must come back as exactly one page (a
                            string above 8185 bytes as one chain); empty pages are 8192 zero bytes.
  scribble                  fills what the format leaves unspecified with 0xA5: the bytes between the data
                            and the bitmap, and the bits above nr in the last bitmap byte.
  LAYOUTS / VARCHAR_LAYOUTS named generators of `cuts`.
  column / varchar_column   cut + scribble + the proof that the result is legal and still the same
                            column (check_column), which every test goes through before a page reaches
                            the library.
"""
import numpy as np

import _pagecheck as pc
from pyrj import pages as pg
from pyrj import plan as pl

INT32, INT64, FP64, VARCHAR = pl.INT32, pl.INT64, pl.FP64, pl.VARCHAR
PS = pg.PAGE_SIZE
FILL = 0xA5
LONG = pc.MAX_INLINE + 1  # 8186: the shortest string that becomes a 0xffff / 0xfffe chain


def rows_full(dtype):
    return pg.rows_per_full_page(dtype)  # 1984 (INT32) / 1007 (INT64, FP64)


def max_null_rows(dtype):
    """rows of one all-NULL page: the bitmap alone fills the page behind the header"""
    return (PS - pg.HDR[dtype]) * 8  # 65 504 (INT32) / 65 472 (INT64, FP64)


def fits(valid_slice, dtype):
    """does a slice of rows fit one fixed-width page?"""
    nr = len(valid_slice)
    return nr <= max_null_rows(dtype) and pg.HDR[dtype] + int(np.count_nonzero(valid_slice)) * pg.WIDTH[dtype] + (nr + 7) // 8 <= PS


# ----------------------------------------------------------------------------------- cutting
def cut_fixed(values, valid, dtype, cuts):
    """pages [len(cuts), 8192] of a fixed-width column cut at `cuts` rows per page (sum(cuts) rows)"""
    values = np.ascontiguousarray(values, dtype=pg.NP_DTYPE[dtype])
    valid = np.ones(values.shape[0], bool) if valid is None else np.asarray(valid, dtype=bool)
    assert sum(cuts) <= values.shape[0], (sum(cuts), values.shape[0])
    out = np.zeros((len(cuts), PS), dtype=np.uint8)
    at = 0
    for k, nr in enumerate(cuts):
        if nr == 0:
            continue  # a page with nr == 0: 8192 zero bytes
        assert fits(valid[at:at + nr], dtype), f"cut {k}: {nr} rows do not fit one page"
        page = pg.pack_fixed(values[at:at + nr], valid[at:at + nr], dtype)
        assert page.shape[0] == 1, f"cut {k}: the packer made {page.shape[0]} pages of {nr} rows"
        out[k] = page[0]
        at += nr
    return out


def cut_varchar(strings, cuts):
    """pages of a VARCHAR column cut at `cuts` rows per page; a slice that is ONE string above 8185 bytes
    becomes its chain of 0xffff / 0xfffe pages (so the column has more pages than cuts)"""
    strings = list(strings)
    assert sum(cuts) <= len(strings)
    out, at = [], 0
    for k, nr in enumerate(cuts):
        if nr == 0:
            out.append(np.zeros((1, PS), dtype=np.uint8))
            continue
        sl = strings[at:at + nr]
        pages = pg.pack_varchar(sl)
        first = int(pages[0, :2].view(np.uint16)[0])
        if first == pc.LONG_FIRST:
            assert nr == 1, f"cut {k}: a long string is a cut of its own"
            assert (pages[1:, :2].view(np.uint16)[:, 0] == pc.LONG_NEXT).all()
        else:
            assert pages.shape[0] == 1, f"cut {k}: {nr} rows do not fit one page"
        out.append(pages)
        at += nr
    return np.concatenate(out) if out else np.zeros((0, PS), dtype=np.uint8)


def scribble(pages, dtype, fill=FILL):
    """a copy with the unspecified regions of every page set to `fill`: the gap between the data and the
    bitmap, and the bits above nr in the last bitmap byte.  Long-string pages: the bytes behind the
    characters.  Pages with nr == 0 stay 8192 zero bytes."""
    out = np.array(pages, dtype=np.uint8, copy=True).reshape(-1, PS)
    for p in out:
        nr, nnn = (int(x) for x in p[:4].view(np.uint16))
        if nr == 0:
            continue
        if dtype == VARCHAR and nr in (pc.LONG_FIRST, pc.LONG_NEXT):
            p[4 + nnn:] = fill
            continue
        nb = (nr + 7) // 8
        if dtype == VARCHAR:
            last = int(p[4:4 + 2 * nnn].view(np.uint16)[-1]) if nnn else 0
            data_end = 4 + 2 * nnn + last
        else:
            data_end = pg.HDR[dtype] + nnn * pg.WIDTH[dtype]
        p[data_end:PS - nb] = fill
        if nr % 8:
            keep = (1 << (nr % 8)) - 1
            p[PS - 1] = (int(p[PS - 1]) & keep) | (fill & ~keep & 0xFF)
    return out


# ------------------------------------------------------------------------- layouts (fixed width)
def _greedy(valid, dtype, start=0, stop=None):
    """the reference's fill rule over rows [start, stop): as many rows per page as fit"""
    stop = len(valid) if stop is None else stop
    cuts, at = [], start
    hdr, w = pg.HDR[dtype], pg.WIDTH[dtype]
    while at < stop:
        nv = nr = 0
        while at + nr < stop and nr < max_null_rows(dtype):
            v = int(valid[at + nr])
            if hdr + (nv + v) * w + (nr // 8 + 1) > PS:
                break
            nv += v
            nr += 1
        cuts.append(nr)
        at += nr
    return cuts


def _full(n, dtype):
    cap = rows_full(dtype)
    return [cap] * (n // cap) + ([n % cap] if n % cap else [])


def canonical(n, dtype, valid, seed=0):
    """the control: what pack_fixed makes"""
    if valid is None or bool(np.all(valid)):
        return _full(n, dtype)
    b = pg._page_boundaries(np.asarray(valid, bool), n, dtype)
    return np.diff(np.concatenate([b, [n]])).astype(int).tolist()


def _capped(n, dtype, valid, first=None, tail=None):
    """pages of at most rows_full rows (which fit whatever the validity), optionally after a first cut
    and before a last one"""
    cuts = [] if first is None else [first]
    body = n - sum(cuts) - (tail or 0)
    assert body >= 0
    cuts += _full(body, dtype)
    if tail is not None:
        cuts.append(tail)
    return cuts


def one_short_middle(n, dtype, valid, seed=0):
    """every page full but one in the middle, which holds rows_full - 1 rows"""
    cap = rows_full(dtype)
    assert n >= 2 * cap
    return [cap, cap - 1] + _full(n - 2 * cap + 1, dtype)


def last_exactly_full(n, dtype, valid, seed=0):
    """a short FIRST page, so that the last page is exactly full"""
    cap = rows_full(dtype)
    assert n > cap
    head = n % cap or cap
    return [head] + [cap] * ((n - head) // cap)


def last_one_row(n, dtype, valid, seed=0):
    return _capped(n, dtype, valid, tail=1)


def last_empty(n, dtype, valid, seed=0):
    return _full(n, dtype) + [0]


def empty_first(n, dtype, valid, seed=0):
    return [0] + _full(n, dtype)


def empty_middle_twice(n, dtype, valid, seed=0):
    """two nr == 0 pages in a row behind the first page"""
    c = _full(n, dtype)
    return c[:1] + [0, 0] + c[1:]


def one_row_per_page(n, dtype, valid, seed=0):
    return [1] * n


def random_cuts(n, dtype, valid, seed=0):
    """seeded, 1 .. rows_full rows per page (with a nr == 0 page now and then)"""
    rng = np.random.default_rng(seed)
    cuts, left = [], n
    while left:
        if rng.random() < 0.1:
            cuts.append(0)
        k = int(min(left, rng.integers(1, rows_full(dtype) + 1)))
        cuts.append(k)
        left -= k
    return cuts


def overfull_with_nulls(n, dtype, valid, seed=0):
    """the greedy rule on a NULL-heavy column: pages that hold MORE than rows_full rows.  Behind them
    one page of 7 rows, so that a short page sits in the middle as well."""
    assert valid is not None and not bool(np.all(valid)), "needs a column with NULLs"
    valid = np.asarray(valid, bool)
    first = _greedy(valid, dtype, 0, n)[0]
    assert first > rows_full(dtype), "not NULL-heavy enough to overfill a page"
    if first + 7 >= n:
        return [first] + ([n - first] if n > first else [])
    return [first, 7] + _greedy(valid, dtype, first + 7, n)


def all_null_max(n, dtype, valid, seed=0):
    """rows_full rows, one all-NULL page of 65 504 (INT32) / 65 472 (INT64, FP64) rows, the rest; the
    column's validity has to be False on exactly that range (null_max_valid)"""
    cap, big = rows_full(dtype), max_null_rows(dtype)
    assert n >= cap + big and valid is not None and not np.asarray(valid)[cap:cap + big].any()
    return [cap, big] + _full(n - cap - big, dtype)


def null_max_valid(n, dtype):
    v = np.ones(n, bool)
    v[rows_full(dtype):rows_full(dtype) + max_null_rows(dtype)] = False
    return v


LAYOUTS = {f.__name__: f for f in (canonical, one_short_middle, last_exactly_full, last_one_row, last_empty, empty_first,
                                   empty_middle_twice, one_row_per_page, random_cuts, overfull_with_nulls, all_null_max)}
NEEDS_NULLS = ("overfull_with_nulls", "all_null_max")


def null_heavy_valid(n, seed=0, keep=0.25):
    """a validity under which the greedy rule overfills pages: three rows in four NULL"""
    return np.random.default_rng(seed).random(n) < keep


def column(values, valid, dtype, cuts, garbage=True):
    """pl.Column of the column cut at `cuts`, its unspecified bytes scribbled over; checked to be legal
    by the strict reader and to decode to (values, valid) over the rows the pages cover"""
    pages = cut_fixed(values, valid, dtype, cuts)
    if garbage:
        pages = scribble(pages, dtype)
    col = pl.Column(dtype, pages)
    covered = sum(cuts)
    got_v, got_m = pc.check_column(col, covered)
    m = np.ones(covered, bool) if valid is None else np.asarray(valid, bool)[:covered]
    assert np.array_equal(got_m, m)
    want = np.ascontiguousarray(np.asarray(values, dtype=pg.NP_DTYPE[dtype])[:covered][m])
    assert np.ascontiguousarray(got_v[m]).tobytes() == want.tobytes()
    return col


# ---------------------------------------------------------------------------- layouts (VARCHAR)
def long_string(tag, length=LONG + 20):
    """a string above 8185 bytes that names itself"""
    head = b"<%s>" % tag
    return head + bytes((np.arange(length - len(head)) % 23 + 97).astype(np.uint8))


def _vc_greedy(strings, start, stop):
    """the reference's fill rule over rows [start, stop); a long string is a cut of one row"""
    cuts, at = [], start
    while at < stop:
        nr = nv = ch = 0
        while at + nr < stop:
            s = strings[at + nr]
            if s is not None and len(s) > pc.MAX_INLINE:
                break
            add_v, add_c = (0, 0) if s is None else (1, len(s))
            if 4 + 2 * (nv + add_v) + ch + add_c + (nr // 8 + 1) > PS:
                break
            nr, nv, ch = nr + 1, nv + add_v, ch + add_c
        if nr == 0:  # a long string
            nr = 1
        cuts.append(nr)
        at += nr
    return cuts


def varchar_layout(name, strings, seed=0):
    """-> (strings', cuts): the column `strings`, with a long string added where a chain_* layout wants
    one, and its cuts.  The fixed-width layouts that make sense for strings carry over by name; a long
    string among `strings` is a cut of its own under every layout."""
    s = list(strings)
    n = len(s)
    base = _vc_greedy(s, 0, n)
    assert len(base) >= 2, "give the layout at least two pages of strings"
    k = base[0]  # rows of the first page

    def chain(tag, length=LONG + 20):
        return long_string(tag, length)

    if name == "canonical":
        return s, base
    if name == "one_short_middle":
        assert base[1] > 1
        return s, [k, base[1] - 1] + _vc_greedy(s, k + base[1] - 1, n)
    if name == "last_one_row":
        return s, _vc_greedy(s, 0, n - 1) + [1]
    if name == "last_empty":
        return s, base + [0]
    if name == "empty_first":
        return s, [0] + base
    if name == "empty_middle_twice":
        return s, base[:1] + [0, 0] + base[1:]
    if name == "one_row_per_page":
        return s, [1] * n
    if name == "random_cuts":
        rng = np.random.default_rng(seed)
        cuts, at = [], 0
        while at < n:
            if rng.random() < 0.1:
                cuts.append(0)
            room = _vc_greedy(s, at, n)[0]
            take = int(rng.integers(1, room + 1))
            cuts.append(take)
            at += take
        return s, cuts
    if name == "chain_first":
        s = [chain(b"first")] + s
        return s, [1] + base
    if name == "chain_last":
        s = s + [chain(b"last", 2 * pc.LONG_PIECE + 5)]  # three pieces
        return s, base + [1]
    if name == "chain_between_empty_pages":
        s = s[:k] + [chain(b"between")] + s[k:]
        return s, [k, 0, 1, 0] + base[1:]
    if name == "two_chains_adjacent":
        s = s[:k] + [chain(b"one"), chain(b"two", pc.LONG_PIECE + 1)] + s[k:]
        return s, [k, 1, 1] + base[1:]
    if name == "chain_then_one_row_page":
        s = s[:k] + [chain(b"then"), b"lonely"] + s[k:]
        return s, [k, 1, 1] + base[1:]
    raise KeyError(name)


VARCHAR_ONLY = ("chain_first", "chain_last", "chain_between_empty_pages", "two_chains_adjacent", "chain_then_one_row_page")
VARCHAR_LAYOUTS = ("canonical", "one_short_middle", "last_one_row", "last_empty", "empty_first", "empty_middle_twice",
                   "one_row_per_page", "random_cuts") + VARCHAR_ONLY


def varchar_column(strings, cuts, garbage=True):
    """pl.Column of the strings cut at `cuts`; checked like `column`"""
    pages = cut_varchar(strings, cuts)
    if garbage:
        pages = scribble(pages, VARCHAR)
    col = pl.Column(VARCHAR, pages)
    covered = sum(cuts)
    assert pc.check_column(col, covered) == list(strings)[:covered]
    return col


def page_first_last_rows(col):
    """(first row, last row) of every page of a column that holds rows; a long string's chain counts as
    one page of one row"""
    nr = np.ascontiguousarray(col.pages).reshape(-1, PS)[:, :2].copy().view(np.uint16)[:, 0].astype(np.int64)
    rows = np.where(nr == pc.LONG_FIRST, 1, np.where(nr == pc.LONG_NEXT, 0, nr))
    base = np.concatenate([[0], np.cumsum(rows)])
    return [(int(base[i]), int(base[i + 1]) - 1) for i in range(len(rows)) if rows[i]]


# ------------------------------------------------------------------------ single cleared bits
def single_null_positions(dtype, nr):
    """rows at which one cleared validity bit tells the bitmap branches apart: around the byte, halfword,
    dword, wave (64) and workgroup-round (256) boundaries, and around the end of the page"""
    want = [0, 1, 7, 8, 15, 16, 31, 32, 63, 64, 255, 256, nr - 17, nr - 16, nr - 9, nr - 8, nr - 1]
    return sorted({r for r in want if 0 <= r < nr})


# (dtype, rows of the page that carries the cleared bit, the bitmap branch of k_page_headers it takes)
#   1984 INT32 rows: 248 bitmap bytes at a dword boundary, nr % 32 == 0       -> dword loads
#   1007 INT64 rows: 126 bitmap bytes at a halfword boundary                   -> halfword loads
#   1001 INT32 rows: 126 bitmap bytes, an even count at an even offset         -> halfword loads as well
#    999 INT32 rows: 125 bitmap bytes, an odd count at an odd offset           -> byte by byte
SINGLE_NULL_SHAPES = ((INT32, 1984, "dword"), (INT64, 1007, "halfword"), (INT32, 1001, "halfword"), (INT32, 999, "byte"))


def bitmap_branch(nr):
    """the branch of k_page_headers (csrc/rj_pages.hip) a page of nr rows takes"""
    nb = (nr + 7) // 8
    boff = PS - nb
    if nr % 32 == 0 and boff % 4 == 0:
        return "dword"
    if boff % 2 == 0 and nb % 2 == 0:
        return "halfword"
    return "byte"


# ------------------------------------------------------------------------------ shared cases
def is_regular(cuts, valid, dtype, num_rows):
    """the library's rule for a column it addresses in place: every page but the last full, the last
    one not empty, no NULL, rows adding up (csrc/rj_table.hip)"""
    cap = rows_full(dtype)
    return (len(cuts) > 0 and all(c == cap for c in cuts[:-1]) and 0 < cuts[-1] <= cap and sum(cuts) == num_rows
            and (valid is None or bool(np.all(np.asarray(valid)[:num_rows]))))


def fixed_rows(name, dtype):
    """rows of the column a fixed-width layout is shown on: two to six pages, odd counts"""
    if name == "all_null_max":
        return max_null_rows(dtype) + 2 * rows_full(dtype)
    if name == "overfull_with_nulls":
        return 12_000
    if name == "one_row_per_page":
        return 2_050
    return {INT32: 3 * 1984 + 137, INT64: 4 * 1007 + 137, FP64: 4 * 1007 + 137}[dtype]


def fixed_valid(name, dtype, n, seed=0):
    """the validity a layout needs (None: no NULLs, so that the canonical control is addressed in place)"""
    if name == "all_null_max":
        return null_max_valid(n, dtype)
    if name == "overfull_with_nulls":
        return null_heavy_valid(n, seed)
    return None


def typed(dtype, ints):
    """integers as values of the type, exactly (FP64: whole numbers and halves stay distinct keys)"""
    a = np.asarray(ints, dtype=np.int64)
    if dtype == INT32:
        return (a * 7 - 11).astype(np.int32)
    if dtype == INT64:
        return a * 1_000_003 - (1 << 40)
    return a.astype(np.float64) * 0.5 - 3.0


class Col:
    """one logical column and the cuts it is fed with"""

    def __init__(self, dtype, values, valid=None, layout="canonical", seed=0, cuts=None):
        self.dtype, self.values, self.valid, self.layout = dtype, values, valid, layout
        if dtype == VARCHAR:
            self.values, self.cuts = varchar_layout(layout, values, seed) if cuts is None else (list(values), cuts)
        else:
            self.cuts = LAYOUTS[layout](len(values), dtype, valid, seed) if cuts is None else cuts

    def __len__(self):
        return len(self.values)

    def canonical_spec(self):
        return (VARCHAR, self.values) if self.dtype == VARCHAR else (self.dtype, self.values, self.valid)

    def cut_column(self):
        if self.dtype == VARCHAR:
            return varchar_column(self.values, self.cuts)
        return column(self.values, self.valid, self.dtype, self.cuts)

    def regular(self, num_rows):
        return self.dtype != VARCHAR and is_regular(self.cuts, self.valid, self.dtype, num_rows)


def tables(cols, num_rows=None):
    """-> (the table in the columns' layouts, the same table as pl.make_table packs it)"""
    n = len(cols[0]) if num_rows is None else num_rows
    assert all(len(c) == len(cols[0]) for c in cols)
    cut = pl.ColumnarTable(n, [c.cut_column() for c in cols])
    canon = pl.make_table([c.canonical_spec() for c in cols])
    assert canon.num_rows == len(cols[0])
    return cut, canon


def scan_all(p, table_id, t):
    return p.new_scan_node(table_id, [(i, c.type) for i, c in enumerate(t.columns)])


def join_plan(lt, rt, la=0, ra=0, build_left=True, kind="join", outs=None):
    """Scan(lt) <kind> Scan(rt) on lt.la = rt.ra, every column of both out (or `outs`)"""
    p = pl.Plan()
    ls, rs = scan_all(p, 0, lt), scan_all(p, 1, rt)
    types = [c.type for c in lt.columns] + [c.type for c in rt.columns]
    outs = list(range(len(types))) if outs is None else outs
    mk = {"join": p.new_join_node, "semi": p.new_semi_join_node, "anti": p.new_anti_join_node,
          "outer": p.new_outer_join_node, "full": p.new_full_outer_join_node}[kind]
    p.root = mk(build_left, ls, rs, la, ra, [(o, types[o]) for o in outs])
    p.new_input(lt)
    p.new_input(rt)
    return p


def scan_plan(t):
    p = pl.Plan()
    p.root = scan_all(p, 0, t)
    p.new_input(t)
    return p


def with_inputs(p, inputs):
    """the same plan over other tables"""
    q = pl.Plan()
    q.nodes, q.root, q.inputs = p.nodes, p.root, list(inputs)
    return q


def layout_join_case(name, dtype, seed=0):
    """The case of one fixed-width layout: a probe table whose key (column 0) and payload (column 1) are
    cut with the layout and whose row ids (column 2) with random cuts, and a build table of 4000 rows
    (the broadcast join's size) whose key is cut at random, whose payload of the type (column 1) is cut
    with the layout as well (all_null_max, which 4000 rows cannot show, aside), and whose INT64 payload
    ends in a page of one row: the row bases differ from column to column.  The control `canonical` has every column as
    pl.make_table packs it.
    -> (plan over the cut tables, plan over the canonical tables, columns of both tables)"""
    rng = np.random.default_rng([seed, dtype, sorted(LAYOUTS).index(name)])
    n, nb = fixed_rows(name, dtype), 4000
    control = name == "canonical"
    other = (lambda lay: "canonical") if control else (lambda lay: lay)
    bkeys = typed(dtype, rng.permutation(nb))
    bvalid = fixed_valid(name, dtype, nb, seed + 1) if name == "overfull_with_nulls" else None
    build = [Col(dtype, bkeys, None, other("random_cuts"), seed + 2),
             Col(dtype, typed(dtype, rng.integers(0, 1 << 20, nb)), bvalid, "last_one_row" if name == "all_null_max" else name, seed),
             Col(INT64, rng.integers(-(1 << 62), 1 << 62, nb), None, other("last_one_row"))]
    pvalid = fixed_valid(name, dtype, n, seed + 3)
    probe = [Col(dtype, typed(dtype, rng.integers(0, nb + 500, n)), pvalid, name, seed),
             Col(dtype, typed(dtype, rng.integers(0, 1 << 20, n)), pvalid, name, seed),
             Col(INT32, np.arange(n, dtype=np.int32), None, other("random_cuts"), seed + 4)]
    bt, bt0 = tables(build)
    pt, pt0 = tables(probe)
    p = join_plan(bt, pt)
    return p, with_inputs(p, [bt0, pt0]), (build, probe)
