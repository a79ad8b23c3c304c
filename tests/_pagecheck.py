"""A strict reader of ColumnarTable columns: the page format restated as rules, each with a name.

Independent of pyrj.pages' decoders (only the constants PAGE_SIZE, HDR and WIDTH come from there).
Written from the reference's format: the writer ColumnInserter (include/plan.h) and Table::to_columnar,
the reader Table::from_columnar (src/build_table.cpp).  Where the reference's reader trusts a page
(it never compares the header's non-null count with the bitmap, it lets NULL rows run past num_rows,
it follows whatever offsets a VARCHAR page holds), this one checks.

A fixed-width page (8192 bytes): u16 row count `nr` at 0, u16 non-null count `nnn` at 2, the non-null
values densely from byte 4 (INT32) / 8 (INT64, FP64) in row order, and in the LAST ceil(nr / 8) bytes a
bitmap, bit i (LSB first) = row i is not NULL.
A VARCHAR page: the same header and bitmap; from byte 4 `nnn` u16 END offsets, then the characters,
string k = characters [offset[k-1], offset[k]) counted from the end of the offset array.  nr == 0xffff is
a page holding the first piece of ONE long string (u16 length at 2, characters from 4), nr == 0xfffe a
further piece of the string before it.

Rules (PageFormatError.rule_name):
  row_limit        nr <= 65504 (what an all-NULL page can hold; 0xffff / 0xfffe mark long strings)
  nnn_popcount     nnn == popcount(bitmap[0:nr])
  fit              fixed: hdr + nnn * width + ceil(nr / 8) <= 8192
                   VARCHAR: 4 + 2 * nnn + last offset + ceil(nr / 8) <= 8192
  offsets_ordered  the nnn end offsets of a VARCHAR page do not decrease
  long_orphan      a 0xfffe page follows a 0xffff or 0xfffe page
  long_length      the length field of a long-string page is in 1 .. 8188
  long_piece       every piece of a chain but the last holds 8188 characters
  long_total       a chain holds more than 8185 characters (a shorter string fits a normal page, and
                   neither encoder makes a chain for it)
  row_total        the rows of all pages add up to exactly num_rows
A page with nr == 0 is legal (the reference's reader accepts it); scan_column counts them.  Bits above
nr in the last bitmap byte and the bytes between the data and the bitmap are unspecified: not checked.
"""
import numpy as np

from pyrj.pages import HDR, PAGE_SIZE, WIDTH

INT32, INT64, FP64, VARCHAR = 0, 1, 2, 3
_NP = {INT32: np.dtype("<i4"), INT64: np.dtype("<i8"), FP64: np.dtype("<f8")}
MAX_ROWS = (PAGE_SIZE - 4) * 8            # 65504: an all-NULL page of a 4-byte header
LONG_FIRST, LONG_NEXT = 0xFFFF, 0xFFFE
LONG_PIECE = PAGE_SIZE - 4                # 8188 characters per long-string page
MAX_INLINE = PAGE_SIZE - 7                # 8185: the longest string of a normal page
RULES = ("row_limit", "nnn_popcount", "fit", "offsets_ordered", "long_orphan", "long_length", "long_piece",
         "long_total", "row_total")


class PageFormatError(Exception):
    def __init__(self, page_index, rule_name, detail=""):
        assert rule_name in RULES, rule_name
        super().__init__(f"page {page_index}: rule {rule_name}: {detail}")
        self.page_index, self.rule_name, self.detail = page_index, rule_name, detail


def _pages(col):
    pages = np.ascontiguousarray(col.pages, dtype=np.uint8)
    if pages.size % PAGE_SIZE:
        raise ValueError("a column is a whole number of pages")
    return pages.reshape(-1, PAGE_SIZE)


def _header(pages):
    h = pages[:, :4].astype(np.uint32)
    return h[:, 0] | (h[:, 1] << 8), h[:, 2] | (h[:, 3] << 8)


def _bits(page, nr):
    """validity of the page's nr rows, from the tail of the page"""
    nb = (nr + 7) // 8
    return np.unpackbits(page[PAGE_SIZE - nb:], bitorder="little")[:nr].astype(bool)


def _row_total(n_pages, rows, num_rows):
    if rows != num_rows:
        raise PageFormatError(n_pages - 1, "row_total", f"the pages hold {rows} rows, the table declares {num_rows}")


def _scan_fixed(col, num_rows):
    dt, hdr, w = _NP[col.type], HDR[col.type], WIDTH[col.type]
    pages = _pages(col)
    nr_all, nnn_all = _header(pages)
    vals, valid, empty = [], [], 0
    for pi in range(pages.shape[0]):
        nr, nnn = int(nr_all[pi]), int(nnn_all[pi])
        if nr > MAX_ROWS:
            raise PageFormatError(pi, "row_limit", f"nr {nr} > {MAX_ROWS}")
        if nr == 0:
            empty += 1
        bits = _bits(pages[pi], nr)
        pop = int(bits.sum())
        if nnn != pop:
            raise PageFormatError(pi, "nnn_popcount", f"header says {nnn} non-null of {nr} rows, the bitmap holds {pop}")
        nb = (nr + 7) // 8
        if hdr + nnn * w + nb > PAGE_SIZE:
            raise PageFormatError(pi, "fit", f"{hdr} + {nnn} * {w} + {nb} > {PAGE_SIZE}")
        v = np.zeros(nr, dtype=dt)
        v[bits] = pages[pi, hdr:hdr + nnn * w].view(dt)
        vals.append(v)
        valid.append(bits)
    rows = int(nr_all.sum())
    _row_total(pages.shape[0], rows, num_rows)
    if not vals:
        return (np.zeros(0, dtype=dt), np.zeros(0, dtype=bool)), empty
    return (np.concatenate(vals), np.concatenate(valid)), empty


def _scan_varchar(col, num_rows):
    pages = _pages(col)
    nr_all, n2_all = _header(pages)
    out, empty = [], 0
    chain = None  # the open long string: [pieces' lengths], and its pieces' bytes
    chain_bytes = []

    def close_chain(last_page):
        nonlocal chain
        if chain is None:
            return
        total = sum(chain)
        if total <= MAX_INLINE:
            raise PageFormatError(last_page, "long_total", f"a chain of {len(chain)} page(s) holds {total} characters, which fit a normal page")
        out.append(b"".join(chain_bytes))
        chain = None
        chain_bytes.clear()

    for pi in range(pages.shape[0]):
        page, nr, n2 = pages[pi], int(nr_all[pi]), int(n2_all[pi])
        if nr in (LONG_FIRST, LONG_NEXT):
            if nr == LONG_FIRST:
                close_chain(pi - 1)
                chain = []
            elif chain is None:
                raise PageFormatError(pi, "long_orphan", "a 0xfffe page that follows no 0xffff / 0xfffe page")
            elif chain[-1] != LONG_PIECE:
                raise PageFormatError(pi - 1, "long_piece", f"a piece of {chain[-1]} characters is followed by another")
            if not 1 <= n2 <= LONG_PIECE:
                raise PageFormatError(pi, "long_length", f"length {n2} outside 1 .. {LONG_PIECE}")
            chain.append(n2)
            chain_bytes.append(page[4:4 + n2].tobytes())
            continue
        close_chain(pi - 1)
        if nr > MAX_ROWS:
            raise PageFormatError(pi, "row_limit", f"nr {nr} > {MAX_ROWS}")
        if nr == 0:
            empty += 1
        bits = _bits(page, nr)
        pop = int(bits.sum())
        if n2 != pop:
            raise PageFormatError(pi, "nnn_popcount", f"header says {n2} non-null of {nr} rows, the bitmap holds {pop}")
        nb = (nr + 7) // 8
        if 4 + 2 * n2 + nb > PAGE_SIZE:
            raise PageFormatError(pi, "fit", f"4 + 2 * {n2} + {nb} > {PAGE_SIZE}: the offsets alone reach the bitmap")
        ends = page[4:4 + 2 * n2].view("<u2").astype(np.int64)
        if n2 > 1 and bool((np.diff(ends) < 0).any()):
            k = int(np.nonzero(np.diff(ends) < 0)[0][0])
            raise PageFormatError(pi, "offsets_ordered", f"offset {k + 1} is {int(ends[k + 1])} after {int(ends[k])}")
        last = int(ends[-1]) if n2 else 0
        if 4 + 2 * n2 + last + nb > PAGE_SIZE:
            raise PageFormatError(pi, "fit", f"4 + 2 * {n2} + {last} + {nb} > {PAGE_SIZE}")
        base = 4 + 2 * n2
        text = page[base:base + last].tobytes()
        begs = [0] + ends[:-1].tolist()
        strs = iter([text[b:e] for b, e in zip(begs, ends.tolist())])
        out.extend([next(strs) if b else None for b in bits.tolist()])
    close_chain(pages.shape[0] - 1)
    _row_total(pages.shape[0], len(out), num_rows)
    return out, empty


def scan_column(col, num_rows):
    """-> (decoded column, number of pages with nr == 0); raises PageFormatError."""
    if col.type == VARCHAR:
        return _scan_varchar(col, int(num_rows))
    return _scan_fixed(col, int(num_rows))


def check_column(col, num_rows):
    """-> (values[num_rows], valid[num_rows]) of a fixed-width column (values of NULL rows are zero), or
    a list of `bytes | None` of a VARCHAR column.  Raises PageFormatError(page_index, rule_name, detail)
    at the first page that breaks a rule."""
    return scan_column(col, num_rows)[0]


def check_table(t):
    """check_column over every column -> the decoded columns, in pl.decode_table's shape"""
    return [check_column(c, t.num_rows) for c in t.columns]


def same_as(decoded, other):
    """Do two decodes of one table (check_table / pl.decode_table) agree?  Values are compared on the
    valid rows, by bit pattern (NaN payloads, -0.0)."""
    if len(decoded) != len(other):
        return False
    for a, b in zip(decoded, other):
        if isinstance(a, list) != isinstance(b, list):
            return False
        if isinstance(a, list):
            if a != b:
                return False
            continue
        (va, ma), (vb, mb) = a, b
        ma, mb = np.asarray(ma, dtype=bool), np.asarray(mb, dtype=bool)
        if ma.shape != mb.shape or not np.array_equal(ma, mb):
            return False
        va, vb = np.ascontiguousarray(np.asarray(va)[ma]), np.ascontiguousarray(np.asarray(vb)[mb])
        if va.dtype.itemsize != vb.dtype.itemsize or va.tobytes() != vb.tobytes():
            return False
    return True


def canonical_rows(decoded):
    """The sorted row multiset of decoded columns, in the shape of pl.canonical_rows (None = NULL, a
    double as ("f64", its bits)) — so that a strict decode compares with a reference table's rows."""
    cols = []
    for d in decoded:
        if isinstance(d, list):
            cols.append(d)
            continue
        v, m = d
        ints = (np.ascontiguousarray(v).view(np.int64) if v.dtype.kind == "f" else v).tolist()
        if v.dtype.kind == "f":
            cols.append([("f64", x) if ok else None for x, ok in zip(ints, m.tolist())])
        else:
            cols.append([x if ok else None for x, ok in zip(ints, m.tolist())])
    rows = list(zip(*cols))
    return sorted(rows, key=lambda r: tuple((2, 0) if x is None else ((1, x[1]) if isinstance(x, tuple) else (0, x)) for x in r))


def strict_rows(t):
    """check_table + agreement with pyrj's decode -> canonical rows of the strict decode"""
    from pyrj import plan as pl

    dec = check_table(t)
    assert same_as(dec, pl.decode_table(t)), "the strict reader and pyrj.pages decode different content"
    return canonical_rows(dec)
