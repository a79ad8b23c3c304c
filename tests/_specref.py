"""A host model of the speculative first radix pass: which rows the sample counts, the capacity every output
sub-range gets, how many tuples it then receives, and hence whether the side falls back to the exact path.

Plain numpy and integers.  Nothing here is taken from the device code; every piece restates a COMMENT of it:

  hash and digit   pyrj.hashing.key_hash (fmix32 of an INT32 key, fmix64 of an INT64 key or of an FP64 key's bit
                   pattern), its low 32 bits; the first pass takes the low pbits[0] bits at shift 0
                   (rj_device.hpp, PassParams::shift: "digit = (word0 >> shift) & (F-1)").  Rows that hold no tuple:
                   NULL keys, and NaN for FP64 (rj_partition.hip, above k_pass_sample: "NULL keys, rows behind the
                   relation's end and hashing are the scatter's"; SrcLoader::hash_keys: "NaN never matches")
  bits per pass    rj_radix_plan.cpp, radix_plan: passes = ceil(bits / 9), the bits split evenly, the first passes
                   take the remainder (pbits)
  tiles, groups    tile t = rows [16384 t, 16384 (t + 1)); a group is tiles_per_group consecutive tiles, workgroup g
                   takes group g and "counts and writes into sub-range g & 7" (rj_device.hpp, PassParams::xcd_log2);
                   tiles_per_group(n, 4096) is radix_tiles_per_group, RJ_TUNE_TPG1 replaces it.  Bin of a tuple:
                   (digit << 3) | (group & 7) (above k_pass_sample: "hist[(d << 3) | (blockIdx.x & 7)]")
  sample slice     above k_pass_sample: "of every tile only one slice of PT_TILE >> sample_log2 consecutive rows is
                   read ... The slice's place inside its tile moves with the tile index by 7 slices ... In a partial
                   last tile the slice ends with the tile at the latest (its place is min(that place, rows - slice));
                   a tile of no more rows than a slice is read whole".  (The comment used to say only "sampled from
                   its first rows on", which holds for rows <= slice; it was brought in line with the kernel when
                   this model was written, and the phase_*_tail cases of test_gpu_spec_model.py pin the clamp.)
  capacity         above k_spec_caps: "cap = 2^s (c + z sqrt(c + 1) + z^2 / 2) tuples, rounded up to a multiple of
                   32", start = exclusive scan in bin order, "Nothing reaches beyond cap_max ... a sub-range that
                   would is cut there".  z arrives as a float (launch_spec_caps' parameter), so it is rounded to
                   float32 first; the expression itself is evaluated in double
  cap_max          rj_radix_plan.cpp, radix_cap_bound and `spec`: C = tiles * (16384 >> s) sampled positions, B = 8 <<
                   pbits[0] sub-ranges, bound = 2^s (C + z sqrt(B (C + B)) + z^2 / 2 B) + 32 B, rounded up to a
                   multiple of 256
  the flag         rj_device.hpp, SpecParams::cursor: a tile reserves its c tuples with one add whatever comes back,
                   and the run fits iff the room before it was >= c.  Reservations only ever add: a sub-range whose
                   tuples all fit never sees room < c, one whose tuples do not fit sees it at the latest in the
                   reservation that passes its capacity — whatever the order of the atomics.  So
                   overflows == any(count > cap), exactly.

The near-boundary band.  The device evaluates the capacity in double too, but its sqrt and a fused multiply-add
may differ from numpy's in the last place, which moves a capacity by one step of 32 when 2^s x lies within that of
an integer.  A prediction is therefore only given when it does not hang on one step: Prediction.overflows is
  True   when some sub-range holds more than cap + 32 tuples (it overflows whichever way its capacity is rounded),
  False  when every sub-range holds at most cap - 32,
  None   ("either") otherwise: some sub-range has cap - 32 < count <= cap + 32 and none is surely too small.
No committed case may answer None (tests/test_spec_model.py).  With z = 0 the capacity is 32 c >> (5 - s), integer
arithmetic that no rounding touches (x = c exactly, ldexp and ceil are exact): the band is empty there and
overflows == any(count > cap) as it stands — every forced-overflow case has sub-ranges all around their capacity."""
import math
from dataclasses import dataclass

import numpy as np

from pyrj import hashing
from pyrj import plan as pl

PT_TILE = 16384
MAXBITS = 9  # radix bits per pass


def pass_bits(bits):
    """Radix bits of each pass."""
    passes = max(1, -(-bits // MAXBITS))
    pb = [bits // passes] * passes
    for i in range(bits % passes):
        pb[i] += 1
    return pb


def tiles_per_group(n, target_groups=4096):
    k = -(-n // (PT_TILE * target_groups))
    return min(max(k, 1), 8)


def slice_of(tile, s, rows=PT_TILE):
    """-> (first row inside the tile, rows read) of tile `tile`'s sample slice; `rows`: rows the tile holds."""
    width = PT_TILE >> s
    place = (7 * tile * width) % PT_TILE
    if rows > width:
        return min(place, rows - width), width
    return 0, rows


def sampled(n, s):
    """Boolean mask over n rows: the rows the sample reads."""
    m = np.zeros(n, bool)
    for t in range(-(-n // PT_TILE)):
        at, cnt = slice_of(t, s, min(PT_TILE, n - t * PT_TILE))
        m[t * PT_TILE + at:t * PT_TILE + at + cnt] = True
    return m


def capacity(c, s, z_tenths):
    """Capacity of a sub-range whose sample holds c tuples (numpy array of counts -> int64 array)."""
    z = float(np.float32(z_tenths / 10.0))
    c = np.asarray(c, dtype=np.float64)
    x = c + z * np.sqrt(c + 1.0) + 0.5 * z * z
    t = np.ceil(np.ldexp(x, s)).astype(np.int64)
    return (t + 31) & ~np.int64(31)


def cap_max(n, bits0, s, z_tenths):
    """The tuples the host makes room for: its bound on the sum of the capacities."""
    z = z_tenths / 10.0
    B = float(8 << bits0)
    C = float(-(-n // PT_TILE)) * float(PT_TILE >> s)
    bound = math.ldexp(C + z * math.sqrt(B * (C + B)) + 0.5 * z * z * B, s) + 32.0 * B
    return (int(math.ceil(bound)) + 255) & ~255


def digits(keys, valid, kt, bits0):
    """-> (first-pass digit of every row, rows that hold a tuple)"""
    keys = np.ascontiguousarray(keys)
    ok = np.ones(keys.shape[0], bool) if valid is None else np.asarray(valid, bool).copy()
    h = hashing.key_hash(keys, kt != pl.INT32)
    if kt == pl.FP64:
        ok &= ~hashing.is_nan_bits(keys.view(np.uint64))
    d = (h & type(h.flat[0])((1 << bits0) - 1)).astype(np.int64)
    return d, ok


@dataclass
class Prediction:
    sample: np.ndarray    # per sub-range (digit << 3) | x: tuples the sample counted
    cap: np.ndarray       # its capacity
    count: np.ndarray     # the tuples the scatter sends there
    overflows: object     # True / False / None ("either": see the module docstring)

    @property
    def fullest(self):
        return float((self.count / np.maximum(self.cap, 1)).max())


def predict(keys, valid, kt, bits, s=5, z_tenths=60, tpg=0):
    """One side of a join.  bits: the plan's radix bits (two passes); tpg: RJ_TUNE_TPG1, 0 = the default."""
    n = int(np.asarray(keys).shape[0])
    bits0 = pass_bits(bits)[0]
    nb = 8 << bits0
    d, ok = digits(keys, valid, kt, bits0)
    g = (np.arange(n) // PT_TILE) // (tpg or tiles_per_group(n))
    sub = (d << 3) | (g & 7)
    count = np.bincount(sub[ok], minlength=nb)
    sample = np.bincount(sub[ok & sampled(n, s)], minlength=nb)
    full = capacity(sample, s, z_tenths)
    end = np.minimum(np.cumsum(full), cap_max(n, bits0, s, z_tenths))  # nothing reaches beyond cap_max
    cap = end - np.concatenate([[0], end[:-1]])
    if z_tenths == 0:
        over = bool((count > cap).any())
    elif (count > cap + 32).any():
        over = True
    elif (count <= cap - 32).all():
        over = False
    else:
        over = None
    return Prediction(sample, cap, count, over)


def plan_sides(p):
    """The two inputs of a Scan JOIN Scan plan -> [(keys, valid, key type)] in input order (key = column 0)."""
    out = []
    for t in p.inputs[:2]:
        kt = t.columns[0].type
        k, v = pl.decode_table(t)[0]
        out.append((np.asarray(k), np.asarray(v, bool), kt))
    return out


def predict_plan(p, bits, s=5, z_tenths=60, tpg=0):
    """-> the predictions for input 0 and input 1 of a two-input join plan."""
    return [predict(k, v, kt, bits, s, z_tenths, tpg) for k, v, kt in plan_sides(p)]
