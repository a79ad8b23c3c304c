"""The library's key hashes, restated in numpy (host logic; lets tests check device output).

INT32 keys use murmur3's fmix32, INT64/FP64 keys fmix64 (the reference hashes with fmix64,
src/execute.cpp:21-27; the choice of hash is not observable in results).  Both are bijections,
which is why partitions can store hashed keys and un-hash on emit (csrc/rj_tuple_util.hpp).
Radix digits come from the LOW bits, LDS slot bits from the bits above them, and the sharding
digit (which rank owns a key) from the TOP bits.
"""
import numpy as np

M32 = np.uint32(0xFFFFFFFF)


def fmix32(k):
    h = np.asarray(k).astype(np.uint32, copy=True)
    with np.errstate(over="ignore"):
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x85EBCA6B)
        h ^= h >> np.uint32(13)
        h *= np.uint32(0xC2B2AE35)
        h ^= h >> np.uint32(16)
    return h


def unfmix32(h):
    h = np.asarray(h).astype(np.uint32, copy=True)
    with np.errstate(over="ignore"):
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x7ED1B41D)
        h ^= (h >> np.uint32(13)) ^ (h >> np.uint32(26))
        h *= np.uint32(0xA5CB9243)
        h ^= h >> np.uint32(16)
    return h


def owner_rank(keys_int32, n_ranks):
    """Which rank owns a key in the sharded join: the top log2(n_ranks) hash bits."""
    rb = (n_ranks - 1).bit_length()
    if rb == 0:
        return np.zeros(np.asarray(keys_int32).shape[0], dtype=np.int64)
    return (fmix32(np.asarray(keys_int32).view(np.uint32)) >> np.uint32(32 - rb)).astype(np.int64)


M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def fmix64(k):
    """murmur3 fmix64 over uint64 (INT64 keys, FP64 keys by bit pattern; csrc/rj_tuple_util.hpp)."""
    h = np.asarray(k).astype(np.uint64, copy=True)
    with np.errstate(over="ignore"):
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xFF51AFD7ED558CCD)
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xC4CEB9FE1A85EC53)
        h ^= h >> np.uint64(33)
    return h


def unfmix64(h):
    h = np.asarray(h).astype(np.uint64, copy=True)
    with np.errstate(over="ignore"):
        h ^= h >> np.uint64(33)
        h *= np.uint64(0x9CB4B2F8129337DB)  # inverse of 0xc4ceb9fe1a85ec53 mod 2^64
        h ^= h >> np.uint64(33)
        h *= np.uint64(0x4F74430C22A54005)  # inverse of 0xff51afd7ed558ccd mod 2^64
        h ^= h >> np.uint64(33)
    return h


def key_hash(keys, wide):
    """The device hash of join keys: fmix32 of an INT32 key's bits (wide=False), fmix64 of an
    INT64 key or of an FP64 key's bit pattern (wide=True)."""
    k = np.ascontiguousarray(keys)
    if not wide:
        return fmix32(k.view(np.uint32))
    return fmix64(k.view(np.uint64))


def is_nan_bits(bits):
    """FP64 bit patterns that are NaN (exponent all ones, mantissa non-zero)."""
    b = np.asarray(bits).astype(np.uint64)
    return ((b & np.uint64(0x7FF0000000000000)) == np.uint64(0x7FF0000000000000)) & \
        ((b & np.uint64(0x000FFFFFFFFFFFFF)) != np.uint64(0))


def keys_with_hash_bits(n, dtype, value=0, mask=0, owner=None, n_ranks=1, rng=None):
    """n distinct keys whose hash carries chosen bits, computed through the inverse mixer (no search).

    dtype: np.int32 (fmix32), np.int64 or np.float64 (fmix64 of the bit pattern).  Every key's hash
    h has ``h & mask == value & mask``; with ``owner`` set, its top log2(n_ranks) bits equal
    ``owner`` as well (the rank of a sharded join, ``owner_rank``).  All other bits vary.  FP64
    results whose bit pattern is a NaN are left out (they never match, so they would not carry
    the construction into a join).  Raises ValueError when fewer than n such keys exist."""
    dtype = np.dtype(dtype)
    width = 32 if dtype == np.int32 else 64
    full = (1 << width) - 1
    fixed_mask, fixed_val = int(mask) & full, int(value) & int(mask) & full
    if owner is not None and n_ranks > 1:
        rb = (n_ranks - 1).bit_length()
        top = ((1 << rb) - 1) << (width - rb)
        fixed_mask |= top
        fixed_val = (fixed_val & ~top) | (int(owner) << (width - rb))
    free = [b for b in range(width) if not (fixed_mask >> b) & 1]
    rng = rng if rng is not None else np.random.default_rng(0)
    ut = np.uint32 if width == 32 else np.uint64
    if len(free) <= 20:
        # few free bits: enumerate them all, in random order
        if (1 << len(free)) < n:
            raise ValueError(f"only {1 << len(free)} hashes carry these bits, {n} asked for")
        idx = rng.permutation(1 << len(free)).astype(np.uint64)
        h = np.full(idx.shape, fixed_val, dtype=np.uint64)
        for i, b in enumerate(free):
            h |= ((idx >> np.uint64(i)) & np.uint64(1)) << np.uint64(b)
        h = h.astype(ut)
    else:
        h = np.empty(0, dtype=ut)
        want = n
        while True:
            r = rng.integers(0, 1 << 63, size=want + want // 4 + 16, dtype=np.uint64) << np.uint64(1)
            r ^= rng.integers(0, 2, size=r.shape, dtype=np.uint64)
            r = (r & np.uint64(~fixed_mask & full)) | np.uint64(fixed_val)
            h = np.concatenate([h, r.astype(ut)])
            _, first = np.unique(h, return_index=True)
            h = h[np.sort(first)]
            if dtype == np.float64:
                h = h[~is_nan_bits(unfmix64(h))]
            if h.shape[0] >= n:
                break
            want = n - h.shape[0]
    if width == 32:
        keys = unfmix32(h).view(np.int32)
    else:
        bits = unfmix64(h)
        if dtype == np.float64:
            bits = bits[~is_nan_bits(bits)]
            if bits.shape[0] < n:
                raise ValueError(f"only {bits.shape[0]} non-NaN keys carry these bits, {n} asked for")
        keys = bits.view(np.int64 if dtype == np.int64 else np.float64)
    return np.ascontiguousarray(keys[:n])
