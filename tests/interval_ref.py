"""The bootstrap interval of a pair's ANI (include/pyskani_amd.h, psk_ci_opts; csrc/interval.hip), restated in plain numpy: the hash, the draw stream, the
bounds. Used by test_interval_cpu.py (against the oracle's hash, the library's host-side draw and the oracle's chunks; no GPU) and test_gpu_interval.py.

For resample b in [0, B) and draw j in [0, m):
    h   = mm_hash64(seed + (b << 32) + (j >> 1))                (64-bit wrap-around)
    w   = high word of h for an odd j, low word for an even one
    idx = (w * m) >> 32
    mean_b = (v[idx_0] + ... + v[idx_(m-1)]) / m                (double, added in draw order)
and, with s the B means in ascending order, lo = float32(s[B // 20]), hi = float32(s[B - 1 - B // 20])."""
import numpy as np

import tier_cases as T

DEFAULT_ITERATIONS = 100
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def mm_hash64(key):
    """skani's mm_hash64 (minimap2's invertible mix) on a uint64 array"""
    u = np.uint64
    with np.errstate(over="ignore"):
        k = np.asarray(key, dtype=np.uint64).copy()
        k = ~(k + (k << u(21)))
        k = k ^ (k >> u(24))
        k = (k + (k << u(3))) + (k << u(8))
        k = k ^ (k >> u(14))
        k = (k + (k << u(2))) + (k << u(4))
        k = k ^ (k >> u(28))
        k = k + (k << u(31))
    return k


def ranks(iterations=0):
    """(B, lo rank, hi rank)"""
    b = iterations if iterations else DEFAULT_ITERATIONS
    return b, b // 20, b - 1 - b // 20


def draw(seed, b, j, m):
    """idx of draw j of resample b among m values, one at a time (any m below 2^32)"""
    key = (seed + (b << 32) + (j >> 1)) & 0xFFFFFFFFFFFFFFFF
    h = int(mm_hash64(np.array([key], dtype=np.uint64))[0])
    w = (h >> 32) if (j & 1) else (h & 0xFFFFFFFF)
    return (w * m) >> 32


def draws(seed, B, m):
    """the [B, m] indices the rule draws"""
    with np.errstate(over="ignore"):
        key = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + (np.arange(B, dtype=np.uint64)[:, None] << np.uint64(32)) + (np.arange(m, dtype=np.uint64)[None, :] >> np.uint64(1))
    h = mm_hash64(key)
    odd = (np.arange(m)[None, :] & 1).astype(bool)
    w = np.where(odd, h >> np.uint64(32), h & np.uint64(0xFFFFFFFF))
    return ((w * np.uint64(m)) >> np.uint64(32)).astype(np.int64)      # (w < 2^32, m < 2^32: no overflow)


def means(values, iterations=0, seed=0):
    """the B resample means, each the sequential double sum of its draws over m"""
    v = np.asarray(values, np.float64)
    B, m = ranks(iterations)[0], len(v)
    g = v[draws(seed, B, m)]                     # [B, m]
    s = np.zeros(B, np.float64)
    for j in range(m):                           # (column by column: every row is added in draw order, in double)
        s = s + g[:, j]
    return s / np.float64(m)


def interval(values, iterations=0, seed=0):
    """(lo, hi) as float32; (-1, -1) without a value"""
    if len(values) == 0:
        return np.float32(-1.0), np.float32(-1.0)
    _, lo, hi = ranks(iterations)
    s = np.sort(means(values, iterations, seed))
    return np.float32(s[lo]), np.float32(s[hi])


def shifted(lo, hi, ani, ani_raw):
    """the bounds of a pair whose `ani` the regression model produced: moved by ani - ani_raw in float, clamped to [0, 1]"""
    d = np.float32(ani) - np.float32(ani_raw)
    return tuple(np.float32(min(max(np.float32(x) + d, np.float32(0.0)), np.float32(1.0))) for x in (lo, hi))


def values_of(chunks, k=T.K):
    """the values of a pair from oracle.last_chunks() (the rows that kept a chain, chunk order)"""
    return T.chunk_values(chunks, k)
