"""The marker screen's rule, restated plainly (numpy, float64): oracle/skani_oracle.c orc_screen line for line, and the same over whole matrices.

A pair (query, reference) is chained when
    rescue and small < 20                                   -> yes          (small = the smaller of the two marker counts)
    small == 0                                              -> no
    n_shared / small > pow(screen_val, 21)                  -> yes, else no (both counts as doubles; the power is libm's pow)
Marker sets are sorted arrays of distinct uint64 values."""
import math

import numpy as np

K_MARKER = 21
SMALL_MARKER_COUNT = 20
MARKER_BITS = 2 * K_MARKER


def shared(q, r):
    """size of the intersection of two sorted distinct uint64 arrays"""
    return int(np.intersect1d(np.asarray(q, np.uint64), np.asarray(r, np.uint64), assume_unique=True).size)


def passes(n_shared, nq, nr, screen_val, rescue):
    small = nq if nq < nr else nr
    if rescue and small < SMALL_MARKER_COUNT:
        return True
    if small == 0:
        return False
    thresh = math.pow(screen_val, float(K_MARKER))
    return float(n_shared) / float(small) > thresh


def first_passing(small, screen_val):
    """the smallest shared count for which the rule itself (no rescue) says yes for a pair whose smaller set holds `small` markers; it may exceed `small`
    (screen_val = 1.0: no pair passes). small = 0 never passes: None."""
    if small == 0:
        return None
    s = max(0, int(math.pow(screen_val, float(K_MARKER)) * small) - 2)
    while s > 0 and passes(s, small, small, screen_val, False):      # (the estimate is only where the walk starts)
        s -= 1
    while not passes(s, small, small, screen_val, False):
        s += 1
    assert s == 0 or not passes(s - 1, small, small, screen_val, False)
    return s


def inverted_bits(total):
    """width of the bucket table build_inverted (csrc/screen.hip) lays over an inverted index of `total` (marker, reference) entries; the bucket of a marker is
    marker >> (MARKER_BITS - bits)"""
    bits = 4
    while bits < 24 and (16 << bits) < total:
        bits += 1
    return min(bits, MARKER_BITS)


class _Table:
    """every (marker, reference) of the reference sets, sorted by marker"""

    def __init__(self, ref_sets):
        self.n_refs = len(ref_sets)
        self.sizes = np.array([len(r) for r in ref_sets], np.int64)
        keys = np.concatenate([np.asarray(r, np.uint64) for r in ref_sets]) if self.n_refs else np.zeros(0, np.uint64)
        ids = np.repeat(np.arange(self.n_refs, dtype=np.int64), self.sizes)
        order = np.argsort(keys, kind="stable")
        self.keys, self.ids = keys[order], ids[order]

    def counts(self, query_sets):
        """shared-marker counts [len(query_sets)][n_refs]: a sorted join of the queries' markers with the table"""
        out = np.zeros((len(query_sets), self.n_refs), np.uint32)
        sizes = np.array([len(q) for q in query_sets], np.int64)
        if not sizes.sum() or not len(self.keys):
            return out
        qm = np.concatenate([np.asarray(q, np.uint64) for q in query_sets])
        qid = np.repeat(np.arange(len(query_sets), dtype=np.int64), sizes)
        lo, hi = np.searchsorted(self.keys, qm, "left"), np.searchsorted(self.keys, qm, "right")
        run = hi - lo
        first = np.cumsum(run) - run
        entry = np.repeat(lo, run) + (np.arange(int(run.sum()), dtype=np.int64) - np.repeat(first, run))
        np.add.at(out, (np.repeat(qid, run), self.ids[entry]), 1)
        return out


def count_matrix(ref_sets, query_sets):
    return _Table(ref_sets).counts(query_sets)


def apply_rule(counts, q_sizes, r_sizes, screen_val, rescue):
    """the rule on every cell of a count matrix"""
    small = np.minimum(np.asarray(q_sizes, np.int64)[:, None], np.asarray(r_sizes, np.int64)[None, :])
    thresh = math.pow(screen_val, float(K_MARKER))
    with np.errstate(divide="ignore", invalid="ignore"):
        ok = counts.astype(np.float64) / small.astype(np.float64) > thresh
    ok &= small != 0
    if rescue:
        ok |= small < SMALL_MARKER_COUNT
    return ok


def pass_matrix(ref_sets, query_sets, screen_val, rescue, rows=128):
    """bool [len(query_sets)][len(ref_sets)], `rows` queries at a time (the counts of a large case do not all sit in memory at once)"""
    table = _Table(ref_sets)
    out = np.zeros((len(query_sets), len(ref_sets)), np.bool_)
    for b in range(0, len(query_sets), rows):
        part = query_sets[b:b + rows]
        out[b:b + rows] = apply_rule(table.counts(part), [len(q) for q in part], table.sizes, screen_val, rescue)
    return out


def pass_matrix_naive(ref_sets, query_sets, screen_val, rescue):
    """the same by shared() and passes(), pair by pair"""
    return np.array([[passes(shared(q, r), len(q), len(r), screen_val, rescue) for r in ref_sets] for q in query_sets], np.bool_).reshape(len(query_sets), len(ref_sets))
