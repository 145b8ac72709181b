"""Pure-Python restatement of the linkage forest's semantics (include/pyskani_amd.h, psk_cluster_forest): the yardstick of tests/test_gpu_forest.py, itself held to an
independent formulation by tests/test_forest_cpu.py. Nothing here is shared with the library: the edges are dereplicate_ref.edge_map's dictionary, the forest is a
sequential Kruskal with union-find.

Write an edge as (a, b, w) with a < b. Edge e precedes f iff w_e > w_f, or the weights are equal and (a_e, b_e) < (a_f, b_f). The forest is what Kruskal keeps walking the
edges in that order, and it comes out in that order."""
import numpy as np

import dereplicate_ref as R


class _Sets:
    def __init__(self, n):
        self.parent = list(range(n))

    def find(self, x):
        p = self.parent
        while p[x] != x:
            p[x] = p[p[x]]
            x = p[x]
        return x

    def union(self, x, y):
        """True iff x and y were apart; the root is the smaller index"""
        x, y = self.find(x), self.find(y)
        if x == y:
            return False
        self.parent[max(x, y)] = min(x, y)
        return True


def edge_order(edges, reverse_ties=False):
    """the edges {(a, b): w} as a list of (a, b, w), first in the order first (reverse_ties: equal weights by DESCENDING (a, b) - another rule, for tests that must
    show the tie rule matters)"""
    sign = -1 if reverse_ties else 1
    return sorted(((a, b, w) for (a, b), w in edges.items()), key=lambda e: (-float(e[2]), sign * e[0], sign * e[1]))


def kruskal(edges, n, reverse_ties=False):
    """(a uint32[], b uint32[], ani float32[]): the forest's edges in the order"""
    sets = _Sets(n)
    kept = [e for e in edge_order(edges, reverse_ties) if sets.union(e[0], e[1])]
    return (np.array([e[0] for e in kept], np.uint32), np.array([e[1] for e in kept], np.uint32), np.array([e[2] for e in kept], np.float32))


def reference(recs, n, *, min_ani=0.80, min_af=0.5, af="both"):
    return kruskal(R.edge_map(recs, n, min_ani, min_af, af), n)


def labels(edges, n, t):
    """uint32[n]: the smallest index of every vertex's component among the edges (dictionary, or an (a, b, ani) triple of arrays) with weight >= float32(t)"""
    if not isinstance(edges, dict):
        edges = {(int(a), int(b)): np.float32(w) for a, b, w in zip(*edges)}
    t = np.float32(t)
    sets = _Sets(n)
    for (a, b), w in edges.items():
        if bool(np.float32(w) >= t):
            sets.union(a, b)
    return np.array([sets.find(v) for v in range(n)], np.uint32)


def components(edges, n):
    return len(set(labels(edges, n, -np.inf).tolist()))


def check_linkage(Z, n):
    """Z is a linkage matrix over n leaves in SciPy's layout: ids in range and used once, left id < right id, counts add up, distances do not decrease"""
    Z = np.asarray(Z)
    assert Z.dtype == np.float64 and Z.shape == (max(n - 1, 0), 4), (Z.dtype, Z.shape)
    count = {v: 1 for v in range(n)}
    used = set()
    last = -np.inf
    for i, (x, y, d, c) in enumerate(Z.tolist()):
        assert x == int(x) and y == int(y) and c == int(c), (i, x, y, c)
        x, y = int(x), int(y)
        assert 0 <= x < y < n + i, (i, x, y)
        assert x not in used and y not in used, (i, x, y)
        used.update((x, y))
        assert c == count[x] + count[y], (i, c, count[x], count[y])
        count[n + i] = int(c)
        assert d >= last, (i, d, last)
        last = d
    if n > 1:
        assert used == set(range(2 * n - 2)) and count[2 * n - 2] == n
