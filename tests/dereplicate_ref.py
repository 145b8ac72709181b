"""Pure-Python restatement of the cluster stage's semantics (include/pyskani_amd.h, psk_cluster_records): the yardstick of tests/test_gpu_dereplicate.py, itself held
to an independent formulation by tests/test_dereplicate_cpu.py. Nothing here is shared with the library: dictionaries, a sequential walk, union-find.

Records are psk_hit_min: q = query & 0x7FFFFFFF, r = ref_index. A record qualifies iff q != r, ani >= float32(min_ani) and the aligned-fraction rule holds, all in
float32; a NaN fails every comparison (so `min(af_query, af_ref) >= min_af` is written as two comparisons joined by `and`, `max(...)` as two joined by `or`: the same
thing for numbers, and defined for a NaN). The unordered pair {q, r} is an edge iff one of its records qualifies; its weight is the largest qualifying ani."""
import numpy as np


def make_records(rows):
    """rows of (q, r, ani, af_query, af_ref[, learned]) -> psk_hit_min records"""
    from pyskani_amd import _capi
    recs = np.zeros(len(rows), np.dtype(_capi.HitMin))
    for k, row in enumerate(rows):
        q, r, ani, afq, afr = row[:5]
        recs[k]["ani"], recs[k]["af_query"], recs[k]["af_ref"], recs[k]["ref_index"] = ani, afq, afr, r
        recs[k]["query"] = q | (0x80000000 if len(row) > 5 and row[5] else 0)
    return recs


def edge_map(recs, n, min_ani=0.95, min_af=0.5, af="both"):
    """{(a, b) with a < b: float32 weight}; ValueError for an index of n or more"""
    assert af in ("both", "either")
    ma = np.float32(0.95 if min_ani <= 0 else min_ani)
    mf = np.float32(0.5 if min_af < 0 else min_af)
    edges = {}
    for rec in recs:
        q, r = int(rec["query"]) & 0x7FFFFFFF, int(rec["ref_index"])
        if q >= n or r >= n:
            raise ValueError("index out of range")
        ani, afq, afr = np.float32(rec["ani"]), np.float32(rec["af_query"]), np.float32(rec["af_ref"])
        if q == r or not bool(ani >= ma):
            continue
        if min_af != 0:
            a, b = bool(afq >= mf), bool(afr >= mf)
            if not ((a and b) if af == "both" else (a or b)):
                continue
        key = (min(q, r), max(q, r))
        if key not in edges or ani > edges[key]:
            edges[key] = ani
    return edges


def order_of(n, priority=None):
    """the genomes, first in the order first: larger priority, then smaller index"""
    if priority is None:
        return list(range(n))
    return sorted(range(n), key=lambda v: (-int(priority[v]), v))


def adjacency(edges, n):
    adj = [dict() for _ in range(n)]
    for (a, b), w in edges.items():
        adj[a][b] = w
        adj[b][a] = w
    return adj


def greedy_representatives(edges, n, priority=None):
    """the sequential walk: the set of representatives"""
    adj = adjacency(edges, n)
    reps = set()
    for v in order_of(n, priority):
        if not any(u in reps for u in adj[v]):
            reps.add(v)
    return reps


def greedy(edges, n, priority=None):
    """(rep_of uint32[n], rep_ani float32[n]): the walk, then every member to its adjacent representative of largest weight, ties to the earlier in the order"""
    adj = adjacency(edges, n)
    reps = greedy_representatives(edges, n, priority)
    rank = {v: i for i, v in enumerate(order_of(n, priority))}
    rep_of, rep_ani = np.zeros(n, np.uint32), np.zeros(n, np.float32)
    for v in range(n):
        if v in reps:
            rep_of[v], rep_ani[v] = v, 1.0
            continue
        best = None
        for u, w in adj[v].items():
            if u in reps and (best is None or w > best[1] or (w == best[1] and rank[u] < rank[best[0]])):
                best = (u, w)
        rep_of[v], rep_ani[v] = best
    return rep_of, rep_ani


def single(edges, n, priority=None):
    """(rep_of, rep_ani): connected components by union-find; the representative is the component's first genome in the order; rep_ani = the direct edge's weight or 0"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in edges:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
    first = {}
    for v in order_of(n, priority):
        first.setdefault(find(v), v)
    rep_of, rep_ani = np.zeros(n, np.uint32), np.zeros(n, np.float32)
    for v in range(n):
        rep = first[find(v)]
        rep_of[v] = rep
        rep_ani[v] = 1.0 if rep == v else edges.get((min(v, rep), max(v, rep)), np.float32(0.0))
    return rep_of, rep_ani


def reference(recs, n, *, min_ani=0.95, min_af=0.5, af="both", linkage="greedy", priority=None):
    edges = edge_map(recs, n, min_ani, min_af, af)
    return (greedy if linkage == "greedy" else single)(edges, n, priority)
