"""GPU: the linkage forest (psk_cluster_forest, pyskani_amd.forest_records, Database.linkage_forest).

Every synthetic case goes through `forest_records` and is compared with tests/forest_ref.py, the sequential Kruskal under the stated edge order: the three arrays equal,
`ani` BIT FOR BIT (a weight is one of the input's floats, never computed), edge for edge and in order. The shipped single linkage is a second, independent yardstick:
`labels(t)` equals `cluster_records(linkage="single", min_ani=t)` at the forest's own weights. The cases are the ones at which the device code takes another path: ties
that only the order decides, a hooking chain that needs every pointer jump, several rounds with mutual picks, a row longer than two wave strides, more than 65 536
vertices."""
import ctypes as C

import numpy as np
import pytest

import dereplicate_ref as R
import forest_ref as F

pytestmark = pytest.mark.gpu

MAX_CUTS = 16


def stats():
    """(edges, rounds, jump_passes) of the default context's last forest call that reached the device"""
    import pyskani_amd
    from pyskani_amd import _capi
    e, r, j = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert _capi.load().psk_ctx_forest_stats(pyskani_amd.default_context(0)._h, C.byref(e), C.byref(r), C.byref(j)) == 0
    return e.value, r.value, j.value


def check(rows_or_recs, n, **kw):
    """the forest against the reference, its cuts against the shipped single linkage, its merges as a linkage matrix; returns the Forest"""
    import pyskani_amd
    recs = rows_or_recs if isinstance(rows_or_recs, np.ndarray) else R.make_records(rows_or_recs)
    f = pyskani_amd.forest_records(recs, n, **kw)
    ref_kw = {"min_ani": 0.80, "min_af": 0.5, "af": "both", **kw}
    edges = R.edge_map(recs, n, ref_kw["min_ani"], ref_kw["min_af"], ref_kw["af"])
    wa, wb, wani = F.kruskal(edges, n)
    assert f.n == n and f.a.dtype == f.b.dtype == np.uint32 and f.ani.dtype == np.float32 and f.names is None
    assert np.array_equal(f.a, wa) and np.array_equal(f.b, wb), (kw, list(zip(f.a.tolist(), f.b.tolist())), list(zip(wa.tolist(), wb.tolist())))
    assert f.ani.tobytes() == wani.tobytes(), (kw, f.ani.tolist(), wani.tolist())
    assert len(f) == n - F.components(edges, n)
    cuts = np.unique(f.ani)
    if len(cuts) > MAX_CUTS:
        cuts = cuts[np.linspace(0, len(cuts) - 1, MAX_CUTS).round().astype(int)]
    for t in cuts:
        single = pyskani_amd.cluster_records(recs, n, linkage="single", min_ani=float(t), min_af=ref_kw["min_af"], af=ref_kw["af"])[0]
        assert np.array_equal(f.labels(t), single), (kw, float(t))
    F.check_linkage(f.merges()[0], n)
    if len(edges):
        assert stats()[0] == len(edges)
    return f


def pairs(f):
    return list(zip(f.a.tolist(), f.b.tolist()))


def test_no_records():
    for n in (1, 5):
        f = check([], n)
        assert len(f) == 0 and f.labels(0.9).tolist() == list(range(n))


def test_two_genomes():
    one = check([(0, 1, 0.97, 0.9, 0.9)], 2)
    assert pairs(one) == [(0, 1)] and one.ani[0] == np.float32(0.97)
    assert pairs(check([(1, 0, 0.97, 0.9, 0.9)], 2)) == [(0, 1)]                                 # the other direction: the same edge
    both = check([(0, 1, 0.949, 0.9, 0.9), (1, 0, 0.951, 0.9, 0.9)], 2, min_ani=0.95)            # one direction qualifies: an edge of its weight
    assert pairs(both) == [(0, 1)] and both.ani[0] == np.float32(0.951)
    assert len(check([(0, 1, 0.949, 0.9, 0.9), (1, 0, 0.9499, 0.9, 0.9)], 2, min_ani=0.95)) == 0
    assert len(check([(0, 1, np.float32(0.95), 0.9, 0.9)], 2, min_ani=0.95)) == 1                # the floor is inclusive, in float
    below = np.nextafter(np.float32(0.95), np.float32(0))
    assert len(check([(0, 1, below, 0.9, 0.9)], 2, min_ani=0.95)) == 0
    assert len(check([(0, 1, np.float32(0.80), 0.9, 0.9)], 2)) == 1                              # ... the default floor as well
    assert len(check([(0, 1, np.nextafter(np.float32(0.80), np.float32(0)), 0.9, 0.9)], 2)) == 0
    assert len(check([(0, 1, 0.96, 0.9, 0.9)], 2, min_ani=-1.0)) == 1 and len(check([(0, 1, 0.94, 0.9, 0.9)], 2, min_ani=0.0)) == 0      # not positive: 0.95
    assert len(check([(1, 1, 0.99, 0.9, 0.9), (0, 0, 0.99, 0.9, 0.9)], 2)) == 0                  # self records are ignored
    assert len(check([(0, 1, np.nan, 0.9, 0.9)], 2)) == 0                                        # a NaN fails every comparison
    assert len(check([(0, 1, 0.99, np.nan, 0.9)], 2)) == 0
    assert len(check([(0, 1, 0.99, np.nan, 0.9)], 2, af="either")) == 1                          # ... its own: the other fraction's still holds
    assert pairs(check([(1, 0, 0.97, 0.9, 0.9, True)], 2)) == [(0, 1)]                           # bit 31 of `query` is no part of the index


def test_one_weight_everywhere_the_order_alone_decides():
    n = 8
    f = check([(i, j, 0.97, 0.9, 0.9) for i in range(n) for j in range(i + 1, n)], n)            # K8: the star at 0
    assert pairs(f) == [(0, j) for j in range(1, n)]
    n = 64
    f = check([(i, (i + 1) % n, 0.97, 0.9, 0.9) for i in range(n)], n)                           # a ring: every edge but the last in the order
    assert pairs(f) == [(0, 1), (0, 63)] + [(i, i + 1) for i in range(1, 62)]


def test_path_of_256_hooks_as_one_chain():
    """strictly increasing weights: every vertex picks the edge to its right, one chain of 254 hooks that eight pointer jumps flatten"""
    n = 256
    f = check([(i, i + 1, 0.90 + 0.0003 * i, 0.9, 0.9) for i in range(n - 1)], n)
    assert pairs(f) == [(i, i + 1) for i in range(n - 2, -1, -1)]
    edges, rounds, jumps = stats()
    assert edges == n - 1 and rounds >= 1 and jumps >= 8, (edges, rounds, jumps)


def test_path_of_64_takes_several_rounds_with_mutual_picks():
    n = 64
    rows = [(i, i + 1, 0.96 + 0.0005 * ((7 * i) % 40), 0.9, 0.9) if i % 2 else (i + 1, i, 0.96 + 0.0005 * ((7 * i) % 40), 0.9, 0.9) for i in range(n - 1)]
    f = check(rows, n)
    assert len(f) == n - 1
    assert stats()[1] >= 2, stats()


def test_star_of_130():
    """a row of 130 entries: three strides of a wave; the two heaviest leaves tie"""
    n = 131
    w = [0.955 + 0.0001 * ((7 * i) % 200) for i in range(n)]
    w[57] = w[99] = 0.99
    rows = [(0, i, w[i], 0.9, 0.9) if i % 3 else (i, 0, w[i], 0.9, 0.9) for i in range(1, n)]
    f = check(rows, n)
    assert len(f) == 130 and pairs(f)[:2] == [(0, 57), (0, 99)] and f.ani[0] == f.ani[1] == np.float32(0.99)


def test_repeated_records_of_one_pair():
    rows = [(3, 1, 0.96, 0.9, 0.9), (1, 3, 0.98, 0.9, 0.9), (3, 1, 0.97, 0.9, 0.9), (1, 3, 0.94, 0.9, 0.9), (3, 1, 0.985, 0.9, 0.2), (1, 3, 0.98, 0.9, 0.9)] * 3
    f = check(rows, 5)
    assert pairs(f) == [(1, 3)] and f.ani[0] == np.float32(0.98)                                # (0.985 fails the fraction rule)
    assert check(rows, 5, af="either").ani[0] == np.float32(0.985)
    assert check(rows, 5, min_ani=0.981, af="either").ani[0] == np.float32(0.985) and len(check(rows, 5, min_ani=0.981)) == 0


@pytest.mark.parametrize("m", [400, 1500])
@pytest.mark.parametrize("seed", range(6))
def test_random_graph_with_many_ties(seed, m):
    n = 300
    rng = np.random.default_rng(200 + seed)
    recs = np.zeros(m, R.make_records([]).dtype)
    recs["query"] = rng.integers(0, n, m).astype(np.uint32) | (rng.integers(0, 2, m).astype(np.uint32) << 31)
    recs["ref_index"] = rng.integers(0, n, m)
    recs["ani"] = np.float32(0.93) + np.float32(0.005) * rng.integers(0, 9, m).astype(np.float32)
    recs["af_query"] = rng.uniform(0.3, 1.0, m).astype(np.float32)
    recs["af_ref"] = rng.uniform(0.3, 1.0, m).astype(np.float32)
    kw = dict(min_ani=0.90, min_af=0.5, af="both")
    edges = R.edge_map(recs, n, **kw)
    assert m // 4 < len(edges) < m, len(edges)                                                 # edges and non-edges
    f = check(recs, n, **kw)
    assert len(np.unique(f.ani)) <= 9 < len(f)                                                 # ties among the forest's own edges
    if m == 1500:      # a guard on the generator: the graph has cycles with ties on them, so another tie rule keeps another SET of edges (at m = 400 it is nearly a forest itself)
        ra, rb, _ = F.kruskal(edges, n, reverse_ties=True)
        assert set(pairs(f)) != set(zip(ra.tolist(), rb.tolist()))


def test_beyond_65536_vertices():
    """a path of 70 000 whose weights cycle through 50 values, and 100 isolated vertices behind it"""
    import pyskani_amd
    path, n = 70_000, 70_100
    i = np.arange(path - 1)
    w = (np.float32(0.90) + np.float32(0.001) * (i % 50).astype(np.float32)).astype(np.float32)
    recs = np.zeros(path - 1, R.make_records([]).dtype)
    recs["query"], recs["ref_index"], recs["ani"], recs["af_query"], recs["af_ref"] = np.where(i % 2, i, i + 1), np.where(i % 2, i + 1, i), w, 0.9, 0.9
    f = pyskani_amd.forest_records(recs, n)
    assert len(f) == path - 1
    order = np.lexsort((i, -w.astype(np.float64)))                                              # every edge is kept: weight descending, then a ascending
    assert np.array_equal(f.a, i[order]) and np.array_equal(f.b, i[order] + 1) and f.ani.tobytes() == w[order].tobytes()
    assert stats()[0] == path - 1 and stats()[1] >= 2
    v = np.arange(n)
    for t in (np.float32(0.80), w[25]):
        starts = np.ones(n, bool)
        starts[1:path] = ~(w >= t)                                                              # vertex v begins a component iff edge (v - 1, v) is below the cut
        want = np.maximum.accumulate(np.where(starts, v, 0))
        assert np.array_equal(f.labels(t), want), float(t)


def test_index_out_of_range_raises_and_the_context_goes_on():
    import pyskani_amd
    n = 4
    good = [(0, 1, 0.97, 0.9, 0.9), (2, 3, 0.97, 0.9, 0.9)]
    for bad in ([(0, 1, 0.97, 0.9, 0.9), (1, n, 0.97, 0.9, 0.9)], [(n, 1, 0.5, 0.9, 0.9)], [(n, n, 0.97, 0.9, 0.9)]):
        with pytest.raises(ValueError, match="n_genomes"):
            pyskani_amd.forest_records(R.make_records(bad), n)
        with pytest.raises(ValueError):
            F.reference(R.make_records(bad), n)
        assert pairs(check(good, n)) == [(0, 1), (2, 3)]                                        # the same context, a valid call


GENOMES = r"""
import numpy as np
lut = np.frombuffer(b"ACGT", np.uint8)
def families(F, M, L, step, seed=123):
    rng = np.random.default_rng(seed)
    def mutate(a, d):
        b = a.copy(); m = rng.random(len(a)) < d; b[m] = (b[m] + rng.integers(1, 4, int(m.sum()), dtype=np.uint8)) & 3; return b
    anc = [rng.integers(0, 4, L, dtype=np.uint8) for _ in range(F)]
    return [(f"f{f}_m{j}", lut[mutate(anc[f], step * j)].tobytes()) for f in range(F) for j in range(M)]
"""


def test_end_to_end_12_genomes():
    import re
    import pyskani_amd
    ns = {}
    exec(GENOMES, ns)
    g = ns["families"](3, 4, 30_000, 0.004)
    n = len(g)
    db = pyskani_amd.Database(compression=30, marker_compression=200)
    db.sketch_many(g)
    names = [x for x, _ in g]
    recs, _ = db.triangle_records()
    assert len(recs) >= 3 * 6
    f = db.linkage_forest()
    assert f.names == names and f.n == n and f.min_ani == 0.80
    again = check(recs, n)
    wa, wb, wani = F.reference(recs, n)
    for other in (again, pyskani_amd.Forest(n, wa, wb, wani, 0.80)):
        assert np.array_equal(f.a, other.a) and np.array_equal(f.b, other.b) and f.ani.tobytes() == other.ani.tobytes()
    lab = f.labels(0.95)
    assert sorted(np.bincount(lab, minlength=n)[np.unique(lab)].tolist()) == [4, 4, 4] and np.unique(lab).tolist() == [0, 4, 8]
    text = f.newick()
    assert text.endswith(";") and sorted(re.findall(r"[(,](f\d_m\d):", text)) == sorted(names)
    F.check_linkage(f.merges()[0], n)
