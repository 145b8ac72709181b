"""CPU: the linkage forest's host side - the yardstick of the GPU tests (forest_ref.py) held to an independent formulation, the C entry points' argument checks (no
device is touched before them), the Python wrapper's (no library or context call before them), and `Forest` on hand-built forests."""
import ctypes as C
import re

import numpy as np
import pytest

import dereplicate_ref as R
import forest_ref as F


def _components_by_search(edges, n, t=None):
    """label[v] = the smallest index reachable from v over the edges of weight >= t (all of them for None): a graph search, no union-find"""
    nb = [[] for _ in range(n)]
    for (a, b), w in edges.items():
        if t is None or bool(w >= t):
            nb[a].append(b)
            nb[b].append(a)
    label = [-1] * n
    for s in range(n):
        if label[s] < 0:
            label[s] = s
            todo = [s]
            while todo:
                for u in nb[todo.pop()]:
                    if label[u] < 0:
                        label[u] = s
                        todo.append(u)
    return label


def _prim_weights(edges, n):
    """the weights of a maximum spanning forest grown vertex by vertex (Prim), ascending: every maximum spanning forest has this multiset"""
    adj = R.adjacency(edges, n)
    seen, out = set(), []
    for s in range(n):
        if s in seen:
            continue
        seen.add(s)
        while True:
            best = None
            for v in seen:
                for u, w in adj[v].items():
                    if u not in seen and (best is None or w > best[1]):
                        best = (u, w)
            if best is None:
                break
            seen.add(best[0])
            out.append(float(best[1]))
    return sorted(out)


def test_kruskal_is_a_maximum_spanning_forest_whose_cuts_are_the_thresholded_components():
    differs = 0
    for seed in range(60):
        rng = np.random.default_rng(seed)
        n = 12
        edges = {}
        for _ in range(int(rng.integers(0, 40))):
            a, b = (int(x) for x in rng.integers(0, n, 2))
            if a != b:
                edges[(min(a, b), max(a, b))] = np.float32(0.90) + np.float32(0.01) * np.float32(rng.integers(0, 6))      # many ties
        a, b, w = F.kruskal(edges, n)
        got = list(zip(a.tolist(), b.tolist()))
        assert all(x < y and edges[(x, y)] == wt for (x, y), wt in zip(got, w)), seed
        # in the order: weight descending, ties by (a, b) ascending
        assert got == [(x, y) for x, y, _ in sorted(zip(a.tolist(), b.tolist(), w.tolist()), key=lambda e: (-e[2], e[0], e[1]))], seed
        # acyclic: every edge joins two trees
        sets = F._Sets(n)
        assert all(sets.union(x, y) for x, y in got), seed
        comp = _components_by_search(edges, n)
        assert len(got) == n - len(set(comp)), seed
        assert sorted(w.astype(np.float64).tolist()) == _prim_weights(edges, n), seed
        for t in sorted(set(edges.values())) + [np.float32(2.0)]:
            want = _components_by_search(edges, n, t)
            assert F.labels((a, b, w), n, t).tolist() == want, (seed, t)
            assert F.labels(edges, n, t).tolist() == want, (seed, t)
        ra, rb, _ = F.kruskal(edges, n, reverse_ties=True)
        differs += got != list(zip(ra.tolist(), rb.tolist()))
    assert differs > 30      # the tie rule decides the forest on most of these graphs


def test_entry_points_check_their_arguments_without_a_device():
    from pyskani_amd import _capi
    lib = _capi.load()
    n = 3
    recs = R.make_records([(0, 1, 0.99, 0.9, 0.9)])
    a, b, w = np.zeros(n - 1, np.uint32), np.zeros(n - 1, np.uint32), np.zeros(n - 1, np.float32)
    ctx = C.create_string_buffer(4096)      # stands for a context: every case below is refused before the context is looked at
    good = _capi.ClusterOpts(0.80, 0.5, 0, 1)
    cnt = C.c_uint32(99)

    def call(ctx_p, recs_p, n_recs, opts_p, n_genomes=n, a_p=a.ctypes.data):
        st = lib.psk_cluster_forest(ctx_p, recs_p, n_recs, n_genomes, opts_p, a_p, b.ctypes.data, w.ctypes.data, C.byref(cnt))
        return st, lib.psk_last_error().decode()
    rp, cp = recs.ctypes.data, C.cast(ctx, C.c_void_p)
    assert call(None, rp, 1, C.byref(good))[0] == _capi.PSK_EINVAL
    assert call(cp, rp, 1, None)[0] == _capi.PSK_EINVAL
    assert call(cp, rp, 1, C.byref(good), a_p=None)[0] == _capi.PSK_EINVAL
    st, msg = call(cp, None, 1, C.byref(good))
    assert st == _capi.PSK_EINVAL and "recs" in msg
    for af_rule, linkage, word in ((2, 0, "af_rule"), (-1, 1, "af_rule"), (0, 2, "linkage"), (0, -1, "linkage")):
        st, msg = call(cp, rp, 1, C.byref(_capi.ClusterOpts(0.80, 0.5, af_rule, linkage)))
        assert st == _capi.PSK_EINVAL and word in msg, (af_rule, linkage, st, msg)
    assert call(cp, rp, 1 << 30, C.byref(good))[0] == _capi.PSK_ELIMIT
    assert call(cp, rp, 1, C.byref(good), n_genomes=1 << 31)[0] == _capi.PSK_ELIMIT
    st, msg = call(cp, rp, 1, C.byref(good), n_genomes=0)
    assert st == _capi.PSK_EINVAL and "n_genomes" in msg
    # no record: no edge, no device needed; both linkage values pass
    for linkage in (0, 1):
        cnt.value = 99
        assert call(cp, None, 0, C.byref(_capi.ClusterOpts(0.80, 0.5, 0, linkage)))[0] == _capi.PSK_OK and cnt.value == 0
    for n_genomes in (0, 1):      # NULL arrays are allowed
        cnt.value = 99
        assert lib.psk_cluster_forest(cp, None, 0, n_genomes, C.byref(good), None, None, None, C.byref(cnt)) == _capi.PSK_OK and cnt.value == 0
    assert lib.psk_ctx_forest_stats(None, None, None, None) == _capi.PSK_EINVAL


def test_forest_records_checks_its_arguments_before_any_library_or_context_call(monkeypatch):
    import pyskani_amd
    from pyskani_amd import _capi, database

    def refuse(*a, **k):
        raise AssertionError("the library or a context was asked for")
    monkeypatch.setattr(_capi, "load", refuse)
    monkeypatch.setattr(database, "default_context", refuse)
    recs = np.zeros(2, np.dtype(_capi.HitMin))
    with pytest.raises(ValueError):
        pyskani_amd.forest_records(recs, 4, af="any")
    with pytest.raises(ValueError):
        pyskani_amd.forest_records(np.zeros(2, np.dtype(_capi.Hit)), 4)            # the 80-byte records
    with pytest.raises(ValueError):
        pyskani_amd.forest_records(np.zeros((2, 5), np.float32), 4)
    with pytest.raises(ValueError):
        pyskani_amd.forest_records([(0, 1)], 4)
    with pytest.raises(ValueError):
        pyskani_amd.forest_records(recs, -1)
    with pytest.raises(AssertionError):                                            # valid arguments do reach the library
        pyskani_amd.forest_records(recs, 4)


def _hand_built():
    from pyskani_amd import Forest
    return Forest(6, [0, 2, 1], [1, 3, 2], [0.99, 0.98, 0.96], 0.95)


def test_forest_holds_read_only_arrays():
    from pyskani_amd import Forest
    f = _hand_built()
    assert (f.n, len(f), f.min_ani, f.names) == (6, 3, 0.95, None)
    assert f.a.dtype == f.b.dtype == np.uint32 and f.ani.dtype == np.float32
    assert f.a.tolist() == [0, 2, 1] and f.b.tolist() == [1, 3, 2] and f.ani.tobytes() == np.array([0.99, 0.98, 0.96], np.float32).tobytes()
    for x in (f.a, f.b, f.ani):
        with pytest.raises(ValueError):
            x[0] = 0
    assert len(Forest(0, [], [], [], 0.8)) == 0 and len(Forest(1, [], [], [], 0.8)) == 0
    for bad in ((3, [0, 1, 0], [1, 2, 2], [0.9, 0.9, 0.9]), (3, [1], [1], [0.9]), (3, [0], [3], [0.9]), (3, [0, 1], [1], [0.9])):
        with pytest.raises(ValueError):
            Forest(*bad, 0.8)
    with pytest.raises(ValueError):
        Forest(3, [0], [1], [0.9], 0.8, names=["a", "b"])


def test_labels_at_cuts_and_below_the_floor():
    f = _hand_built()
    assert f.labels(0.95).dtype == np.uint32
    assert f.labels(0.95).tolist() == [0, 0, 0, 0, 4, 5]
    assert f.labels(np.float32(0.96)).tolist() == [0, 0, 0, 0, 4, 5]      # >= is inclusive, in float32
    assert f.labels(0.96).tolist() == [0, 0, 0, 0, 4, 5]                  # (the double 0.96 is above float32(0.96); the cut is taken in float32)
    assert f.labels(np.nextafter(np.float32(0.96), np.float32(1))).tolist() == [0, 0, 2, 2, 4, 5]
    assert f.labels(0.985).tolist() == [0, 0, 2, 3, 4, 5]
    assert f.labels(1.0).tolist() == list(range(6))
    for t in (0.9499, 0.0, -1.0, np.nan):
        with pytest.raises(ValueError, match="floor"):
            f.labels(t)
    edges = (f.a, f.b, f.ani)
    for t in (0.95, 0.97, 0.985, 0.99, 0.995):
        assert f.labels(t).tolist() == F.labels(edges, 6, t).tolist(), t


def test_merges_are_a_linkage_matrix():
    from pyskani_amd import Forest
    f = _hand_built()
    Z, order = f.merges()
    F.check_linkage(Z, 6)
    d = [1.0 - float(np.float32(x)) for x in (0.99, 0.98, 0.96)]
    assert Z.tolist() == [[0, 1, d[0], 2], [2, 3, d[1], 2], [6, 7, d[2], 4], [4, 8, 1.0, 5], [5, 9, 1.0, 6]]
    assert order.dtype == np.int64 and order.tolist() == [5, 4, 0, 1, 2, 3]
    for n in (0, 1):
        Z, order = Forest(n, [], [], [], 0.8).merges()
        assert Z.shape == (0, 4) and Z.dtype == np.float64 and order.tolist() == list(range(n))
    Z, order = Forest(4, [], [], [], 0.8).merges()                       # no edge: a caterpillar at distance 1
    F.check_linkage(Z, 4)
    assert Z.tolist() == [[0, 1, 1.0, 2], [2, 4, 1.0, 3], [3, 5, 1.0, 4]]
    rng = np.random.default_rng(5)
    for _ in range(20):
        n = int(rng.integers(2, 40))
        edges = {}
        for _ in range(int(rng.integers(0, 2 * n))):
            a, b = (int(x) for x in rng.integers(0, n, 2))
            if a != b:
                edges[(min(a, b), max(a, b))] = np.float32(rng.integers(80, 100)) / np.float32(100)
        g = Forest(n, *F.kruskal(edges, n), 0.8)
        Z, order = g.merges()
        F.check_linkage(Z, n)
        assert sorted(order.tolist()) == list(range(n))
        assert Z[:len(g), 2].tolist() == (1.0 - g.ani.astype(np.float64)).tolist() and (Z[len(g):, 2] == 1.0).all()
    with pytest.raises(ValueError, match="cycle"):
        Forest(4, [0, 1, 0], [1, 2, 2], [0.9, 0.9, 0.9], 0.8).merges()


def test_newick_names_every_leaf_once():
    from pyskani_amd import Forest
    assert Forest(2, [0], [1], [0.75], 0.5).newick() == "(0:0.25,1:0.25);"
    assert Forest(2, [0], [1], [0.75], 0.5, names=["a b", "it's"]).newick() == "('a b':0.25,'it''s':0.25);"
    assert Forest(1, [], [], [], 0.5, names=["only"]).newick() == "only;" and Forest(0, [], [], [], 0.5).newick() == ";"
    assert Forest(3, [1], [2], [0.5], 0.5).newick() == "(0:1,(1:0.5,2:0.5):0.5);"
    f = _hand_built()
    text = f.newick()
    assert text.endswith(";") and text.count("(") == text.count(")") == 5
    assert sorted(int(x) for x in re.findall(r"[(,](\d+):", text)) == list(range(6))
    f.names = [f"g{i}" for i in range(6)]
    assert sorted(re.findall(r"[(,](g\d):", f.newick())) == f.names
