"""GPU: the cluster stage (psk_cluster_records, pyskani_amd.cluster_records, Database.dereplicate).

Every synthetic case goes through `cluster_records` and is compared with tests/dereplicate_ref.py, the pure-Python restatement of the semantics: rep_of equal, rep_ani
equal BIT FOR BIT (a weight is one of the input's floats, never computed), for both linkages. The cases are the ones at which the device code takes another path: a
decision chain deeper than the four rounds of one synchronisation and than one wave, a row longer than two wave strides, ties, repeated and two-directional records."""
import ctypes as C

import numpy as np
import pytest

import dereplicate_ref as R

pytestmark = pytest.mark.gpu

LINKAGES = ("greedy", "single")


def check(rows_or_recs, n, **kw):
    """both linkages against the helper; returns {linkage: (rep_of, rep_ani)}"""
    import pyskani_amd
    recs = rows_or_recs if isinstance(rows_or_recs, np.ndarray) else R.make_records(rows_or_recs)
    out = {}
    for linkage in LINKAGES:
        rep_of, rep_ani = pyskani_amd.cluster_records(recs, n, linkage=linkage, **kw)
        want_of, want_ani = R.reference(recs, n, linkage=linkage, **kw)
        assert rep_of.dtype == np.uint32 and rep_ani.dtype == np.float32 and len(rep_of) == len(rep_ani) == n
        assert np.array_equal(rep_of, want_of), (linkage, kw, rep_of.tolist(), want_of.tolist())
        assert rep_ani.tobytes() == want_ani.tobytes(), (linkage, kw, rep_ani.tolist(), want_ani.tolist())
        out[linkage] = (rep_of, rep_ani)
    return out


def test_no_records():
    for n in (1, 5):
        for rep_of, rep_ani in check([], n).values():
            assert rep_of.tolist() == list(range(n)) and rep_ani.tolist() == [1.0] * n


def test_two_genomes():
    one = check([(0, 1, 0.97, 0.9, 0.9)], 2)
    assert one["greedy"][0].tolist() == [0, 0] and one["greedy"][1].tolist() == [1.0, float(np.float32(0.97))]
    assert check([(1, 0, 0.97, 0.9, 0.9)], 2)["single"][0].tolist() == [0, 0]                     # the other direction: the same edge
    both = check([(0, 1, 0.949, 0.9, 0.9), (1, 0, 0.951, 0.9, 0.9)], 2)                           # one direction qualifies: an edge of its weight
    assert both["greedy"][0].tolist() == [0, 0] and both["greedy"][1][1] == np.float32(0.951)
    assert check([(0, 1, 0.949, 0.9, 0.9), (1, 0, 0.9499, 0.9, 0.9)], 2)["greedy"][0].tolist() == [0, 1]
    exact = check([(0, 1, np.float32(0.95), 0.9, 0.9)], 2)                                        # >= is inclusive, in float
    assert exact["greedy"][0].tolist() == [0, 0]
    below = np.nextafter(np.float32(0.95), np.float32(0))
    assert check([(0, 1, below, 0.9, 0.9)], 2)["greedy"][0].tolist() == [0, 1]
    assert check([(1, 1, 0.99, 0.9, 0.9), (0, 0, 0.99, 0.9, 0.9)], 2)["single"][0].tolist() == [0, 1]      # self records are ignored
    assert check([(0, 1, np.nan, 0.9, 0.9)], 2)["greedy"][0].tolist() == [0, 1]                   # a NaN fails every comparison
    assert check([(0, 1, 0.99, np.nan, 0.9)], 2)["greedy"][0].tolist() == [0, 1]
    assert check([(0, 1, 0.99, np.nan, 0.9)], 2, af="either")["greedy"][0].tolist() == [0, 0]     # ... its own: the other fraction's still holds
    learned = check([(0, 1, 0.97, 0.9, 0.9, True)], 2)                                            # bit 31 of `query` is no part of the index
    assert learned["greedy"][0].tolist() == [0, 0]
    assert check([(1, 0, 0.97, 0.9, 0.9, True)], 2, priority=[1, 2])["single"][0].tolist() == [1, 1]


def test_aligned_fraction_rules():
    rows = [(0, 1, 0.99, 0.6, 0.4), (2, 3, 0.99, 0.4, 0.6), (4, 5, 0.99, 0.4, 0.45), (6, 7, 0.99, 0.5, 0.5)]
    assert check(rows, 8, af="both")["greedy"][0].tolist() == [0, 1, 2, 3, 4, 5, 6, 6]
    assert check(rows, 8, af="either")["greedy"][0].tolist() == [0, 0, 2, 2, 4, 5, 6, 6]
    assert check(rows, 8, min_af=0)["greedy"][0].tolist() == [0, 0, 2, 2, 4, 4, 6, 6]             # no aligned-fraction condition
    assert check(rows, 8, min_af=0, af="either")["single"][0].tolist() == [0, 0, 2, 2, 4, 4, 6, 6]
    assert check(rows, 8, min_af=0.45, af="both")["greedy"][0].tolist() == [0, 1, 2, 3, 4, 5, 6, 6]
    assert check(rows, 8, min_af=-1.0)["greedy"][0].tolist() == [0, 1, 2, 3, 4, 5, 6, 6]          # negative: the default 0.5
    assert check(rows, 8, min_ani=0.995, min_af=0)["greedy"][0].tolist() == list(range(8))
    assert check(rows, 8, min_ani=-1.0, min_af=0)["greedy"][0].tolist() == [0, 0, 2, 2, 4, 4, 6, 6]      # not positive: the default 0.95


@pytest.mark.parametrize("prio", ["descending", "equal", "ascending"])
def test_path_of_64(prio):
    """vertex i's decision waits for vertex i - 1's (i + 1's when the priorities ascend): a chain of 64 decisions, deeper than one synchronisation's four rounds"""
    n = 64
    rng = np.random.default_rng(1)
    rows = [(i, i + 1, 0.96 + 0.0005 * int(rng.integers(0, 40)), 0.9, 0.9) if i % 2 else (i + 1, i, 0.96 + 0.0005 * int(rng.integers(0, 40)), 0.9, 0.9) for i in range(n - 1)]
    priority = {"descending": np.arange(n, 0, -1), "equal": np.full(n, 7), "ascending": np.arange(n)}[prio].astype(np.uint64)
    got = check(rows, n, priority=priority)
    reps = np.flatnonzero(got["greedy"][0] == np.arange(n)).tolist()
    assert reps == (list(range(1, n, 2)) if prio == "ascending" else list(range(0, n, 2)))
    assert set(got["single"][0].tolist()) == {n - 1 if prio == "ascending" else 0}
    if prio == "equal":
        assert all(np.array_equal(a, b) and c.tobytes() == d.tobytes() for (a, c), (b, d) in zip(check(rows, n).values(), got.values()))      # no priorities: the same order


def test_star_of_130():
    """a row of 130 entries: three strides of a wave"""
    n = 131
    w = [0.955 + 0.0001 * ((7 * i) % 200) for i in range(n)]
    w[57] = w[99] = 0.99                                                       # the two heaviest leaves tie
    rows = [(0, i, w[i], 0.9, 0.9) if i % 3 else (i, 0, w[i], 0.9, 0.9) for i in range(1, n)]
    first = check(rows, n)                                                     # the centre is first: one cluster
    assert first["greedy"][0].tolist() == [0] * n
    prio = np.ones(n, np.uint64); prio[0] = 0
    last = check(rows, n, priority=prio)                                       # the centre is last: 130 representatives, the centre goes to the heaviest, ties to the earlier
    assert last["greedy"][0].tolist() == [57] + list(range(1, n)) and last["greedy"][1][0] == np.float32(0.99)
    assert last["single"][0].tolist() == [1] * n
    prio[99] = 5
    assert check(rows, n, priority=prio)["greedy"][0][0] == 99                 # ... earlier in the ORDER, not by index


def test_member_goes_to_a_heavier_representative_that_comes_after_it():
    rows = [(0, 1, 0.96, 0.9, 0.9), (1, 2, 0.99, 0.9, 0.9)]
    got = check(rows, 3, priority=[3, 2, 1])
    assert got["greedy"][0].tolist() == [0, 2, 2] and got["greedy"][1][1] == np.float32(0.99)
    assert got["single"][0].tolist() == [0, 0, 0] and got["single"][1].tolist() == [1.0, float(np.float32(0.96)), 0.0]      # 2 has no direct edge to 0


def test_repeated_records_of_one_pair():
    rows = [(3, 1, 0.96, 0.9, 0.9), (1, 3, 0.98, 0.9, 0.9), (3, 1, 0.97, 0.9, 0.9), (1, 3, 0.94, 0.9, 0.9), (3, 1, 0.985, 0.9, 0.2), (1, 3, 0.98, 0.9, 0.9)] * 3
    got = check(rows, 5)
    assert got["greedy"][0].tolist() == [0, 1, 2, 1, 4] and got["greedy"][1][3] == np.float32(0.98)      # (0.985 fails the fraction rule)
    assert check(rows, 5, af="either")["greedy"][1][3] == np.float32(0.985)


@pytest.mark.parametrize("seed", range(6))
def test_random_graph(seed):
    n, m = 300, 1500
    rng = np.random.default_rng(100 + seed)
    recs = np.zeros(m, R.make_records([]).dtype)
    recs["query"] = rng.integers(0, n, m).astype(np.uint32) | (rng.integers(0, 2, m).astype(np.uint32) << 31)
    recs["ref_index"] = rng.integers(0, n, m)
    recs["ani"] = rng.uniform(0.93, 0.97, m).astype(np.float32)
    recs["af_query"] = rng.uniform(0.3, 1.0, m).astype(np.float32)
    recs["af_ref"] = rng.uniform(0.3, 1.0, m).astype(np.float32)
    priority = rng.integers(0, 8, n).astype(np.uint64)                         # many ties
    edges = R.edge_map(recs, n)
    assert 0 < len(edges) < m // 2, len(edges)                                 # edges and non-edges
    got = check(recs, n, priority=priority)
    for linkage in LINKAGES:
        assert np.bincount(got[linkage][0], minlength=n).max() >= 3, linkage  # a cluster of three or more
    check(recs, n, priority=priority, af="either", min_ani=0.94)
    check(recs, n, min_af=0)


def test_index_out_of_range_raises_and_the_context_goes_on():
    import pyskani_amd
    n = 4
    good = R.make_records([(0, 1, 0.97, 0.9, 0.9), (2, 3, 0.97, 0.9, 0.9)])
    for bad in ([(0, 1, 0.97, 0.9, 0.9), (1, n, 0.97, 0.9, 0.9)], [(n, 1, 0.5, 0.9, 0.9)], [(n, n, 0.97, 0.9, 0.9)]):
        for linkage in LINKAGES:
            with pytest.raises(ValueError, match="n_genomes"):
                pyskani_amd.cluster_records(R.make_records(bad), n, linkage=linkage)
            with pytest.raises(ValueError):
                R.reference(R.make_records(bad), n, linkage=linkage)
        assert check(good, n)["greedy"][0].tolist() == [0, 0, 2, 2]           # the same context, a valid call


GENOMES = r"""
import numpy as np
lut = np.frombuffer(b"ACGT", np.uint8)
def families(F, M, L, step, seed=123, shuffle=None):
    rng = np.random.default_rng(seed)
    def mutate(a, d):
        b = a.copy(); m = rng.random(len(a)) < d; b[m] = (b[m] + rng.integers(1, 4, int(m.sum()), dtype=np.uint8)) & 3; return b
    anc = [rng.integers(0, 4, L, dtype=np.uint8) for _ in range(F)]
    g = [(f"f{f}_m{j}", lut[mutate(anc[f], step * j)].tobytes()) for f in range(F) for j in range(M)]
    if shuffle is not None:
        g = [g[i] for i in np.random.default_rng(shuffle).permutation(F * M)]
    return g
"""


def test_end_to_end_12_genomes():
    import pyskani_amd
    ns = {}
    exec(GENOMES, ns)
    g = ns["families"](3, 4, 30_000, 0.004)
    n = len(g)
    db = pyskani_amd.Database(compression=30, marker_compression=200)
    db.sketch_many(g)
    names = [x for x, _ in g]
    lengths = np.zeros(n, np.uint64)
    tl = C.c_uint64()
    for i in range(n):
        assert db._lib.psk_sketch_info(db._lib.psk_db_sketch(db._h, i), None, None, None, C.byref(tl), None) == 0
        lengths[i] = tl.value
    assert (lengths > 0).all()
    recs, _ = db.triangle_records()
    assert len(recs) >= 3 * 6

    def run(**kw):
        res = db.dereplicate(**kw)
        prio = kw.pop("priority", "length")
        want_of, want_ani = R.reference(recs, n, priority=lengths if isinstance(prio, str) else prio, **kw)
        assert np.array_equal(res.rep_of, want_of) and res.rep_ani.tobytes() == want_ani.tobytes(), (kw, res.rep_of.tolist(), want_of.tolist())
        reps = np.flatnonzero(res.rep_of == np.arange(n))
        assert res.representatives.tolist() == reps.tolist() and res.names == [names[i] for i in reps] and len(res) == len(reps)
        cl = res.clusters()
        assert sorted(cl) == reps.tolist()
        assert all(m.tolist() == np.flatnonzero(res.rep_of == r).tolist() for r, m in cl.items())
        return res
    res = run()
    assert np.array_equal(res.priority, lengths)
    assert len(res.representatives) == 3 and sorted(len(m) for m in res.clusters().values()) == [4, 4, 4]
    assert [nm.split("_")[0] for nm in res.names] == ["f0", "f1", "f2"]
    run(linkage="single")
    run(priority=None)
    run(priority=np.arange(n, dtype=np.uint64))
    med = float(np.median(recs["ani"]))
    q = np.float32(med)
    assert 0 < int((recs["ani"] >= q).sum()) and int((recs["ani"] < q).sum()) > 0      # the threshold splits the records
    run(min_ani=med)
    run(min_ani=med, linkage="single", af="either")
