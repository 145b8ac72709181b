"""CPU: the cluster stage's host side - the yardstick of the GPU tests held to an independent formulation, the C entry point's argument checks (no device is
touched before them) and the Python wrapper's (no library or context call before them)."""
import ctypes as C

import numpy as np
import pytest

import dereplicate_ref as R


def _fixpoint_representatives(edges, n, priority):
    """The representatives as the fixpoint the device iterates to, Jacobi style: every round reads the states of the round before. A vertex with a better-ranked
    neighbour that is a representative becomes a member; one whose better-ranked neighbours are all members (or that has none) becomes a representative."""
    rank = {v: i for i, v in enumerate(R.order_of(n, priority))}
    better = [[] for _ in range(n)]
    for a, b in edges:
        if rank[a] < rank[b]:
            better[b].append(a)
        else:
            better[a].append(b)
    state = [0] * n      # 0 undecided, 1 representative, 2 member
    rounds = 0
    while 0 in state:
        new = list(state)
        for v in range(n):
            if state[v] == 0:
                if any(state[u] == 1 for u in better[v]):
                    new[v] = 2
                elif all(state[u] == 2 for u in better[v]):
                    new[v] = 1
        assert new != state, "a round decided nothing"
        state = new
        rounds += 1
        assert rounds <= n
    return {v for v in range(n) if state[v] == 1}


def test_sequential_walk_equals_the_fixpoint_on_random_graphs():
    for seed in range(50):
        rng = np.random.default_rng(seed)
        n = int(rng.integers(2, 60))
        m = int(rng.integers(0, 4 * n))
        edges = {}
        for _ in range(m):
            a, b = (int(x) for x in rng.integers(0, n, 2))
            if a != b:
                edges[(min(a, b), max(a, b))] = np.float32(rng.uniform(0.95, 1.0))
        priority = None if seed % 3 == 0 else rng.integers(0, 4 if seed % 3 == 1 else 1 << 40, n).astype(np.uint64)
        reps = R.greedy_representatives(edges, n, priority)
        assert reps == _fixpoint_representatives(edges, n, priority), seed
        # ... and it is a maximal independent set: no edge inside it, every other vertex next to it
        adj = R.adjacency(edges, n)
        assert not any(a in reps and b in reps for a, b in edges), seed
        assert all(v in reps or any(u in reps for u in adj[v]) for v in range(n)), seed
        rep_of, rep_ani = R.greedy(edges, n, priority)
        assert all(int(rep_of[v]) in reps and (int(rep_of[v]) == v or rep_ani[v] == adj[v][int(rep_of[v])]) for v in range(n)), seed


def test_entry_point_checks_its_arguments_without_a_device():
    from pyskani_amd import _capi
    lib = _capi.load()
    n = 3
    recs = R.make_records([(0, 1, 0.99, 0.9, 0.9)])
    rep = np.zeros(n, np.uint32)
    ctx = C.create_string_buffer(4096)      # stands for a context: every case below is refused before the context is looked at
    good = _capi.ClusterOpts(0.95, 0.5, 0, 0)

    def call(ctx_p, recs_p, n_recs, opts_p, rep_p):
        st = lib.psk_cluster_records(ctx_p, recs_p, n_recs, n, None, opts_p, rep_p, None, None)
        return st, lib.psk_last_error().decode()
    rp, ip = recs.ctypes.data, rep.ctypes.data
    cp = C.cast(ctx, C.c_void_p)
    assert call(None, rp, 1, C.byref(good), ip)[0] == _capi.PSK_EINVAL
    assert call(cp, rp, 1, None, ip)[0] == _capi.PSK_EINVAL
    assert call(cp, rp, 1, C.byref(good), None)[0] == _capi.PSK_EINVAL
    st, msg = call(cp, None, 1, C.byref(good), ip)
    assert st == _capi.PSK_EINVAL and "recs" in msg
    for af_rule, linkage, word in ((2, 0, "af_rule"), (-1, 0, "af_rule"), (0, 2, "linkage"), (0, -1, "linkage")):
        st, msg = call(cp, rp, 1, C.byref(_capi.ClusterOpts(0.95, 0.5, af_rule, linkage)), ip)
        assert st == _capi.PSK_EINVAL and word in msg, (af_rule, linkage, st, msg)
    assert call(cp, rp, 1 << 30, C.byref(good), ip)[0] == _capi.PSK_ELIMIT
    # no record: every genome its own representative, no device needed
    ani = np.zeros(n, np.float32)
    cnt = C.c_uint32(99)
    assert lib.psk_cluster_records(cp, None, 0, n, None, C.byref(good), ip, ani.ctypes.data, C.byref(cnt)) == _capi.PSK_OK
    assert rep.tolist() == [0, 1, 2] and ani.tolist() == [1.0, 1.0, 1.0] and cnt.value == 3
    assert lib.psk_cluster_records(cp, None, 0, 0, None, C.byref(good), ip, None, None) == _capi.PSK_OK


def test_cluster_records_checks_its_arguments_before_any_library_or_context_call(monkeypatch):
    import pyskani_amd
    from pyskani_amd import _capi, database

    def refuse(*a, **k):
        raise AssertionError("the library or a context was asked for")
    monkeypatch.setattr(_capi, "load", refuse)
    monkeypatch.setattr(database, "default_context", refuse)
    recs = np.zeros(2, np.dtype(_capi.HitMin))
    with pytest.raises(ValueError):
        pyskani_amd.cluster_records(recs, 4, af="any")
    with pytest.raises(ValueError):
        pyskani_amd.cluster_records(recs, 4, linkage="complete")
    with pytest.raises(ValueError):
        pyskani_amd.cluster_records(np.zeros(2, np.dtype(_capi.Hit)), 4)            # the 80-byte records
    with pytest.raises(ValueError):
        pyskani_amd.cluster_records(np.zeros((2, 5), np.float32), 4)
    with pytest.raises(ValueError):
        pyskani_amd.cluster_records([(0, 1)], 4)
    for prio in ([1, 2, 3], [1, 2, 3, 4, 5], [[1, 2, 3, 4]], [1.0, 2.0, 3.0, 4.0], [1, 2, -3, 4]):
        with pytest.raises(ValueError):
            pyskani_amd.cluster_records(recs, 4, priority=prio)
    with pytest.raises(AssertionError):                                             # valid arguments do reach the library
        pyskani_amd.cluster_records(recs, 4, priority=[4, 3, 2, 1])
