"""GPU: the bootstrap confidence interval of the ANI (csrc/interval.hip; psk_query_many_ci, psk_chain_ci, Database.query_ci) against tests/interval_ref.py on the
oracle's chunks, at the edges of the kernel's three tiers. The tiers' capacities are the reduce's - 512 chunk rows for the wave tier, 4096 kept values for the
workgroup tier - so interval_cases.py takes tier_cases' batches with pairs of 1, 64, 65, 512, 513, 4096 and 4097 rows, the twins of 513 and 4097 rows (more rows
than a capacity, fewer kept values), and a small batch of its own with 1, 2 and 30 rows and a pair without a chunk table; test_interval_cpu.py holds those batches
to having real intervals (lo < hi, a bound that moves with the seed).

Tolerance: tier_cases.TOL = 1e-6, the suite's own (test_gpu_parity.py). An order statistic of the resample means moves by no more than the largest change of any
mean, so a last-bit difference between the device's pow and libm's stays near 1e-16; the rounding to float32 is 6e-8."""
import ctypes as C

import numpy as np
import pytest

import gbdt_util as G
import interval_cases as IC
import interval_ref as R
import tier_cases as T

pytestmark = pytest.mark.gpu
SHARED = ("ani", "af_query", "af_ref", "ref_index", "query")
_db = {}


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    import os
    for k in [k for k in os.environ if k.startswith("PSK_") and k != "PSK_LIB_PATH"]:
        monkeypatch.delenv(k)


@pytest.fixture(scope="module")
def cases(oracle):
    return IC.cases(oracle)


def _batch(case, model=None):
    """the case's database and query sketches, made once"""
    key = (case.name, model is not None)
    if key not in _db:
        import pyskani_amd as psk
        db = psk.Database(compression=T.C, marker_compression=T.MARKER_C, model=model)
        db.sketch_many([(n, *g) for n, g in case.refs])
        sk = db._sketch_many([(n, *g) for n, g in case.queries], True)
        _db[key] = (db, sk, (C.c_void_p * len(sk))(*[s._h for s in sk]))
    return _db[key]


def _stats(db, reset=0):
    pairs, draws, tiers = C.c_uint64(), C.c_uint64(), (C.c_uint64 * 3)()
    assert db._lib.psk_ctx_interval_stats(db._ctx._h, C.byref(pairs), C.byref(draws), tiers, reset) == 0
    return pairs.value, draws.value, tuple(tiers)


def _ci(case, **kw):
    db, sk, handles = _batch(case)
    kw.setdefault("learned_ani", False)
    return db.query_handles_ci(handles, len(sk), **kw)


def _same_shared_fields(ci, offs, mn, moffs, what):
    assert np.array_equal(offs, moffs), what
    for f in SHARED:
        assert ci[f].tobytes() == mn[f].tobytes(), (what, f)


def _check_bounds(oracle, case, recs, iterations, seed, what):
    assert len(recs)
    named = {p: n for n, p in case.pairs.items()}
    for h in recs:
        pair = (int(h["query"]) & 0x7FFFFFFF, int(h["ref_index"]))
        lo, hi = IC.reference(oracle, case, pair, iterations, seed)
        who = (what, named.get(pair, pair), float(h["ci_lo"]), float(h["ci_hi"]), float(lo), float(hi))
        assert abs(float(h["ci_lo"]) - float(lo)) < T.TOL and abs(float(h["ci_hi"]) - float(hi)) < T.TOL, who
        assert h["ci_lo"] <= h["ci_hi"], who


@pytest.mark.parametrize("name", IC.CASES)
def test_every_pair_equals_the_reference_and_the_expected_tiers_ran(cases, oracle, name):
    case, ch = cases[name], T.chained(oracle, cases[name])
    db, sk, handles = _batch(case)
    _stats(db, reset=1)
    recs, offs = _ci(case)
    pairs, draws, tiers = _stats(db)
    mn, moffs = db.query_handles(handles, len(sk), learned_ani=False)
    _same_shared_fields(recs, offs, mn, moffs, name)
    hit_pairs = {(int(h["query"]), int(h["ref_index"])) for h in recs}
    assert {p for p in case.pairs.values() if ch.res[p].ani > 0.1} <= hit_pairs and len(hit_pairs) == len(recs)
    _check_bounds(oracle, case, recs, 0, 0, name)
    # the tiers the host launches for the batch, and the work: every pair that has an ANI got bounds, each from 100 x m draws
    assert tuple(t > 0 for t in tiers) == IC.tiers(ch), (name, tiers)
    with_ani = [p for p in ch.pairs if ch.res[p].ani >= 0]
    assert pairs == len(with_ani) and draws == 100 * sum(int(ch.res[p].n_chunks) for p in with_ani), (name, pairs, draws)


@pytest.mark.parametrize("name", ["ci_small", "big"])
def test_chain_ci_is_chain_and_the_bounds_of_query_many_ci(cases, oracle, name):
    case = cases[name]
    db, sk, handles = _batch(case)
    lib, n = db._lib, len(case.refs)
    refs = (C.c_void_p * n)(*[lib.psk_db_sketch(db._h, i) for i in range(n)])
    opts = db._opts(False, False, False, None, False)
    from pyskani_amd import _capi
    plain, out = (_capi.Hit * n)(), (_capi.Hit * n)()
    lo, hi = (C.c_float * n)(), (C.c_float * n)()
    _capi.check(lib.psk_chain(db._ctx._h, refs, n, sk[0]._h, C.byref(opts), plain))
    _capi.check(lib.psk_chain_ci(db._ctx._h, refs, n, sk[0]._h, C.byref(opts), None, out, lo, hi))
    assert bytes(plain) == bytes(out)
    recs, offs = _ci(case)
    mine = recs[offs[0]:offs[1]]
    by_ref = {int(h["ref_index"]): h for h in mine}
    assert by_ref
    for i in range(n):
        if i in by_ref:      # the same kernel, values and order: the same bits
            assert np.float32(lo[i]).tobytes() == by_ref[i]["ci_lo"].tobytes() and np.float32(hi[i]).tobytes() == by_ref[i]["ci_hi"].tobytes(), (name, i)
        elif out[i].ani_raw < 0:
            assert (lo[i], hi[i]) == (-1.0, -1.0), (name, i)
    if name == "ci_small":
        i = [nm for nm, _ in case.refs].index("unrelated")
        assert out[i].n_chunks == 0 and (lo[i], hi[i]) == (-1.0, -1.0)
        one = [nm for nm, _ in case.refs].index("rows_1")
        assert out[one].n_chunks == 1 and np.float32(lo[one]).tobytes() == np.float32(hi[one]).tobytes() == np.float32(out[one].ani_raw).tobytes()


def test_batches_and_rounds_do_not_move_a_bound(cases, monkeypatch):
    """edges_a: one batch with the live list by default; 1024 pairs per batch (none has the live list) and 7 queries per round here"""
    want = _ci(cases["edges_a"])
    monkeypatch.setenv("PSK_BATCH_PAIRS_LOG2", "10")
    monkeypatch.setenv("PSK_ROUND_QUERIES", "7")
    got = _ci(cases["edges_a"])
    assert np.array_equal(got[1], want[1]) and got[0].tobytes() == want[0].tobytes()


# ---- families of relatives: 320 genomes of 60 kb = two blocks of the seed index; in a shuffled insertion order the locality order is not the identity

def _families(shuffle=None):
    rng = np.random.default_rng(123)

    def mutate(a, d):
        b = a.copy()
        m = rng.random(len(a)) < d
        b[m] = (b[m] + rng.integers(1, 4, int(m.sum()), dtype=np.uint8)) & 3
        return b
    anc = [rng.integers(0, 4, 60_000, dtype=np.uint8) for _ in range(4)]
    g = [(f"f{f}_m{j}", T.LUT[mutate(anc[f], 0.0005 * j)].tobytes()) for f in range(4) for j in range(80)]
    perm = np.arange(len(g)) if shuffle is None else np.random.default_rng(shuffle).permutation(len(g))
    return [g[i] for i in perm], perm


def _family_db(shuffle=None):
    key = ("families", shuffle)
    if key not in _db:
        import pyskani_amd as psk
        g, perm = _families(shuffle)
        db = psk.Database(compression=T.C, marker_compression=T.MARKER_C)
        db.sketch_many(g)
        _db[key] = (db, perm)
    return _db[key]


def _family_run(shuffle=None, **kw):
    db, perm = _family_db(shuffle)
    recs, offs = db.query_handles_ci(db.sketch_handles(), len(db), learned_ani=False, **kw)
    return recs, offs, perm


@pytest.fixture(scope="module")
def family_base():
    recs, offs, _ = _family_run()
    assert len(recs) >= 320 * 80 and (recs["ci_lo"] < recs["ci_hi"]).sum() > len(recs) // 2      # (three or four chunks per pair: most intervals are real)
    return recs, offs


def test_two_lanes_do_not_move_a_bound(family_base, monkeypatch):
    # (2 000 seeds per genome: PSK_PROBE=0 keeps the round off the contig join, PSK_GSI_SLICE=1 puts it on the slice join, whose rounds may run on two lanes)
    for k, v in (("PSK_PIPELINE", "1"), ("PSK_PROBE", "0"), ("PSK_GSI_SLICE", "1"), ("PSK_BATCH_ITEMS_LOG2", "18")):      # several batches on both lanes
        monkeypatch.setenv(k, v)
    db, _ = _family_db()
    refit = C.c_uint64()
    assert db._lib.psk_ctx_rerun_stats(db._ctx._h, None, None, None, None, 1) == 0
    _stats(db, reset=1)
    recs, offs, _ = _family_run()
    assert db._lib.psk_ctx_rerun_stats(db._ctx._h, None, None, None, C.byref(refit), 0) == 0 and refit.value == 0      # (the lanes kept their batches)
    assert _stats(db)[2][0] >= 8 and _stats(db)[0] == 320 * 80 == len(recs)      # (many batches; a genome passes the screen against its own family: each such pair got bounds once)
    assert np.array_equal(offs, family_base[1]) and recs.tobytes() == family_base[0].tobytes()


def test_rounds_and_batches_of_one_chain_do_not_move_a_bound(family_base, monkeypatch):
    for k, v in (("PSK_PIPELINE", "0"), ("PSK_ROUND_QUERIES", "37"), ("PSK_BATCH_ITEMS_LOG2", "18")):
        monkeypatch.setenv(k, v)
    recs, offs, _ = _family_run()
    assert np.array_equal(offs, family_base[1]) and recs.tobytes() == family_base[0].tobytes()


def test_the_insertion_order_does_not_move_a_bound(family_base):
    db, perm = _family_db(shuffle=9)
    ident = C.c_uint32(9)
    recs, offs, _ = _family_run(shuffle=9)
    assert db._lib.psk_db_locality(db._h, None, None, C.byref(ident)) == 0 and ident.value == 0      # (hits are mapped back and sorted again)
    got = recs.copy()
    got["query"] = perm[recs["query"] & 0x7FFFFFFF].astype(np.uint32) | (recs["query"] & np.uint32(0x80000000))
    got["ref_index"] = perm[recs["ref_index"]]
    got = got[np.lexsort((got["ref_index"], got["query"] & 0x7FFFFFFF))]
    assert got.tobytes() == family_base[0].tobytes()


def test_the_triangle_is_the_full_runs_upper_half(family_base):
    db, _ = _family_db()
    recs, offs = db.triangle_records_ci(learned_ani=False)
    full = family_base[0]
    want = full[full["ref_index"] > (full["query"] & 0x7FFFFFFF)]
    assert len(want) and recs.tobytes() == want.tobytes()
    mn, moffs = db.triangle_records(learned_ani=False)
    assert np.array_equal(offs, moffs) and all(recs[f].tobytes() == mn[f].tobytes() for f in SHARED)


# ---- options

@pytest.mark.parametrize("iterations,seed", [(20, 0), (1024, 0), (100, 7), (0, 2 ** 64 - 1)])
def test_iterations_and_seed(cases, oracle, iterations, seed):
    for name in ("ci_small", "edges_b"):
        recs, _ = _ci(cases[name], iterations=iterations, rng_seed=seed)
        _check_bounds(oracle, cases[name], recs, iterations, seed, (name, iterations, seed))


def test_refusals_leave_the_context_usable(cases):
    from pyskani_amd import _capi
    case = cases["ci_small"]
    db, sk, handles = _batch(case)
    lib, n = db._lib, len(sk)
    want = _ci(case)

    def call(opts, ci):
        hits_p, offs = C.POINTER(_capi.HitCi)(), (C.c_uint64 * (n + 1))()
        rc = lib.psk_query_many_ci(db._h, handles, n, None, 0, C.byref(opts), C.byref(ci) if ci is not None else None, C.byref(hits_p), offs)
        msg = lib.psk_last_error().decode()
        if hits_p:
            lib.psk_free(hits_p)
        return rc, msg
    mean = db._opts(False, False, False, None, False)
    for ci in (_capi.CiOpts(19, 0, 0), _capi.CiOpts(1025, 0, 0), _capi.CiOpts(0, 1, 0)):
        rc, msg = call(mean, ci)
        assert rc == _capi.PSK_EINVAL, (ci.iterations, ci.reserved)
        with pytest.raises(ValueError):
            _capi.check(rc)
    for flags in ((True, False), (False, True)):
        rc, msg = call(db._opts(False, *flags, None, False), None)
        assert rc == _capi.PSK_EINVAL and "mean" in msg, msg
        refs = (C.c_void_p * 1)(lib.psk_db_sketch(db._h, 0))
        out, lo, hi = (_capi.Hit * 1)(), (C.c_float * 1)(), (C.c_float * 1)()
        assert lib.psk_chain_ci(db._ctx._h, refs, 1, sk[0]._h, C.byref(db._opts(False, *flags, None, False)), None, out, lo, hi) == _capi.PSK_EINVAL
    for bad in (19, 1025, -1):
        with pytest.raises(ValueError):
            _ci(case, iterations=bad)
    with pytest.raises(ValueError):
        _ci(case, rng_seed=-1)
    assert call(mean, None)[0] == 0      # NULL options: the defaults
    got = _ci(case)
    assert np.array_equal(got[1], want[1]) and got[0].tobytes() == want[0].tobytes()


def test_learned_bounds_move_with_the_ani(cases, oracle):
    import pyskani_amd as psk
    case = cases["ci_small"]
    trees = G.random_trees(np.random.default_rng(2), n_trees=2, depth=2)
    db, sk, handles = _batch(case, model=psk.Model.from_trees(trees, bias=98.0))
    raw, roffs = db.query_handles(handles, len(sk), learned_ani=True, raw=True)
    recs, offs = db.query_handles_ci(handles, len(sk), learned_ani=True)
    assert np.array_equal(offs, roffs) and len(recs) >= 3 and (raw["learned"] == 1).all() and (recs["query"] >> 31 == 1).all()
    assert (raw["ani"] != raw["ani_raw"]).any()
    for h, r in zip(recs, raw):
        assert h["ani"].tobytes() == r["ani"].tobytes() and h["ref_index"] == r["ref_index"]
        lo, hi = IC.reference(oracle, case, (0, int(h["ref_index"])))
        lo, hi = R.shifted(lo, hi, r["ani"], r["ani_raw"])
        assert abs(float(h["ci_lo"]) - float(lo)) < T.TOL and abs(float(h["ci_hi"]) - float(hi)) < T.TOL and 0.0 <= h["ci_lo"] <= h["ci_hi"] <= 1.0
    plain, _ = db.query_handles_ci(handles, len(sk), learned_ani=False)      # without the model's ANI: the raw bounds
    _check_bounds(oracle, case, plain, 0, 0, "model loaded, learned_ani=False")
    assert (plain["query"] >> 31 == 0).all()


# ---- the Python surface

def test_query_ci_returns_interval_hits(cases):
    import pyskani_amd as psk
    case = cases["ci_small"]
    db, _, _ = _batch(case)
    contigs = case.queries[0][1]
    hits = db.query("q", *contigs, learned_ani=False)
    got = db.query_ci("q", *contigs, learned_ani=False)
    assert len(got) == len(hits) >= 3 and all(type(h) is psk.IntervalHit and isinstance(h, psk.Hit) for h in got)
    for a, b in zip(got, hits):
        assert (a.identity, a.query_name, a.query_fraction, a.reference_name, a.reference_fraction) == (b.identity, b.query_name, b.query_fraction, b.reference_name, b.reference_fraction)
        assert a.identity_low <= a.identity_high and a.learned is False
        with pytest.raises(AttributeError):
            a.identity_low = 0.5
    wide = [h for h in got if h.reference_name == "rows_30"]
    assert wide and wide[0].identity_low < wide[0].identity < wide[0].identity_high
    assert db.query_ci("q", *contigs, learned_ani=False, rng_seed=7)[0].query_name == "q"


# ---- off means off

def test_a_call_without_intervals_launches_nothing_of_them(cases):
    case = cases["edges_b"]
    db, sk, handles = _batch(case)
    lib, ctx = db._lib, db._ctx._h
    ms, n = C.c_double(), C.c_uint64()
    assert lib.psk_ctx_set_timing(ctx, 1) == 0
    try:
        assert lib.psk_ctx_timing(ctx, b"reset", None, None) == 0
        _stats(db, reset=1)
        db.query_handles(handles, len(sk), learned_ani=False)
        assert lib.psk_ctx_timing(ctx, b"interval", C.byref(ms), C.byref(n)) == 0 and n.value == 0 and ms.value == 0.0
        assert _stats(db) == (0, 0, (0, 0, 0))
        _ci(case)      # ... and the timer does see the launches of a call that asks
        assert lib.psk_ctx_timing(ctx, b"interval", C.byref(ms), C.byref(n)) == 0 and n.value >= 1 and ms.value > 0.0
        assert _stats(db)[0] > 0
    finally:
        assert lib.psk_ctx_set_timing(ctx, 0) == 0
