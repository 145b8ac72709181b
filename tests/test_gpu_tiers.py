"""GPU: the size tiers of the chain selection (csrc/select.hip) and of the per-pair reduce (csrc/reduce.hip) at their edges - 4 / 5, 64 / 65, 512 / 513,
1024 / 1025 and 4096 / 4097 chunk rows, 8 / 9, 512 / 513 and 1024 / 1025 candidate chains, 128 / 129 conflicted candidates, a running maximum carried across
a 64-lane group, rows without a kept chain on both sides of the compaction's boundaries - under every host state that decides who launches what
(tier_cases.py; test_tier_cases_cpu.py holds every case to what it promises). Every case is one call of psk_query_many (query_handles: the general
path, not the fused small-query one) = one batch of the chain stage.
  - against the oracle, for {}, median, robust: the same hit lists (a pair below min_af is absent on both sides), every integer field equal, ani, af_query,
    af_ref and ani_std within 1e-6 (the suite's tolerance, test_gpu_parity.py) - for EVERY pair of the batch, the named ones among them;
  - psk_ctx_tier_stats: the kernels launched are the ones the restated host predicates name, and the pairs in the live list, left by the lane
    selection, passed to the second and to the workgroup selection tier are the oracle's counts; with the timers on, psk_ctx_join_work's candidate total is
    the oracle's sum;
  - tier against tier: the same batch with PSK_REDUCE_TINY=0, PSK_REDUCE_SMALL=0, PSK_REDUCE_WAVE=0, PSK_SELECT_TINY=0 and PSK_CHAIN_SERIAL=1 (each checked, by
    the counters, to have moved the work) gives bit-equal records but for ani_std, which may be one float32 step away: the tiers add the squared deviations
    in different association orders in double - far below a float32 ulp, not zero. The reduce switches run under all three flag sets, the selection's two
    under the default one (the selection does not see the flags)."""
import ctypes as C

import numpy as np
import pytest

import tier_cases as T

pytestmark = pytest.mark.gpu
CASES = ("edges_a", "edges_b", "edges_c", "edges_d", "big", "conflicts")
INT_FIELDS = ("n_anchors", "n_chunks", "n_intervals", "covered_query", "covered_ref", "sum_chain_anchors", "sum_chunk_seeds")
FLAG_IDS = ["mean", "median", "robust"]
_db = {}


def _batch(case):
    """the case's database and query sketches, made once"""
    if case.name not in _db:
        import pyskani_amd as psk
        db = psk.Database(compression=T.C, marker_compression=T.MARKER_C)
        db.sketch_many([(n, *g) for n, g in case.refs])
        sk = db._sketch_many([(n, *g) for n, g in case.queries], True)
        _db[case.name] = (db, sk, (C.c_void_p * len(sk))(*[s._h for s in sk]))
    return _db[case.name]


def _run(case, flags, timing=False):
    """(records, offsets, tier stats, candidates read by the selection - timers on) of one call under the environment as it stands"""
    db, sk, handles = _batch(case)
    lib, ctx = db._lib, db._ctx._h
    stats, cands = (C.c_uint64 * len(T.STATS))(), C.c_uint64()
    assert lib.psk_ctx_tier_stats(ctx, stats, 0, 1) == 0 and lib.psk_ctx_join_work(ctx, None, None, None, None, 1) == 0
    if timing:
        assert lib.psk_ctx_set_timing(ctx, 1) == 0
    try:
        recs, offs = db.query_handles(handles, len(sk), learned_ani=False, raw=True, **flags)
    finally:
        if timing:
            assert lib.psk_ctx_set_timing(ctx, 0) == 0
    assert lib.psk_ctx_tier_stats(ctx, stats, len(T.STATS), 0) == 0 and lib.psk_ctx_join_work(ctx, None, None, C.byref(cands), None, 0) == 0
    return recs, offs, dict(zip(T.STATS, list(stats))), cands.value


def _check_stats(got, want, what):
    """launch counters: launched or not (a batch sent round again launches again); pair counters: exact"""
    for k in T.STATS[:7]:
        assert (got[k] > 0) == bool(want[k]), (what, k, got, want)
    for k in T.STATS[7:]:
        assert got[k] == want[k], (what, k, got, want)


_default = {}


def _default_run(case, flags):
    key = (case.name, tuple(flags))
    if key not in _default:
        _default[key] = _run(case, flags)
    return _default[key]


@pytest.fixture(scope="module")
def cases(oracle):
    return T.cases(oracle)


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    import os
    for k in [k for k in os.environ if k.startswith("PSK_") and k != "PSK_LIB_PATH"]:      # (every switch off; which build is loaded is no switch)
        monkeypatch.delenv(k)


@pytest.mark.parametrize("flags", T.FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("name", CASES)
def test_every_pair_equals_the_oracle_and_the_expected_tiers_ran(cases, oracle, name, flags):
    case, ch = cases[name], T.chained(oracle, cases[name], flags)
    recs, offs, stats, _ = _default_run(case, flags)
    named = {p: n for n, p in case.pairs.items()}
    n_hits = 0
    for qi in range(len(case.queries)):
        mine = recs[offs[qi]:offs[qi + 1]]
        assert mine["ref_index"].tolist() == ch.hits(qi), (name, case.queries[qi][0])      # (the named pairs below min_af: absent on both sides)
        for h in mine:
            pair = (qi, int(h["ref_index"]))
            want, who = ch.res[pair], (name, named.get(pair, pair))
            for f in INT_FIELDS:
                assert int(h[f]) == int(getattr(want, f)), (who, f, int(h[f]), int(getattr(want, f)))
            for f in ("ani", "af_query", "af_ref", "ani_std"):
                assert abs(float(h[f]) - float(getattr(want, f))) < T.TOL, (who, f, float(h[f]), float(getattr(want, f)))
            n_hits += 1
    assert n_hits >= sum(1 for p in case.pairs.values() if ch.res[p].ani > 0.1) > 0
    _check_stats(stats, T.expected_stats(T.regime(ch.pair_rows, mean=not flags), ch.rows, ch.cands), (name, flags))


@pytest.mark.parametrize("name", CASES)
def test_candidates_read_by_the_selection_are_the_oracles(cases, oracle, name):
    case, ch = cases[name], T.chained(oracle, cases[name])
    recs, offs, stats, cands = _run(case, {}, timing=True)
    assert cands == sum(ch.cands), (name, cands, sum(ch.cands))
    want = _default_run(case, {})
    assert recs.tobytes() == want[0].tobytes() and np.array_equal(offs, want[1])


def _same_but_for_a_step_of_std(got, want, what):
    assert np.array_equal(got[1], want[1]), what
    a, b = got[0], want[0]
    for f in a.dtype.names:
        if f != "ani_std":
            assert a[f].tobytes() == b[f].tobytes(), (what, f, np.nonzero(a[f] != b[f])[0][:5])
    x, y = a["ani_std"], b["ani_std"]
    ok = (x == y) | (x == np.nextafter(y, np.float32(np.inf))) | (x == np.nextafter(y, np.float32(-np.inf)))
    assert ok.all(), (what, x[~ok][:5], y[~ok][:5])


# (the reduce switches under every flag set; the selection's two under the default one)
TIER_RUNS = [(var, flags) for var in T.SWITCHES for flags in T.FLAGS if var.startswith("PSK_REDUCE") or not flags]


@pytest.mark.parametrize("var,flags", TIER_RUNS, ids=[f"{v}-{FLAG_IDS[T.FLAGS.index(f)]}" for v, f in TIER_RUNS])
@pytest.mark.parametrize("name", CASES)
def test_tier_against_tier(cases, oracle, monkeypatch, name, var, flags):
    """(big, PSK_CHAIN_SERIAL=1: one lane selects among 4 097 candidates, O(C^2) reads of global memory - 11 s, the one slow case of this file)"""
    case, ch = cases[name], T.chained(oracle, cases[name], flags)
    want = _default_run(case, flags)
    val, off = T.SWITCHES[var]
    monkeypatch.setenv(var, val)
    got = _run(case, flags)
    monkeypatch.delenv(var)
    _check_stats(got[2], T.expected_stats(T.regime(ch.pair_rows, mean=not flags, off=(off,)), ch.rows, ch.cands), (name, flags, var))
    _same_but_for_a_step_of_std(got, want, (name, flags, var))
