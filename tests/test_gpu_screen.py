"""GPU: every path of the marker screen (csrc/screen.hip) against tests/screen_ref.py, bit for bit, on the hand-made marker sets of tests/screen_cases.py - the
whole pass matrix through psk_screen_many, the path and the sub-launches that produced it through psk_ctx_screen_stats - then on sketches of real sequences against
the oracle, and against the hits of query_many. Nothing here has a tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

import screen_cases as S
import screen_ref as R
from conftest import mutate, random_genome

pytestmark = pytest.mark.gpu

# the ways to call the many-query screen: the switches of a call (expected_path: the path it must then take)
MODES = {
    "default": {},
    "brute": {"PSK_SCREEN": "brute"},
    "inv": {"PSK_SCREEN": "inv"},
    "inv_lane": {"PSK_SCREEN": "inv", "PSK_SCREEN_WAVE": "0"},
    "inv_global": {"PSK_SCREEN": "inv", "PSK_SCREEN_GLOBAL": "1"},
    "lane": {"PSK_SCREEN_WAVE": "0"},              # the two switches alone: the size of the call picks the inverted index (the wide case)
    "global": {"PSK_SCREEN_GLOBAL": "1"},
}
SMALL_MODES = ("default", "brute", "inv", "inv_lane", "inv_global")
SWITCHES = ("PSK_SCREEN", "PSK_SCREEN_WAVE", "PSK_SCREEN_GLOBAL")


@pytest.fixture(scope="module")
def psk():
    import pyskani_amd
    return pyskani_amd


def sketches_of(psk, ctx, sets, prefix):
    from pyskani_amd import storage
    empty = np.zeros(0, storage.SEED_DTYPE)
    lens = np.array([1000], "<u4")
    return [psk.Sketch.from_record(ctx, storage.Record(S.PARAMS, f"{prefix}{i}", lens, empty, m), markers_only=True) for i, m in enumerate(sets)]


def add_refs(db, sketches):
    from pyskani_amd import _capi
    for sk in sketches:
        sk._owned = False
        _capi.check(db._lib.psk_db_add(db._h, sk.name.encode(), sk._h))
        db._names.append(sk.name)
        db._resident.append(False)
        db._n_lazy += 1


def database_of(psk, ref_sets):
    db = psk.Database()
    add_refs(db, sketches_of(psk, db._ctx, ref_sets, "r"))
    return db


def expected_path(mode, n_refs, n_queries, n_ref_markers, max_query):
    """the path screen_many_device takes, restated (one sub-launch)"""
    force = MODES[mode].get("PSK_SCREEN")
    inverted = force == "inv" if force else n_refs * n_queries >= 1 << 18
    if not inverted:
        return "sliced" if max_query > 4 * S.SLICE and n_refs * n_queries <= 1 << 22 else "brute"
    if n_refs > S.INV_LDS_REFS or "PSK_SCREEN_GLOBAL" in MODES[mode]:
        return "inv_global"
    return "inv_lane" if "PSK_SCREEN_WAVE" in MODES[mode] or n_ref_markers == 0 else "inv_wave"


def screen(db, sketches, mode, screen_val, rescue):
    """(pass matrix, sub-launches by path) of one psk_screen_many call under the mode's switches, set and cleared around the call"""
    for k, v in MODES[mode].items():
        os.environ[k] = v
    try:
        db.screen_stats(reset=True)
        got = db.screen_many(sketches, cutoff=screen_val, faster_small=not rescue)
        return got, {k: v for k, v in db.screen_stats().items() if v}
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)


def differing(got, want, rows=()):
    bad = np.flatnonzero((got != want).any(axis=1))
    cells = [(int(q), int(r), bool(got[q, r]), bool(want[q, r])) for q in bad[:6] for r in np.flatnonzero(got[q] != want[q])[:4]]
    return f"{len(bad)} rows differ, first {bad[:12].tolist()}; (query, ref, got, want): {cells}; rows {[(r, bool((got[r] == want[r]).all())) for r in rows if r < len(got)]}"


@pytest.mark.parametrize("name", S.SMALL_CASES)
def test_small_cases_every_path_and_the_single_query(psk, name):
    ref_sets, query_sets, screen_val, rescue, _ = S.case(name)
    want = R.pass_matrix(ref_sets, query_sets, screen_val, rescue)
    counts = R.count_matrix(ref_sets, query_sets)
    db = database_of(psk, ref_sets)
    queries = sketches_of(psk, db._ctx, query_sets, "q")
    n_ref_markers, max_query = sum(len(r) for r in ref_sets), max(len(q) for q in query_sets)
    for mode in SMALL_MODES:
        got, stats = screen(db, queries, mode, screen_val, rescue)
        assert got.shape == want.shape and got.dtype == np.bool_
        assert np.array_equal(got, want), (mode, differing(got, want))
        assert stats == {expected_path(mode, len(ref_sets), len(queries), n_ref_markers, max_query): 1}, mode
    # the same queries one at a time through psk_screen: flags and shared counts
    db.screen_stats(reset=True)
    n = len(ref_sets)
    for qi, q in enumerate(queries):
        flags, shared = np.full(n, 7, np.uint8), np.full(n, 77, np.uint32)
        assert db._lib.psk_screen(db._h, q._h, screen_val, int(rescue), flags.ctypes.data_as(C.c_void_p), shared.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(shared, counts[qi]), (qi, shared.tolist(), counts[qi].tolist())
        assert np.array_equal(flags, want[qi].astype(np.uint8)), qi
    assert {k: v for k, v in db.screen_stats().items() if v} == {"single": len(queries)}


def test_sliced_queries_and_the_same_database_unsliced(psk):
    ref_sets, query_sets, screen_val, rescue, _ = S.sliced()
    want = R.pass_matrix(ref_sets, query_sets, screen_val, rescue)
    db = database_of(psk, ref_sets)
    queries = sketches_of(psk, db._ctx, query_sets, "q")
    for mode in ("brute", "default"):
        got, stats = screen(db, queries, mode, screen_val, rescue)
        assert np.array_equal(got, want), (mode, got.astype(int).tolist())
        assert stats == {"sliced": 1}
    rest = [i for i in range(len(queries)) if i not in S.SLICED_LARGE_QUERIES]      # up to 65 536 markers: a workgroup per pair
    got, stats = screen(db, [queries[i] for i in rest], "brute", screen_val, rescue)
    assert np.array_equal(got, want[rest]) and stats == {"brute": 1}
    # (the inverted paths have no slices: the same matrix)
    for mode in ("inv", "inv_lane", "inv_global"):
        got, stats = screen(db, queries, mode, screen_val, rescue)
        assert np.array_equal(got, want), mode
    flags, shared = np.zeros(3, np.uint8), np.zeros(3, np.uint32)
    assert db._lib.psk_screen(db._h, queries[0]._h, screen_val, 0, flags.ctypes.data_as(C.c_void_p), shared.ctypes.data_as(C.c_void_p)) == 0
    assert shared.tolist() == [8, 0, 0] and flags.tolist() == [1, 0, 0]


# ------------------------------------------------------------------ wide: 36 864 references, then one more
@pytest.fixture(scope="module")
def wide(psk):
    ref_sets, query_sets, screen_val, rescue, _, extra = S.wide()
    db = database_of(psk, ref_sets)
    queries = sketches_of(psk, db._ctx, query_sets, "q")
    want = R.pass_matrix(ref_sets + [extra], query_sets, screen_val, rescue)
    return {"db": db, "queries": queries, "want": want, "extra": extra, "screen_val": screen_val, "rescue": rescue}


WIDE_ROWS = (454, 455, 1819, 1820)      # either side of the second sub-launch's first row: brute (455 queries per launch), inverted (1 820)


@pytest.mark.parametrize("mode,path,launches", [("default", "inv_wave", 2), ("lane", "inv_lane", 2), ("global", "inv_global", 2), ("brute", "brute", 5)])
def test_wide_paths_and_sub_launches(wide, mode, path, launches):
    db, n = wide["db"], S.INV_LDS_REFS
    assert len(db) == n, "runs before test_wide_one_more_reference adds its reference (file order)"
    got, stats = screen(db, wide["queries"], mode, wide["screen_val"], wide["rescue"])
    want = wide["want"][:, :n]
    assert path == expected_path(mode, n, len(wide["queries"]), 1, 24) and stats == {path: launches}
    assert np.array_equal(got, want), differing(got, want, WIDE_ROWS)


def test_wide_one_more_reference_leaves_lds(psk, wide):
    db, n = wide["db"], S.INV_LDS_REFS
    if len(db) == n:
        add_refs(db, sketches_of(psk, db._ctx, [wide["extra"]], "extra"))
    assert len(db) == n + 1
    got, stats = screen(db, wide["queries"], "default", wide["screen_val"], wide["rescue"])
    assert stats == {"inv_global": 2}      # 36 865 counters do not fit the LDS row; (1 << 26) // 36 865 = 1 820 queries per launch still
    assert np.array_equal(got, wide["want"]), differing(got, wide["want"], WIDE_ROWS)
    assert wide["want"][:, n].any() and not wide["want"][:, n].all()


def test_screen_many_refusals_and_empty_calls(psk, wide):
    from pyskani_amd import _capi
    db, lib = wide["db"], wide["db"]._lib
    q = wide["queries"][1]
    flags = np.full(8, 7, np.uint8)
    one = (C.c_void_p * 1)(q._h)
    assert lib.psk_screen_many(None, one, 1, 0.8, 1, flags.ctypes.data_as(C.c_void_p)) == _capi.PSK_EINVAL
    assert lib.psk_screen_many(db._h, None, 1, 0.8, 1, flags.ctypes.data_as(C.c_void_p)) == _capi.PSK_EINVAL
    assert lib.psk_screen_many(db._h, one, 1, 0.8, 1, None) == _capi.PSK_EINVAL
    too_many = (1 << 30) // len(db) + 1
    many = (C.c_void_p * too_many)(*([q._h] * too_many))
    assert lib.psk_screen_many(db._h, many, too_many, 0.8, 1, flags.ctypes.data_as(C.c_void_p)) == _capi.PSK_ELIMIT
    assert b"2^30" in lib.psk_last_error()
    assert lib.psk_screen_many(db._h, one, 0, 0.8, 1, flags.ctypes.data_as(C.c_void_p)) == 0      # no query: nothing written
    empty = psk.Database()
    assert lib.psk_screen_many(empty._h, one, 1, 0.8, 1, flags.ctypes.data_as(C.c_void_p)) == 0  # no reference: nothing written
    assert (flags == 7).all() and empty.screen_many([q]).shape == (1, 0)
    stats = (C.c_uint64 * 8)(*([9] * 8))
    assert lib.psk_ctx_screen_stats(None, stats, 8, 0) == _capi.PSK_EINVAL and lib.psk_ctx_screen_stats(db._ctx._h, None, 8, 0) == _capi.PSK_EINVAL
    assert lib.psk_ctx_screen_stats(db._ctx._h, stats, 8, 0) == 0 and list(stats)[6:] == [0, 0]
    assert list(db.screen_stats()) == ["brute", "sliced", "inv_wave", "inv_lane", "inv_global", "single"]


# ------------------------------------------------------------------ sketches of sequences: the oracle, and the hits of query_many
@pytest.fixture(scope="module")
def sequenced(psk, oracle):
    rng = np.random.default_rng(301)
    a, b = random_genome(rng, 150_000), random_genome(rng, 100_000)
    genomes = [(f"a{i}", [mutate(rng, a, d, 0.0002)]) for i, d in enumerate((0.0, 0.02, 0.05, 0.10, 0.14))]
    genomes += [(f"b{i}", [m[:40_000], m[40_000:]]) for i, m in enumerate(mutate(rng, b, d) for d in (0.0, 0.03, 0.08, 0.14))]
    genomes.append(("short", [random_genome(rng, 6000)]))
    db = psk.Database()
    for name, contigs in genomes:
        db.sketch(name, *contigs)
    queries = genomes + [("nothing", [random_genome(rng, 300)])]      # (a contig below 500 bases is dropped: a sketch without markers)
    sketches = [db._sketch(name, contigs, True) for name, contigs in queries]
    osk = [oracle.Sketch(contigs) for _, contigs in queries]
    assert 0 < len(osk[9].markers) < R.SMALL_MARKER_COUNT and len(osk[10].markers) == 0
    return {"db": db, "names": [n for n, _ in genomes], "sketches": sketches, "osk": osk}


@pytest.mark.parametrize("rescue", [True, False])
def test_sequenced_sketches_match_the_oracle_cell_by_cell(oracle, sequenced, rescue):
    db, osk = sequenced["db"], sequenced["osk"]
    want = np.array([[oracle.screen(q, r, 0.80, rescue)[0] for r in osk[:10]] for q in osk])
    assert np.array_equal(want, R.pass_matrix([s.markers for s in osk[:10]], [s.markers for s in osk], 0.80, rescue))
    assert want[:9, :9].any() and not want[:9, :9].all()
    for mode in SMALL_MODES:
        got, stats = screen(db, sequenced["sketches"], mode, 0.80, rescue)
        assert np.array_equal(got, want), (mode, differing(got, want))
        assert stats == {expected_path(mode, 10, 11, 1, 0): 1}


def test_query_many_hits_lie_in_passing_cells_and_passing_chains_are_hits(oracle, sequenced):
    db, osk, names = sequenced["db"], sequenced["osk"], sequenced["names"]
    sketches = sequenced["sketches"][:10]      # (the markerless one has nothing to chain)
    got, _ = screen(db, sketches, "default", 0.80, True)
    hits = db.query_sketches(sketches, learned_ani=False)
    hit_cells = {(qi, names.index(h.reference_name)) for qi, hs in enumerate(hits) for h in hs}
    assert len(hit_cells) >= 20 and all(got[q, r] for q, r in hit_cells)
    chained = {(int(q), int(r)) for q, r in zip(*np.nonzero(got)) if oracle.chain(osk[r], osk[q]).ani > 0.1}
    assert chained == hit_cells, chained ^ hit_cells


def test_import_refuses_a_marker_beyond_42_bits(psk):
    from pyskani_amd import storage
    ctx = psk.Database()._ctx
    rec = lambda markers: storage.Record(S.PARAMS, "m", np.array([1000], "<u4"), np.zeros(0, storage.SEED_DTYPE), np.array(markers, np.uint64))
    with pytest.raises(ValueError, match="marker 2 "):
        psk.Sketch.from_record(ctx, rec([5, 6, 1 << 42]), markers_only=True)
    ok = psk.Sketch.from_record(ctx, rec([5, 6, (1 << 42) - 1]), markers_only=True)
    assert ok.export()[1].tolist() == [5, 6, (1 << 42) - 1]
