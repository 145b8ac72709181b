"""GPU: triangle mode (psk_query_many_tri, Database.triangle_records) - every unordered pair of an all-vs-all chained once, no genome against itself.

The reference of every equality here is the FULL all-vs-all of the same database in the same process, `query_handles(handles, n, raw=True)`, filtered on the host to
ref_index > query index: the 80-byte records must be the same bytes, integers and floats alike - the mask only removes cells of the screen's pass matrix, the pairs that
stay go through the same kernels in the same roles. Each setting runs in a process of its own (the $PSK_* switches are read per call, the locality order where it is
computed)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the genomes: families of mutated members (tests/test_gpu_locality.py's generator); exec'd by the children and, for the oracle's sample, by the parent
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
def small_set(): return families(3, 4, 30_000, 0.004)                         # 12 genomes: m * n <= 65 536, the pass rows are counted on the host
def big_set(): return families(4, 80, 60_000, 0.0005, shuffle=9)              # 320 references in a seeded shuffle = 2 index blocks, m * n > 65 536: counted on the device
def contig_set(): return families(6, 10, 2_500, 0.002, seed=5)                # 60 references of 2.5 kb: fewer than 20 markers at the default marker compression
"""

COMMON = r"""
import sys, json, ctypes as C
sys.path.insert(0, %r)
import pyskani_amd as psk
from pyskani_amd.database import triangle_matrix
""" % ROOT + GENOMES + r"""
INTS = ("n_anchors", "n_chunks", "n_intervals", "covered_query", "covered_ref", "sum_chain_anchors", "sum_chunk_seeds")
def work(db, reset=1):
    p, i, a = C.c_uint64(), C.c_uint64(), C.c_uint64(); assert db._lib.psk_ctx_work(db._ctx._h, C.byref(p), C.byref(i), C.byref(a), reset) == 0; return p.value
def is_identity(db):
    v = C.c_uint32(9); assert db._lib.psk_db_locality(db._h, None, None, C.byref(v)) == 0; return v.value
def with_query(recs, offs):
    # raw records carry no query index (`reserved` is 0 as the library returns them): written here, as triangle_records writes it
    assert (recs["reserved"] == 0).all()
    recs = recs.copy(); recs["reserved"] = np.repeat(np.arange(len(offs) - 1, dtype=np.uint32), np.diff(offs)); return recs
def full_and_triangle(db, **kw):
    # the full all-vs-all, its filter to ref_index > query, the triangle, and the pairs each of the two calls chained
    n = len(db)
    work(db)
    full, foffs = db.query_handles(db.sketch_handles(), n, raw=True, learned_ani=False, **kw)
    pairs_full = work(db)
    tri, toffs = db.triangle_records(raw=True, learned_ani=False, **kw)
    pairs_tri = work(db)
    full = with_query(full, foffs)
    want = full[full["ref_index"] > full["reserved"]]
    return full, want, tri, toffs, pairs_full, pairs_tri
def compare(want, tri, toffs, n):
    # records equal byte for byte; offsets of n + 1 entries that end at the filtered count and cut the records by query; nothing on or below the diagonal
    out = {"n_want": int(len(want)), "n_tri": int(len(tri)), "equal": bool(len(want) == len(tri) and want.tobytes() == tri.tobytes()),
           "offsets_len": int(len(toffs)), "offsets_last": int(toffs[-1]),
           "offsets_cut": bool(np.array_equal(toffs, np.searchsorted(tri["reserved"], np.arange(n + 1)))),
           "below": int((tri["ref_index"] <= tri["reserved"]).sum()),
           "sorted": bool((np.diff(tri["reserved"].astype(np.int64) * (1 << 32) + tri["ref_index"]) > 0).all())}
    if not out["equal"]:      # what differs, for the log
        for f in want.dtype.names:
            if len(want) == len(tri) and not np.array_equal(want[f], tri[f]): print("field", f, "differs in", int((want[f] != tri[f]).sum()), "records", file=sys.stderr)
    return out
"""

SMALL = COMMON + r"""
g = small_set(); n = len(g)
db = psk.Database(compression=30, marker_compression=200)
db.sketch_many(g)
full, want, tri, toffs, pairs_full, pairs_tri = full_and_triangle(db)
out = compare(want, tri, toffs, n)
out.update(n=n, pairs_full=pairs_full, pairs_tri=pairs_tri, self_hits=int((full["ref_index"] == full["reserved"]).sum()))
# min records: the same hits, `query` = the insertion index
tmin, moffs = db.triangle_records(learned_ani=False)
out["min_equal"] = bool(np.array_equal(moffs, toffs) and all(np.array_equal(tmin[f], tri[f]) for f in ("ani", "af_query", "af_ref", "ref_index")) and np.array_equal(tmin["query"], tri["reserved"]))
# Database.triangle(): Hits by insertion index, names and the three numbers of the records
hits = db.triangle(learned_ani=False)
names = [x for x, _ in g]
flat = [(i, h) for i, hs in enumerate(hits) for h in hs]
out["hits_len"] = len(hits)
out["hits_equal"] = bool(len(flat) == len(tri) and all(h.query_name == names[i] == names[int(r["reserved"])] and h.reference_name == names[int(r["ref_index"])] and h.identity == float(r["ani"])
                                                      and h.query_fraction == float(r["af_query"]) and h.reference_fraction == float(r["af_ref"]) for (i, h), r in zip(flat, tri)))
# the dense form of the triangle against the dense form of the full run
ani, af = triangle_matrix(tri, n)
fa = np.zeros((n, n), np.float32); fa[full["reserved"], full["ref_index"]] = full["ani"]
out["matrix_upper"] = bool(np.array_equal(np.triu(ani, 1), np.triu(fa, 1)) and np.array_equal(ani, ani.T) and (np.diag(ani) == 1).all())

# ---- keys and base: A = genomes [0, 5), B = [5, 12); all 12 sketches against each, keys = their indices in the whole set
whole = db.sketch_handles()
A = psk.Database(compression=30, marker_compression=200); A.sketch_many(g[:5])
B = psk.Database(compression=30, marker_compression=200); B.sketch_many(g[5:])
ra, oa = A.query_handles(whole, n, raw=True, learned_ani=False, keys=range(n), ref_base=0)
rb, ob = B.query_handles(whole, n, raw=True, learned_ani=False, keys=list(range(n)), ref_base=5)
ra, rb = with_query(ra, oa), with_query(rb, ob)
rb["ref_index"] += 5
merged = np.concatenate([ra, rb])
merged = merged[np.lexsort((merged["ref_index"], merged["reserved"]))]
out["ab_parts"] = [int(len(ra)), int(len(rb))]
out["ab_equal"] = bool(len(merged) == len(tri) and merged.tobytes() == tri.tobytes())
# every key -1: the plain call
plain, poffs = db.query_handles(whole, n, raw=True, learned_ani=False)
neg, noffs = db.query_handles(whole, n, raw=True, learned_ani=False, keys=[-1] * n, ref_base=0)
out["neg_equal"] = bool(np.array_equal(poffs, noffs) and plain.tobytes() == neg.tobytes() and len(plain) == len(full))
# a key >= ref_base + n - 1 leaves its query nothing; the queries beside it keep their plain rows (key -1) or their triangle rows
keys = np.full(n, -1, np.int64); keys[3] = n - 1; keys[7] = 10 ** 12; keys[2] = 2
mix, xoffs = db.query_handles(whole, n, raw=True, learned_ani=False, keys=keys, ref_base=0)
mix = with_query(mix, xoffs)
want_mix = full[(keys[full["reserved"]] < 0) | (full["ref_index"].astype(np.int64) > keys[full["reserved"]])]
out["mix_empty"] = [int(xoffs[4] - xoffs[3]), int(xoffs[8] - xoffs[7])]
out["mix_equal"] = bool(mix.tobytes() == want_mix.tobytes())
kb = np.arange(n, dtype=np.int64) + 5; kb[9] = 5 + len(B) - 1
rb2, ob2 = B.query_handles(whole, n, raw=True, learned_ani=False, keys=kb, ref_base=5)      # (sketch i of the whole set as if it were 5 places further on)
out["base_last_key"] = int(ob2[10] - ob2[9])

# ---- boundary behaviour
def raises(exc, fn):
    try: fn()
    except exc: return True
    except Exception as e: return repr(e)
    return False
D = psk.Database(compression=30, marker_compression=200); D.sketch_many(g[:4]); D.sketch(g[1][0], g[5][1])
out["dup_raises"] = raises(ValueError, lambda: D.triangle_records(learned_ani=False))
E = psk.Database(compression=30, marker_compression=200)
r0, o0 = E.triangle_records(learned_ani=False, raw=True)
out["empty"] = [int(len(r0)), o0.tolist(), r0.dtype.itemsize, E.triangle(learned_ani=False)]
E.sketch(*g[0])
r1, o1 = E.triangle_records(learned_ani=False)
out["one"] = [int(len(r1)), o1.tolist(), r1.dtype.itemsize, E.triangle(learned_ani=False)]
class NoLib:
    def __getattr__(self, name): raise AssertionError("library call " + name)
lib = db._lib; db._lib = NoLib()
try: out["keys_len_raises"] = [raises(ValueError, lambda: db.query_handles(whole, n, keys=list(range(n - 1)))), raises(ValueError, lambda: db.query_handles(whole, n, keys=list(range(n + 1))))]
finally: db._lib = lib
# the C entry points' own argument checks
opts = db._opts(False, False, False, None, False)
hp, offs = C.POINTER(psk._capi.Hit)(), (C.c_uint64 * (n + 1))()
out["null_keys_status"] = lib.psk_query_many_tri(db._h, whole, n, None, 0, C.byref(opts), C.byref(hp), offs)
k64 = (C.c_int64 * n)(*range(n))
out["limit_status"] = lib.psk_query_many_tri(db._h, whole, n, k64, (1 << 63) - n + 1, C.byref(opts), C.byref(hp), offs)
print(json.dumps(out))
"""

BIG = COMMON + r"""
g = big_set(); n = len(g)
db = psk.Database(compression=30, marker_compression=200)
db.sketch_many(g)
full, want, tri, toffs, pairs_full, pairs_tri = full_and_triangle(db)
out = compare(want, tri, toffs, n)
out.update(n=n, pairs_full=pairs_full, pairs_tri=pairs_tri, identity=is_identity(db))
lk = C.c_uint64(); db._lib.psk_ctx_join_work(db._ctx._h, C.byref(lk), None, None, None, 1); out["lookups"] = lk.value
names = [x for x, _ in g]
pick = np.random.default_rng(31).choice(len(tri), 6, replace=False)
out["picks"] = [[names[int(r["reserved"])], names[int(r["ref_index"])]] + [int(r[f]) for f in INTS] + [float(r["ani"]), float(r["af_query"]), float(r["af_ref"])] for r in tri[np.sort(pick)]]
print(json.dumps(out))
"""

CONTIGS = COMMON + r"""
g = contig_set(); n = len(g)
db = psk.Database()      # the defaults: c = 125, marker compression 1 000 - a 2.5 kb reference has two or three markers and is rescued against everything
db.sketch_many(g)
out = {"markers_max": int(max(len(r.markers) for r in db._marker_records()))}
full, want, tri, toffs, pairs_full, pairs_tri = full_and_triangle(db, faster_small=False)
out.update(compare(want, tri, toffs, n))
out.update(n=n, pairs_full=pairs_full, pairs_tri=pairs_tri)
print(json.dumps(out))
"""


def _run(code, extra, timeout=600):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PSK_")}
    env.update(extra)
    out = subprocess.check_output([sys.executable, "-c", code], env=env, timeout=timeout).decode().strip().splitlines()[-1]
    return json.loads(out)


def _check_equal(o):
    print({k: v for k, v in o.items() if k != "picks"})
    assert o["n_want"] > 0, "the full run has no hit above the diagonal: nothing is compared"
    assert o["equal"] and o["n_tri"] == o["n_want"]
    assert o["offsets_len"] == o["n"] + 1 and o["offsets_last"] == o["n_want"] and o["offsets_cut"]
    assert o["below"] == 0 and o["sorted"]
    # the pairs were never chained, not dropped afterwards: the screen is symmetric and every genome passes itself
    assert (o["pairs_full"] - o["n"]) % 2 == 0 and o["pairs_tri"] == (o["pairs_full"] - o["n"]) // 2, (o["pairs_full"], o["pairs_tri"], o["n"])


@pytest.fixture(scope="module")
def small():
    return _run(SMALL, {})


def test_small_round_counted_on_the_host(small):
    """12 genomes = 3 families x 4 of 30 kb: m * n <= 65 536, the pass rows cross and are counted on the host."""
    _check_equal(small)
    assert small["n"] == 12 and small["self_hits"] == 12
    assert small["n_want"] >= 3 * 6                                       # every pair of a family
    assert small["min_equal"] and small["matrix_upper"]


def test_keys_and_base(small):
    """The 12 sketches against A = genomes [0, 5) with ref_base 0 and B = [5, 12) with ref_base 5, keys = their indices in the whole set: merged by (query, reference)
    the two results are the whole database's triangle. Every key -1: the plain call. A key >= ref_base + n - 1: no hit for that query."""
    print({k: small[k] for k in ("ab_parts", "ab_equal", "neg_equal", "mix_empty", "mix_equal", "base_last_key")})
    assert small["ab_equal"] and min(small["ab_parts"]) > 0
    assert small["neg_equal"]
    assert small["mix_empty"] == [0, 0] and small["mix_equal"]
    assert small["base_last_key"] == 0


def test_boundary_behaviour(small):
    print({k: small[k] for k in ("dup_raises", "empty", "one", "keys_len_raises", "hits_len", "hits_equal", "null_keys_status", "limit_status")})
    assert small["dup_raises"] is True                                    # a name sketched twice: ValueError
    assert small["empty"] == [0, [0], 80, []] and small["one"] == [0, [0, 0], 20, [[]]]      # no record, offsets of n + 1 entries, the record type asked for
    assert small["keys_len_raises"] == [True, True]                       # wrong length: ValueError before any library call
    assert small["hits_len"] == 12 and small["hits_equal"]                # Database.triangle(): Hits whose names and three numbers are the records'
    assert small["null_keys_status"] == 1 and small["limit_status"] == 6  # PSK_EINVAL, PSK_ELIMIT


@pytest.fixture(scope="module")
def sliced():
    return _run(BIG, {"PSK_GSI_SLICE": "1"})


def test_device_counted_round_in_locality_order_through_the_slice_join(sliced):
    """4 families x 80 members of 60 kb in a seeded shuffle: 320 references = 2 index blocks, m * n > 65 536 (pass rows counted on the device), a locality order that
    is not the identity - the mask acts on the insertion-order matrix BEFORE the gather into slot order - and the slice join."""
    assert sliced["identity"] == 0
    assert sliced["lookups"] > 0                                          # (the index join ran)
    _check_equal(sliced)
    assert sliced["n"] == 320 and sliced["n_want"] >= 4 * 80 * 79 // 2


def test_rounds(sliced):
    """PSK_ROUND_QUERIES=7: 46 rounds; the key of a round's query i is key[b + i]."""
    o = _run(BIG, {"PSK_ROUND_QUERIES": "7"})
    _check_equal(o)
    assert o["n_want"] == sliced["n_want"]


def test_two_lanes(sliced):
    o = _run(BIG, {"PSK_PIPELINE": "1", "PSK_GSI_SLICE": "1", "PSK_BATCH_ITEMS_LOG2": "18"})      # several batches on both lanes
    _check_equal(o)
    assert o["n_want"] == sliced["n_want"] and o["lookups"] > 0


def test_per_pair_join(sliced):
    o = _run(BIG, {"PSK_GSI_SLICE": "0", "PSK_GSI_JOIN": "0"})
    _check_equal(o)
    assert o["n_want"] == sliced["n_want"] and o["lookups"] == 0


def test_rescued_contigs_with_the_prefilter():
    """60 references of 2.5 kb at the default compressions: fewer than 20 markers each, so every pair passes the screen and the prefilter of rescued contigs (forced:
    PSK_PREFILTER=1) takes out those that cannot chain - after the triangle's mask, on the same matrix."""
    o = _run(CONTIGS, {"PSK_PREFILTER": "1"})
    assert 0 < o["markers_max"] < 20
    _check_equal(o)      # (the anchor count of a pair is the same from either side, and a contig has MIN_ANCHORS seeds in common with itself: the prefilter keeps the matrix symmetric)
    assert o["pairs_full"] < o["n"] * o["n"]                              # (the prefilter took pairs out: without it every one of the 3 600 is chained)


def test_sampled_triangle_hits_match_the_oracle(sliced, oracle):
    """6 hits of the triangle (locality order, slice join), sampled with a fixed seed, recomputed by the CPU oracle: every chain integer equal, floats to 1e-6."""
    ns = {}
    exec(GENOMES, ns)
    genomes = dict(ns["big_set"]())                                       # (the children's generator, draw for draw)
    picks = sliced["picks"]
    assert len(picks) == 6
    for p in picks:
        q, r = p[0], p[1]
        want = oracle.chain(oracle.Sketch([genomes[r]], c=30, marker_c=200), oracle.Sketch([genomes[q]], c=30, marker_c=200))
        for f, got in zip(("n_anchors", "n_chunks", "n_intervals", "covered_query", "covered_ref", "sum_chain_anchors", "sum_chunk_seeds"), p[2:9]):
            assert got == int(getattr(want, f)), (q, r, f, got, int(getattr(want, f)))
        assert abs(p[9] - want.ani) < 1e-6 and abs(p[10] - want.af_query) < 1e-6 and abs(p[11] - want.af_ref) < 1e-6, (q, r, p[9:], want.ani, want.af_query, want.af_ref)
