"""GPU: the database's locality order (csrc/locality.hip). Families inserted in a shuffled order are grouped again inside the database, so the plan takes the
seed-index joins for them - with the same hits, in the same order, as the insertion-order layout ($PSK_LOCALITY=0) and as the per-pair join; the order itself
is held to the numpy statement of its rule in tests/test_locality_cpu.py. Every setting runs in a process of its own (the switch acts where the order is computed)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COMMON = r"""
import sys, hashlib, json, ctypes as C
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import pyskani_amd as psk
lut = np.frombuffer(b"ACGT", np.uint8)
rng = np.random.default_rng(123)
def mutate(a, d):
    b = a.copy(); m = rng.random(len(a)) < d; b[m] = (b[m] + rng.integers(1, 4, int(m.sum()), dtype=np.uint8)) & 3; return b
def digest(hit_lists, index_of):
    # every chaining integer and the floats, keyed by names; the hits of a query must come in ascending insertion index of their references
    h = hashlib.sha256(); n = 0
    for hs in hit_lists:
        idx = [index_of[x.reference_name] for x in hs]
        assert idx == sorted(idx), "hits are not in ascending insertion order"
        for x in hs:
            r = x._raw
            h.update(repr((x.query_name, x.reference_name, int(r["ref_index"]), int(r["n_anchors"]), int(r["n_chunks"]), int(r["n_intervals"]), int(r["covered_query"]), int(r["covered_ref"]),
                           int(r["sum_chain_anchors"]), int(r["sum_chunk_seeds"]), float(r["ani"]), float(r["af_query"]), float(r["af_ref"]), float(r["ani_std"]))).encode())
            n += 1
    return n, h.hexdigest()
def lookups(db, reset=1):
    lk = C.c_uint64(); db._lib.psk_ctx_join_work(db._ctx._h, C.byref(lk), None, None, None, reset); return lk.value
def is_identity(db):
    v = C.c_uint32(9); assert db._lib.psk_db_locality(db._h, None, None, C.byref(v)) == 0; return v.value
# F families x M members of ~90 kb (c = 30: ~3 000 seeds per genome - a round of mid-sized pairs, the slice join's shape); F * M = 1 600 references = 7 index blocks
F, M, L = 16, 100, 90_000
anc = [rng.integers(0, 4, L, dtype=np.uint8) for _ in range(F)]
ordered = [(f"f{f}_m{j}", lut[mutate(anc[f], 0.0004 * j)].tobytes()) for f in range(F) for j in range(M)]
order = np.random.default_rng(9).permutation(F * M)
shuffled = [ordered[i] for i in order]
fam_of = lambda name: int(name[1:name.index("_")])
""" % (ROOT, os.path.join(ROOT, "tests"))

ALL_VS_ALL = COMMON + r"""
db = psk.Database(compression=30, marker_compression=200)
db.sketch_many(shuffled)
index_of = {n: i for i, (n, _) in enumerate(shuffled)}
lookups(db)
res = db.query_many(shuffled[::2], learned_ani=False)
n, d = digest(res, index_of)
lk = lookups(db)
picks = []
pick = np.random.default_rng(31)
for q in pick.choice(len(res), 8, replace=False):
    hs = [x for x in res[int(q)] if x.reference_name != x.query_name]      # (not the query against itself: ANI 1 checks little)
    x = hs[int(pick.integers(0, len(hs)))]; r = x._raw
    picks.append([x.query_name, x.reference_name] + [int(r[f]) for f in ("n_anchors", "n_chunks", "n_intervals", "covered_query", "covered_ref", "sum_chain_anchors", "sum_chunk_seeds")]
                 + [float(r["ani"]), float(r["af_query"]), float(r["af_ref"])])
print(json.dumps({"n": n, "digest": d, "lookups": lk, "identity": is_identity(db), "picks": picks}))
"""

ORDER = COMMON + r"""
from test_locality_cpu import locality_order
out = {}
db = psk.Database(compression=30, marker_compression=200)
db.sketch_many(shuffled)
slot_of, groups = db.locality()
names = [n for n, _ in shuffled]
want_slot, want_groups = locality_order([r.markers for r in db._marker_records()])
out["perm"] = sorted(slot_of.tolist()) == list(range(F * M))
out["groups"] = groups
out["rule"] = bool((slot_of == want_slot).all()) and groups == want_groups
runs, ascending = True, True
fams = np.array([fam_of(n) for n in names])
for f in range(F):
    sl = slot_of[fams == f]
    runs = runs and int(sl.max()) - int(sl.min()) + 1 == len(sl)
    ascending = ascending and bool((np.diff(sl.astype(np.int64)) > 0).all())
out["runs"], out["ascending"], out["identity_shuffled"] = runs, ascending, is_identity(db)
# one more member of family 0: the order is computed again, the newcomer sits inside its family's run
db.sketch("f0_extra", lut[mutate(anc[0], 0.001)].tobytes())
slot2, groups2 = db.locality()
f0 = slot2[:F * M][fams == 0]
out["extra"] = bool(int(f0.min()) <= int(slot2[F * M]) <= int(f0.max()) + 1) and groups2 == F and len(slot2) == F * M + 1
db2 = psk.Database(compression=30, marker_compression=200)
db2.sketch_many(ordered)
s2, g2 = db2.locality()
out["identity_ordered"] = is_identity(db2); out["ordered_is_arange"] = bool((s2 == np.arange(F * M)).all()); out["groups_ordered"] = g2
print(json.dumps(out))
"""

DUPS = COMMON + r"""
# a shuffled database with names sketched twice (the last sketch of a name wins) ...
refs = list(shuffled[:1200])
for k in (5, 300, 777):
    name = refs[k][0]; f = fam_of(name)
    refs.append((name, lut[mutate(anc[(f + 1) % F], 0.002)].tobytes()))      # the name's LAST sketch belongs to another family
db = psk.Database(compression=30, marker_compression=200)
db.sketch_many(refs)
qs = [refs[5], refs[300], refs[-1], refs[40]]
res = db.query_many(qs, learned_ani=False)
out = {"identity": is_identity(db), "dups": [[(x.reference_name, int(x._raw["ref_index"]), round(float(x._raw["ani"]), 6)) for x in hs] for hs in res]}
# ... and one with references sketched with seed=False: the error names the first such reference a query passes against
db2 = psk.Database(compression=30, marker_compression=200)
db2.sketch_many(shuffled[:700])
for i in (700, 701, 702): db2.sketch(shuffled[i][0], shuffled[i][1], seed=False)
db2.sketch_many(shuffled[703:1200])
try:
    db2.query_many([shuffled[700], shuffled[701], shuffled[3]], learned_ani=False); out["error"] = None
except Exception as e:
    out["error"] = str(e)
print(json.dumps(out))
"""

CONTIGS = COMMON + r"""
# the shuffled database queried with 4 800 short contigs (three in four below 20 markers: rescued, they pass the screen against every reference - 1 600 x 3 600 pairs, the
# prefilter's default range - and go through the contig join: the database-wide index and the blocked one, both laid out by slot)
db = psk.Database(compression=30, marker_compression=200)
db.sketch_many(shuffled)
index_of = {n: i for i, (n, _) in enumerate(shuffled)}
contigs = []
for i in range(4800):
    a = anc[i %% F]; ln = int(rng.integers(1200, 3500)) if i %% 4 else int(rng.integers(6000, 12000)); st = int(rng.integers(0, len(a) - ln))
    contigs.append((f"c{i}", lut[mutate(a[st:st + ln], rng.uniform(0, 0.04))].tobytes()))
lookups(db)
n, d = digest(db.query_many(contigs, learned_ani=False), index_of)
print(json.dumps({"n": n, "digest": d, "lookups": lookups(db), "identity": is_identity(db)}))
""".replace("%%", "%")

LARGE = COMMON + r"""
import time
# 66 000 references of ~21 kb at c = 10 (2 100 seeds: the slice join's range; 258 index blocks, no database-wide index beyond 65 536 references) in families of 50,
# inserted in a random order; genome queries (slice join) and contig queries (contig join and prefilter through the blocks alone)
N, FAM, GL, CC, MC = 66000, 50, 21000, 10, 100
def near(a, n_mut):
    b = a.copy(); p = rng.integers(0, len(a), n_mut); b[p] = (b[p] + rng.integers(1, 4, n_mut, dtype=np.uint8)) & 3; return b
refs = []
for f in range(N // FAM):
    a = rng.integers(0, 4, GL + 500, dtype=np.uint8)
    for j in range(FAM):
        refs.append((f"r{f * FAM + j}", lut[near(a, 30 * j)[: GL + (j * 37) %% 500]].tobytes()))
perm = np.random.default_rng(4).permutation(N)
refs = [refs[i] for i in perm]
index_of = {n: i for i, (n, _) in enumerate(refs)}
db = psk.Database(compression=CC, marker_compression=MC)
db.sketch_many(refs)
t0 = time.perf_counter()
slot_of, groups = db.locality()
t_loc = time.perf_counter() - t0
fams = np.array([int(n[1:]) // FAM for n, _ in refs])
order_by_fam = np.argsort(fams, kind="stable")
sl = slot_of[order_by_fam].reshape(N // FAM, FAM).astype(np.int64)
contiguous = int(((sl.max(1) - sl.min(1) + 1) == FAM).sum())
genomes = [refs[i] for i in range(0, N, 110)]      # 600 genome queries
contigs = []
for j in range(3000):
    i = int(rng.integers(0, N)); g = np.frombuffer(refs[i][1], np.uint8)
    ln = int(rng.integers(GL // 30, GL // 8)); st = int(rng.integers(0, len(g) - ln))
    c = g[st:st + ln].copy(); p = rng.integers(0, ln, ln // 100); c[p] = lut[rng.integers(0, 4, len(p))]
    contigs.append((f"c{j}", c.tobytes()))
lookups(db)
ng, dg = digest(db.query_many(genomes, learned_ani=False), index_of)
nc, dc = digest(db.query_many(contigs, learned_ani=False), index_of)
print(json.dumps({"n": ng + nc, "ng": ng, "nc": nc, "digest": dg + dc, "lookups": lookups(db), "identity": is_identity(db), "groups": groups, "families": N // FAM,
                  "contiguous_families": contiguous, "perm": bool((np.sort(slot_of) == np.arange(N)).all()), "locality_seconds": round(t_loc, 3)}))
""".replace("%%", "%")


def _run(code, extra, timeout=1500):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PSK_")}
    env.update(extra)
    out = subprocess.check_output([sys.executable, "-c", code], env=env, timeout=timeout).decode().strip().splitlines()[-1]
    return json.loads(out)


@pytest.fixture(scope="module")
def all_vs_all():
    return {"default": _run(ALL_VS_ALL, {}), "insertion": _run(ALL_VS_ALL, {"PSK_LOCALITY": "0"}), "per_pair": _run(ALL_VS_ALL, {"PSK_GSI_SLICE": "0", "PSK_GSI_JOIN": "0"})}


def test_shuffled_families_take_the_index_join_and_give_the_same_hits(all_vs_all):
    """1 600 genomes of 16 families inserted in a random order: in insertion order a query's 100 relatives sit in all 7 index blocks and the plan refuses the slice
    join (no index lookups - what every build before the locality order did with this input); in locality order they sit in one or two and the plan takes it."""
    d, ins, pp = all_vs_all["default"], all_vs_all["insertion"], all_vs_all["per_pair"]
    print({k: {f: v[f] for f in ("n", "digest", "lookups", "identity")} for k, v in all_vs_all.items()})
    assert d["n"] >= 800 * 90
    assert (d["n"], d["digest"]) == (ins["n"], ins["digest"]) == (pp["n"], pp["digest"])
    assert d["lookups"] > 0 and d["identity"] == 0
    assert ins["lookups"] == 0 and ins["identity"] == 1
    assert pp["lookups"] == 0


def test_the_order_itself():
    o = _run(ORDER, {})
    print(o)
    assert o["perm"] and o["runs"] and o["ascending"] and o["groups"] == 16 and o["identity_shuffled"] == 0
    assert o["rule"]                      # the GPU's order = the numpy statement of the rule on the database's marker sets
    assert o["extra"]
    assert o["identity_ordered"] == 1 and o["ordered_is_arange"] and o["groups_ordered"] == 16


def test_duplicate_names_and_unseeded_references_in_a_shuffled_database():
    d, ins = _run(DUPS, {}), _run(DUPS, {"PSK_LOCALITY": "0"})
    print(d["identity"], ins["identity"], d["error"])
    assert d["identity"] == 0 and ins["identity"] == 1
    assert d["dups"] == ins["dups"] and all(len(h) > 10 for h in d["dups"])
    assert d["error"] == ins["error"] and "seed=False" in d["error"] and "cannot be chained" in d["error"]


def test_contigs_against_a_shuffled_database():
    """The contig join (gsi_join through the database-wide index and the blocked one), the prefilter of rescued contigs and their slot-ordered pass matrix:
    locality order == insertion order == the probe-table join that reads no seed index."""
    d, ins, probe = _run(CONTIGS, {}), _run(CONTIGS, {"PSK_LOCALITY": "0"}), _run(CONTIGS, {"PSK_GSI_JOIN": "0"})
    print(d, ins, probe)
    assert d["n"] > 4800 * 20
    assert (d["n"], d["digest"]) == (ins["n"], ins["digest"]) == (probe["n"], probe["digest"])
    assert d["identity"] == 0 and ins["identity"] == 1 and probe["identity"] == 0
    assert d["lookups"] > 0 and ins["lookups"] > 0 and probe["lookups"] == 0      # (contigs walk an index in either layout; PSK_GSI_JOIN=0 walks none)


def test_large_shuffled_database():
    """66 000 references in a random order: the order is computed (a permutation; the subprocess's time limit bounds it, the seconds are printed), the blocked index
    is built by slots with no database-wide index beside it, and genome and contig queries give the hits of the insertion-order layout."""
    d = _run(LARGE, {}, timeout=1500)
    print({k: v for k, v in d.items() if k != "digest"})
    ins = _run(LARGE, {"PSK_LOCALITY": "0"}, timeout=1500)
    assert d["perm"] and d["identity"] == 0 and ins["identity"] == 1
    assert d["ng"] > 600 * 30 and d["nc"] > 3000 * 20
    assert (d["n"], d["digest"]) == (ins["n"], ins["digest"])
    assert d["lookups"] > 0


def test_sampled_hits_match_the_oracle(all_vs_all, oracle):
    """8 hits of the default run (locality order, slice join), sampled with a fixed seed, recomputed by the CPU oracle: integers equal, floats to 1e-6. All 8 are checked."""
    import numpy as np
    lut = np.frombuffer(b"ACGT", np.uint8)
    rng = np.random.default_rng(123)

    def mutate(a, d):
        b = a.copy(); m = rng.random(len(a)) < d; b[m] = (b[m] + rng.integers(1, 4, int(m.sum()), dtype=np.uint8)) & 3; return b
    F, M, L = 16, 100, 90_000
    anc = [rng.integers(0, 4, L, dtype=np.uint8) for _ in range(F)]
    genomes = {f"f{f}_m{j}": lut[mutate(anc[f], 0.0004 * j)].tobytes() for f in range(F) for j in range(M)}      # (the children's generator, draw for draw)
    picks = all_vs_all["default"]["picks"]
    assert len(picks) == 8
    for p in picks:
        q, r = p[0], p[1]
        want = oracle.chain(oracle.Sketch([genomes[r]], c=30, marker_c=200), oracle.Sketch([genomes[q]], c=30, marker_c=200))
        for f, got in zip(("n_anchors", "n_chunks", "n_intervals", "covered_query", "covered_ref", "sum_chain_anchors", "sum_chunk_seeds"), p[2:9]):
            assert got == int(getattr(want, f)), (q, r, f, got, int(getattr(want, f)))
        assert abs(p[9] - want.ani) < 1e-6 and abs(p[10] - want.af_query) < 1e-6 and abs(p[11] - want.af_ref) < 1e-6, (q, r, p[9:], want.ani, want.af_query, want.af_ref)
