"""Inputs for the two walks of the slice join (csrc/slice_join.hip gsl_walk_kernel): what a walk wave does once per index block - the table from a block's local
reference to the entry's pair slot - and once per query seed - the cursor that deals a seed's index run out in steps of 64 entries. Plain module:
tests/test_walk_cases_cpu.py holds every input to its claim on the oracle and numpy alone, tests/test_gpu_walk_cases.py runs the database in one process of its own
and compares the 80-byte hit records of the tagged index, the untagged index and the per-pair join byte for byte.

ONE database, added family after family so that the locality order is the identity (the GPU test asserts it):
  slots   0..39    40 unrelated genomes: every one's only pair is itself (P = 1)
  slots  40..231   families of 63, 64 and 65 members: entries of exactly 63, 64 and 65 pairs
  slots 232..531   a family of 300 at 2 % divergence: 24 references at the end of block 0 (local ids 232..255), all 256 of block 1, 20 at the start of block 2.
                   A query of it has TWO entries: ranks 0..255 (blocks 0 and 1, ending at local id 231 of block 1) and ranks 256..299 (rank_lo = 256: from local id
                   232 of block 1 into block 2) - so block 1 is walked by both, with passing references below rank_lo in one and at or above rank_hi in the other,
                   slots 0 and 255, local ids 0, 31, 32 and 255, P = 256 and P = 44.
The queries: every reference, and four built ones.
  qa  a member of the 300 followed by planted windows whose k-mers are held by exactly 1, 63, 64, 65, 128, 129 and 256 references of block 1 (the same window in the
      block's first that many members): runs of one step less one entry, one step, one step and one entry, two steps, ... On the TAGGED index (buckets of 256
      k-mers) the k-mers are chosen so that their bucket holds nothing else in any block: the run is exactly that long. The untagged index of a database this small
      has buckets 32 times as wide, whose other k-mers lengthen the run on both sides.
  qb  the same member with 3 kb of random sequence in its middle: ~300 seeds in a row that no reference holds. Their buckets are seldom empty in the full blocks;
      in block 2 (20 references) most are: whole 64-seed batches without a run, and lanes without a run beside lanes with one everywhere else.
  qc  a member followed by two k-mers of 64 references each: c1 is held once by block 1's first 63 members and TWICE by the 64th (entries 63 and 64 of its run on the
      tagged index: a (seed, reference) group cut by the step boundary, on the emit walk's dup path); c2 twice by the FIRST member and once by the next 63.
  qd  1 800 bases of a member: 200 seeds or fewer - less than one 256-seed slice, and its last 64-seed batch is partial.
`planted` lists the (query, reference) pairs of qa, qb and qc that are held to the oracle one by one.

index_tag_cases.run_child starts that module's own child_main, which knows its own cases only and reports no work per query: the child here is its twin (same switches per
configuration - CONFIGS is imported -, same record digest) plus the index entries visited by qa alone."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

from index_tag_cases import BSI_BLOCK, CONFIGS, is_forward_seed, plant_words, seed_kmers
from rerun_cases import FLOAT_FIELDS, INT_FIELDS
from sq_edges import mutate, random_genome

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALK_C, WALK_MC, WALK_K = 10, 40, 15
N_UNRELATED, SMALL_FAMILIES, BIG = 40, (63, 64, 65), 300
BIG_SLOT0 = N_UNRELATED + sum(SMALL_FAMILIES)      # 232
B1_FIRST = BSI_BLOCK - BIG_SLOT0                   # 24: the member of the 300 that is block 1's local reference 0
RUN_LENGTHS = (1, 63, 64, 65, 128, 129, 256)
TAG_SHIFT = 8                                      # a tagged index' buckets: k-mer >> 8
INSERT_AT, INSERT_LEN = 12000, 3000
DUP_GAP = 200


def _word(rng, v):
    """25 random bases and the window of k-mer v (index_tag_cases.kmer_window): the SAME bytes in every member that holds it"""
    return plant_words(rng, [v], WALK_K)


def _free_kmers(rng, taken_buckets, n):
    """n forward seeds whose tagged bucket no seed of the database's genomes lies in, in buckets of their own"""
    out = []
    while len(out) < n:
        cand = rng.integers(0, 1 << (2 * WALK_K), 4096).astype(np.uint64)
        cand = cand[is_forward_seed(cand, WALK_K, WALK_C)]
        for v in cand:
            b = int(v) >> TAG_SHIFT
            if b not in taken_buckets and len(out) < n:
                taken_buckets.add(b)
                out.append(int(v))
    return out


def gen_walk():
    rng = np.random.default_rng(9400)
    refs = [(f"u{i}", random_genome(rng, int(rng.integers(20000, 30001)))) for i in range(N_UNRELATED)]
    for m in SMALL_FAMILIES:
        root = random_genome(rng, 30000)
        refs += [(f"s{m}_{i}", mutate(rng, root[:int(rng.integers(20000, 30001))], 0.02)) for i in range(m)]
    root = random_genome(rng, 29000)      # (the planted tails are below 1 kb: every genome stays within 20-30 kb)
    big = [mutate(rng, root[:int(rng.integers(20000, 29001))], 0.02) for _ in range(BIG)]
    qbase = mutate(rng, root[:25000], 0.02)
    held = np.unique(np.concatenate([seed_kmers(g, WALK_K, WALK_C) for g in [g for _, g in refs] + big + [qbase]]))
    insert = random_genome(rng, INSERT_LEN)
    while np.isin(seed_kmers(insert, WALK_K, WALK_C), held).any():      # (300 seeds against 1.3 M of 2^30: one draw in three holds one by chance)
        insert = random_genome(rng, INSERT_LEN)
    taken = set((np.concatenate([held, seed_kmers(insert, WALK_K, WALK_C)]) >> np.uint64(TAG_SHIFT)).tolist())
    kmers = _free_kmers(rng, taken, len(RUN_LENGTHS) + 2)
    run_kmers, (c1, c2) = dict(zip(RUN_LENGTHS, kmers)), kmers[len(RUN_LENGTHS):]
    words = {n: _word(rng, v) for n, v in run_kmers.items()}
    w1, w2 = _word(rng, c1), _word(rng, c2)

    def twice(w):      # the window again, DUP_GAP bases after its first copy
        return w + random_genome(rng, DUP_GAP - len(w) + 25) + w[25:]
    for i in range(BIG):
        j = i - B1_FIRST      # local reference of block 1
        tail = b""
        if 0 <= j < BSI_BLOCK:
            tail += b"".join(words[n] for n in RUN_LENGTHS if j < n)
            if j < 64:
                tail += twice(w1) if j == 63 else w1
                tail += twice(w2) if j == 0 else w2
        refs.append((f"b{i}", big[i] + tail))
    all_words = b"".join(words[n] for n in RUN_LENGTHS)
    qa = qbase + all_words
    qb = qbase[:INSERT_AT] + insert + qbase[INSERT_AT:] + all_words
    qc = mutate(rng, root[:25000], 0.02) + w1 + w2
    qd = mutate(rng, root[:1800], 0.02)
    first, doubled = f"b{B1_FIRST}", f"b{B1_FIRST + 63}"
    refs = [(n, [g]) for n, g in refs]
    queries = list(refs) + [("qa", [qa]), ("qb", [qb]), ("qc", [qc]), ("qd", [qd])]
    planted = [("qa", first), ("qa", f"b{B1_FIRST + 255}"), ("qb", first), ("qc", doubled), ("qc", first)]
    return dict(c=WALK_C, marker_c=WALK_MC, k=WALK_K, refs=refs, queries=queries, planted=planted, kind="walk", run_kmers=run_kmers, c1=c1, c2=c2,
                insert=insert, first=first, doubled=doubled)


_MADE = {}


def case(name="walk"):
    if name not in _MADE:
        _MADE[name] = gen_walk()
    return _MADE[name]


def run_lengths(q_kmers, block_kmers, shift):
    """per query seed the length of its index run in a block: the block's seeds in the seed's bucket (k-mer >> shift)"""
    b, n = np.unique(np.asarray(block_kmers, np.uint64) >> np.uint64(shift), return_counts=True)
    qb = np.asarray(q_kmers, np.uint64) >> np.uint64(shift)
    at = np.minimum(np.searchsorted(b, qb), len(b) - 1)
    return np.where(b[at] == qb, n[at], 0)


def entries_visited(q_kmers, ref_kmers, passing, shift):
    """index entries in the runs the count walk of one query finds (psk_ctx_join_work's `visited`): the query's passing references, in slot order, are cut into
    entries of BSI_BLOCK pairs; an entry walks every index block that holds one of its references, and in a block every query seed finds its bucket's run"""
    passing = sorted(passing)
    total = 0
    for e0 in range(0, len(passing), BSI_BLOCK):
        for blk in sorted({s // BSI_BLOCK for s in passing[e0:e0 + BSI_BLOCK]}):
            held = np.concatenate([ref_kmers[s] for s in range(blk * BSI_BLOCK, min((blk + 1) * BSI_BLOCK, len(ref_kmers)))])
            total += int(run_lengths(q_kmers, held, shift).sum())
    return total


# ---------------------------------------------------------------------------------------------------------------- the runs
def child_main(configs):
    """(in ONE process) for every named configuration in turn: its switches set, a fresh database, one query_many call over all queries; in "slice_untagged" a
    second call with qa alone, for the index entries its count walk visits. One JSON line"""
    import ctypes as C
    import pyskani_amd as psk
    cs = case()
    queries = [(n, *contigs) for n, contigs in cs["queries"]]

    def work(db, reset):
        lk, vis = C.c_uint64(), C.c_uint64()
        assert db._lib.psk_ctx_join_work(db._ctx._h, C.byref(lk), C.byref(vis), None, None, reset) == 0
        return lk.value, vis.value

    def run(config):
        for k in [k for k in os.environ if k.startswith("PSK_")]:
            del os.environ[k]
        os.environ.update(CONFIGS[config])
        db = psk.Database(compression=cs["c"], marker_compression=cs["marker_c"], k=cs["k"])
        db.sketch_many([(n, *contigs) for n, contigs in cs["refs"]])
        work(db, 1)
        res = db.query_many(queries, learned_ani=False)
        lookups, _ = work(db, 1)
        v = [C.c_int(-1) for _ in range(3)]
        assert db._lib.psk_db_seed_index_info(db._h, *[C.byref(x) for x in v]) == 0
        ident = C.c_uint32()
        assert db._lib.psk_db_locality(db._h, None, None, C.byref(ident)) == 0
        h = hashlib.sha256()
        recs = []
        for (qn, *_), hs in zip(queries, res):
            for x in hs:
                h.update(x._raw.tobytes())
                recs.append([qn, x.reference_name] + [int(x._raw[f]) for f in INT_FIELDS] + [repr(float(x._raw[f])) for f in FLOAT_FIELDS])
        out = dict(info=[x.value for x in v], lookups=lookups, identity=ident.value, digest=h.hexdigest(), n_records=len(recs),
                   record_bytes=int(res[0][0]._raw.nbytes) if res and res[0] else 0, records=recs if config == "slice_tagged" else None)
        if config == "slice_untagged":
            qa = [q for q in queries if q[0] == "qa"]
            out["qa_hits"] = [x.reference_name for x in db.query_many(qa, learned_ani=False)[0]]
            out["qa_lookups"], out["qa_visited"] = work(db, 1)
        return out
    print(json.dumps({config: run(config) for config in configs}))


def run_walk_child(configs, timeout=600):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PSK_")}
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import walk_cases; walk_cases.child_main(%r)" % (ROOT, os.path.join(ROOT, "tests"), list(configs))
    out = subprocess.check_output([sys.executable, "-c", code], env=env, timeout=timeout).decode().strip().splitlines()[-1]
    return json.loads(out)
