"""Inputs for the tagged blocked seed index (csrc/seed_index.hip psk_bsi_plan, csrc/slice_join.hip): an entry of a tagged index matches a query k-mer when it lies
in the k-mer's bucket (k-mer >> shift, shift <= 8) and its value's top byte equals the k-mer's low byte - no key is read. Plain module:
tests/test_index_tag_cases_cpu.py holds every input to its claim on the oracle alone, tests/test_gpu_index_tag.py runs every case in a process of its own
($PSK_BSI_TAG is read when an index is built: a fresh database per setting) and compares the 80-byte hit records of the tagged, the untagged and the per-pair join byte for byte.

A case is a dict: c, marker_c, k, refs [(name, [contig, ...])], queries [(name, [contig, ...])], planted [(query, reference)] (pairs held to the oracle one by one)
and what its kind adds. Every generator is deterministic (fixed seeds)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

from rerun_cases import FLOAT_FIELDS, INT_FIELDS, K_MARKER
from sq_edges import mutate, random_genome

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BSI_BLOCK = 256           # csrc/common.h: 2^BSI_BLOG references per index block
TAG_C, TAG_MC = 10, 40
MASK64 = np.uint64(0xFFFFFFFFFFFFFFFF)


# ---------------------------------------------------------------------------------------------------------------- k-mers as the oracle sees them
def mm_hash64(key):
    """oracle/skani_oracle.c orc_mm_hash64 on a uint64 array (wrapping arithmetic)"""
    key = np.asarray(key, np.uint64)
    with np.errstate(over="ignore"):
        key = ~(key + (key << np.uint64(21)))
        key = key ^ (key >> np.uint64(24))
        key = (key + (key << np.uint64(3))) + (key << np.uint64(8))
        key = key ^ (key >> np.uint64(14))
        key = (key + (key << np.uint64(2))) + (key << np.uint64(4))
        key = key ^ (key >> np.uint64(28))
        key = key + (key << np.uint64(31))
    return key


def revcomp_kmer(v, k):
    """the 2-bit code (first base in the highest bits) of the reverse complement"""
    v = np.asarray(v, np.uint64)
    out = np.zeros_like(v)
    for i in range(k):
        out = (out << np.uint64(2)) | (np.uint64(3) - ((v >> np.uint64(2 * i)) & np.uint64(3)))
    return out


def is_forward_seed(v, k, c):
    """k-mers that are seeds at compression c AND smaller than their reverse complement: planted as written, the index holds them under this very value"""
    v = np.asarray(v, np.uint64)
    return (mm_hash64(v) < np.uint64(0xFFFFFFFFFFFFFFFF // c)) & (v < revcomp_kmer(v, k))


def kmer_window(rng, v, k):
    """a K_MARKER-base window whose centred k-mer is v (the flanks random)"""
    lo = (K_MARKER - k) // 2      # (orc_sketch_new: off_lo bases before the k-mer, the rest behind it)
    mid = bytes(b"ACGT"[(int(v) >> (2 * (k - 1 - i))) & 3] for i in range(k))
    return random_genome(rng, lo) + mid + random_genome(rng, K_MARKER - k - lo)


def plant_words(rng, kmers, k):
    """every k-mer once, in a window of its own, 25 random bases before each (rerun_cases._planted's spacing)"""
    return b"".join(random_genome(rng, 25) + kmer_window(rng, v, k) for v in kmers)


# ---------------------------------------------------------------------------------------------------------------- block edge
EDGE_FAMILIES, EDGE_PER_FAMILY = 4, 80


def top_tag_kmers(k, c, n):
    """the first n forward seeds whose low byte is 0xFF. A canonical k-mer rarely ends in TTTT (its reverse complement then begins with AAAA and is the smaller
    one, unless the k-mer begins with AAAA too), so a random genome of 25 kb holds none: these are planted"""
    mid = np.arange(1 << (2 * k - 16), dtype=np.uint64)
    v = (mid << np.uint64(8)) | np.uint64(0xFF)      # AAAA, the middle, TTTT
    return v[is_forward_seed(v, k, c)][:n]


def gen_block_edge():
    """320 genomes of 20-30 kb in 4 families of 80, added family after family: the order is the locality order already, and the last family holds slots
    240..319 - astride 255 | 256, the last reference of block 0 (local id 255) and the first of block 1 (local id 0). Those two end in the same four planted
    windows of k-mers with tag 0xFF (tag 0x00 occurs by itself), so local ids 255 and 0 sit beside both extreme tags, in anchors of the pair"""
    rng = np.random.default_rng(9100)
    refs = []
    tail = plant_words(rng, top_tag_kmers(15, TAG_C, 4), 15)
    for f in range(EDGE_FAMILIES):
        root = random_genome(rng, 30000)
        for i in range(EDGE_PER_FAMILY):
            n = int(rng.integers(20000, 30001))
            edge = len(refs) in (BSI_BLOCK - 1, BSI_BLOCK)
            refs.append((f"f{f}_{i}", [mutate(rng, root[:n - len(tail)], 0.02) + tail if edge else mutate(rng, root[:n], 0.02)]))
    return dict(c=TAG_C, marker_c=TAG_MC, k=15, refs=refs, queries=list(refs), planted=[(refs[255][0], refs[256][0]), (refs[256][0], refs[255][0])], kind="block_edge",
                top_tags=[int(x) for x in top_tag_kmers(15, TAG_C, 4)])


# ---------------------------------------------------------------------------------------------------------------- bucket neighbours
NEIGHBOUR_MIN = 32
NEIGHBOUR_KINDS = ("low", "mid", "high")


def neighbour_kmers(seeds, k, c, rng):
    """{kind: k-mers that are forward seeds and no seed of the query}. low: a query seed with other bits 0..7 (its bucket in a tagged index, another tag);
    mid: other bits 8..14, bits 0..7 kept (the same tag - mistaken for the seed by a forced index that kept a shift of 9 or more); high: bits 0..7 kept,
    other bits above (another bucket, the same tag)"""
    seeds = np.unique(np.asarray(seeds, np.uint64))
    out = {}
    top = np.uint64((1 << (2 * k)) - 1)
    for kind in NEIGHBOUR_KINDS:
        if kind == "low":
            cand = (seeds[:, None] & ~np.uint64(0xFF)) | np.arange(256, dtype=np.uint64)[None, :]
        elif kind == "mid":
            cand = (seeds[:, None] & ~np.uint64(0x7F00)) | (np.arange(128, dtype=np.uint64)[None, :] << np.uint64(8))
        else:
            cand = ((rng.integers(0, 1 << (2 * k - 8), (len(seeds), 64)).astype(np.uint64) << np.uint64(8)) | (seeds[:, None] & np.uint64(0xFF))) & top
        cand = np.unique(cand.ravel())
        cand = cand[~np.isin(cand, seeds)]
        out[kind] = cand[is_forward_seed(cand, k, c)]
    return out


def gen_neighbours():
    """one query; "plain" = the query mutated, "planted" = the same bases followed by NEIGHBOUR_MIN or more planted k-mers of every kind; two bystanders. The
    query's seed k-mers are computed here as the oracle computes them (the CPU test holds them to the oracle's)"""
    rng = np.random.default_rng(9200)
    k, c = 15, TAG_C
    q = random_genome(rng, 40000)
    seeds = seed_kmers(q, k, c)
    nb = neighbour_kmers(seeds, k, c, rng)
    plants = {kind: rng.permutation(v)[:NEIGHBOUR_MIN + 8] for kind, v in nb.items()}
    plain = mutate(rng, q, 0.02)
    planted = plain + b"".join(plant_words(rng, plants[kind], k) for kind in NEIGHBOUR_KINDS)
    refs = [("plain", [plain]), ("planted", [planted]), ("far", [mutate(rng, q, 0.06)]), ("none", [random_genome(rng, 40000)])]
    return dict(c=c, marker_c=TAG_MC, k=k, refs=refs, queries=[("q", [q])], planted=[("q", "planted"), ("q", "plain")], kind="neighbours",
                plants={kind: [int(x) for x in v] for kind, v in plants.items()}, query_seeds=[int(x) for x in seeds])


def seed_kmers(seq, k, c):
    """the seed k-mers of one contig (canonical values), as orc_sketch_new selects them"""
    codes = np.frombuffer(seq.translate(bytes.maketrans(b"ACGT", bytes([0, 1, 2, 3]))), np.uint8).astype(np.uint64)
    n = len(codes) - K_MARKER + 1
    start = (K_MARKER - k) // 2      # the k-mer's first base within the window
    f = np.zeros(n, np.uint64)
    for i in range(k):
        f = (f << np.uint64(2)) | codes[start + i:start + i + n]
    cs = np.minimum(f, revcomp_kmer(f, k))
    return cs[mm_hash64(cs) < np.uint64(0xFFFFFFFFFFFFFFFF // c)]


# ---------------------------------------------------------------------------------------------------------------- other k
def gen_other_k(k):
    """all-vs-all of 12 genomes of 100 kb in 3 families (k = 14: 28-bit k-mers, a tagged index has 20-bit bucket tables; k = 16: 32 bits and 24)"""
    rng = np.random.default_rng(9300 + k)
    refs = []
    for f in range(3):
        root = random_genome(rng, 100000)
        refs += [(f"k{k}_f{f}_{i}", [mutate(rng, root, 0.015 * (i + 1))]) for i in range(4)]
    return dict(c=30, marker_c=200, k=k, refs=refs, queries=list(refs), planted=[], kind="other_k")


GENERATORS = {"block_edge": (gen_block_edge, ()), "neighbours": (gen_neighbours, ()), "k14": (gen_other_k, (14,)), "k16": (gen_other_k, (16,))}
_MADE = {}


def case(name):
    if name not in _MADE:
        fn, args = GENERATORS[name]
        _MADE[name] = fn(*args)
    return _MADE[name]


# ---------------------------------------------------------------------------------------------------------------- the runs
SLICE_TAGGED = {"PSK_GSI_SLICE": "1", "PSK_BSI_TAG": "1"}
SLICE_UNTAGGED = {"PSK_GSI_SLICE": "1", "PSK_BSI_TAG": "0"}
PAIRS_TAGGED = {"PSK_GSI_SLICE": "0", "PSK_BSI_TAG": "1"}
CONTIG_JOIN = {"PSK_PROBE": "1", "PSK_JOIN_PAIRS": "1", "PSK_GSI_ONEPASS": "0"}      # rerun_cases.CAPACITY_ROUTES: bsi_two_pass (gsi_join_kernel on the blocked index)


CONFIGS = {"slice_tagged": SLICE_TAGGED, "slice_untagged": SLICE_UNTAGGED, "pairs_tagged": PAIRS_TAGGED, "slice_default": {"PSK_GSI_SLICE": "1"},
           "contig_tagged": dict(CONTIG_JOIN, PSK_BSI_TAG="1"), "contig_untagged": dict(CONTIG_JOIN, PSK_BSI_TAG="0")}


def child_main(name, configs):
    """(in ONE process of its own per case: the suite starts few processes) for every named configuration in turn: its switches set ($PSK_BSI_TAG is read
    whenever an index is built, the others at every call), a fresh database of the case, one query_many call. One JSON line: per configuration the sha256
    over the 80-byte records, the index's layout before and after the call, index lookups and - "slice_tagged" only - the hits' integers"""
    import ctypes as C
    import pyskani_amd as psk
    cs = case(name)
    queries = [(n, *contigs) for n, contigs in cs["queries"]]

    def run(config):
        for k in [k for k in os.environ if k.startswith("PSK_")]:
            del os.environ[k]
        os.environ.update(CONFIGS[config])
        db = psk.Database(compression=cs["c"], marker_compression=cs["marker_c"], k=cs["k"])
        db.sketch_many([(n, *contigs) for n, contigs in cs["refs"]])
        v = [C.c_int(-1) for _ in range(3)]
        assert db._lib.psk_db_seed_index_info(db._h, *[C.byref(x) for x in v]) == 0
        before = [x.value for x in v]
        lk = C.c_uint64()
        assert db._lib.psk_ctx_join_work(db._ctx._h, C.byref(lk), None, None, None, 1) == 0
        res = db.query_many(queries, learned_ani=False)
        assert db._lib.psk_ctx_join_work(db._ctx._h, C.byref(lk), None, None, None, 1) == 0
        assert db._lib.psk_db_seed_index_info(db._h, *[C.byref(x) for x in v]) == 0
        ident = C.c_uint32()
        assert db._lib.psk_db_locality(db._h, None, None, C.byref(ident)) == 0
        h = hashlib.sha256()
        recs = []
        for (qn, *_), hs in zip(queries, res):
            for x in hs:
                h.update(x._raw.tobytes())
                recs.append([qn, x.reference_name] + [int(x._raw[f]) for f in INT_FIELDS] + [repr(float(x._raw[f])) for f in FLOAT_FIELDS])
        return dict(info=[x.value for x in v], info_before=before, lookups=lk.value, identity=ident.value, digest=h.hexdigest(), n_records=len(recs),
                    record_bytes=int(res[0][0]._raw.nbytes) if res and res[0] else 0, records=recs if config == "slice_tagged" else None)
    print(json.dumps({config: run(config) for config in configs}))


def run_child(name, configs, timeout=600):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PSK_")}
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import index_tag_cases; index_tag_cases.child_main(%r, %r)" % (ROOT, os.path.join(ROOT, "tests"), name, list(configs))
    out = subprocess.check_output([sys.executable, "-c", code], env=env, timeout=timeout).decode().strip().splitlines()[-1]
    return json.loads(out)
