"""GPU: the slice join's 8-byte anchors (q pos relative to the head of its chunk, ref contig << 1 | strand, r pos; csrc/chain_dev.h pk_anchor) against the
per-pair join's 16-byte records (PSK_GSI_SLICE=0). The batch is built to reach the edges of the packed record: anchors exactly FRAGMENT_LENGTH after their
chunk's head and the first one beyond it (which opens a new row), chunks that span slice boundaries (256 query seeds), reverse-strand matches, a
reference that holds a segment six times over 20 kb (several anchors per (seed, pair) - the emit walk's dup branch - and chunks with more chain trees than the
lane kernel keeps: chain_chunk_list_kernel), multi-contig queries and references (a reference contig index above 255) and reference positions above 2^24.
Every DP kernel that runs after the slice join is forced in turn; every hit must be identical, and a sample is held to the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAGMENT_LENGTH = 20000

GENOMES = r"""
import numpy as np
lut = np.frombuffer(b"ACGT", np.uint8)
rng = np.random.default_rng(2031)
def mutate(a, d):
    b = a.copy(); m = rng.random(len(a)) < d; b[m] = (b[m] + rng.integers(1, 4, int(m.sum()), dtype=np.uint8)) & 3; return b
def rc(a): return (3 - a)[::-1].copy()
def enc(parts): return [lut[p].tobytes() for p in parts]
big = rng.integers(0, 4, 17_200_000, dtype=np.uint8)                      # reference positions up to 17.2 M > 2^24
rep = rng.integers(0, 4, 3_000, dtype=np.uint8)
mid = np.concatenate([rng.integers(0, 4, 300_000, dtype=np.uint8), rep, rng.integers(0, 4, 300_000, dtype=np.uint8)])
six = np.concatenate([mid[:100_000]] + [np.concatenate([mutate(rep, 0.004), rng.integers(0, 4, 400, dtype=np.uint8)]) for _ in range(6)] + [mid[100_000:]])
genomes = [
    ("big0", enc([big])), ("big1", enc([mutate(big, 0.004)])), ("big_rc", enc([rc(mutate(big, 0.002))])),
    ("mid0", enc([mid])), ("mid1", enc([mutate(mid, 0.003)])), ("mid_rc", enc([rc(mutate(mid, 0.002))])),
    ("mid_300", enc(np.array_split(mutate(mid, 0.001), 300))),            # 300 contigs of ~2 kb: reference contig indices up to 299
    ("mid_3", enc(np.split(mutate(mid, 0.002), [150_000, 151_000]))),     # three contigs, one of them a single chunk
    ("mid_six", enc([six])),                                             # the repeat six times within 20 kb
]
"""

RUN = r"""
import sys, hashlib, ctypes as C
sys.path.insert(0, %r)
import pyskani_amd as psk
""" % (ROOT,) + GENOMES + r"""
c = int(sys.argv[1])
db = psk.Database(compression=c, marker_compression=max(c, 200))
db.sketch_many([(n, *g) for n, g in genomes])
lk = C.c_uint64(); db._lib.psk_ctx_join_work(db._ctx._h, C.byref(lk), None, None, None, 1)
res = db.query_many([(n, *g) for n, g in genomes], learned_ani=False)
db._lib.psk_ctx_join_work(db._ctx._h, C.byref(lk), None, None, None, 1)
h = hashlib.sha256(); n = 0
for hs in res:
    for x in hs:
        r = x._raw
        h.update(repr((x.reference_name, int(r["n_anchors"]), int(r["n_chunks"]), int(r["n_intervals"]), int(r["covered_query"]), int(r["covered_ref"]),
                       int(r["sum_chain_anchors"]), int(r["sum_chunk_seeds"]), float(r["ani"]), float(r["af_query"]), float(r["af_ref"]), float(r["ani_std"]))).encode())
        n += 1
print(n, h.hexdigest(), lk.value)
"""


def _run(c, extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PSK_")}
    env.update(extra)
    out = subprocess.check_output([sys.executable, "-c", RUN, str(c)], env=env, timeout=900).decode().split()
    return int(out[0]), out[1], int(out[2])


def test_packed_anchors_match_the_per_pair_join_in_every_dp_kernel():
    n, d, lookups = _run(125, {"PSK_GSI_SLICE": "1"})
    assert lookups > 0                      # the slice join ran
    assert n >= 3 * 3 + 6 * 6               # every genome finds its family
    ref = _run(125, {"PSK_GSI_SLICE": "0"})
    assert ref[2] == 0 and ref[:2] == (n, d)
    # lane kernel (default above), quad kernel, wave-register kernel, wave-per-chunk kernel, the lane-serial path, the lane kernel with LDS tree slots
    for extra in ({"PSK_CHAIN_LANE": "q"}, {"PSK_CHAIN_LANE": "0", "PSK_CHAIN_WAVE_REG": "1"}, {"PSK_CHAIN_LANE": "0", "PSK_CHAIN_WAVE_REG": "0"},
                  {"PSK_CHAIN_SERIAL": "1"}, {"PSK_LANE_XTREES": "1"}):
        assert _run(125, dict(extra, PSK_GSI_SLICE="1"))[:2] == (n, d), extra


def test_packed_anchors_with_a_band_beyond_the_lane_window():
    """c = 30: a band of 83 anchors - the four-lanes-per-chunk deep kernel and its list, or the wave kernels."""
    n, d, lookups = _run(30, {"PSK_GSI_SLICE": "1"})
    assert lookups > 0 and n >= 3 * 3 + 6 * 6
    assert _run(30, {"PSK_GSI_SLICE": "0"})[:2] == (n, d)
    assert _run(30, {"PSK_GSI_SLICE": "1", "PSK_CHAIN_WAVE_REG": "1"})[:2] == (n, d)


def test_packed_anchor_edges_and_sampled_hits_match_the_oracle(oracle):
    """The batch does reach the edges: a chunk with an anchor exactly FRAGMENT_LENGTH after its head (q_rel = 20 000) in the self pairs of big0 and mid0
    (every query seed is an anchor there), a reference of more than 256 contigs; and 8 hits of the slice join - among them big_rc x big0 (reverse strand,
    r > 2^24), mid_six x mid0 and the 300-contig genome as query and as reference - recomputed by the oracle."""
    ns = {}
    exec(GENOMES, ns)
    genomes = dict(ns["genomes"])
    for name in ("big0", "mid0"):
        s = oracle.Sketch(genomes[name]).seeds
        pos = np.sort(s["pos"][s["contig"] == 0])
        at, head = 0, None
        for p in pos.tolist():
            if head is None or p > head + FRAGMENT_LENGTH:
                head = p
            elif p == head + FRAGMENT_LENGTH:
                at += 1
        assert at > 0, name
    assert oracle.Sketch(genomes["mid_300"]).contig_lens.size > 256
    import pyskani_amd as psk
    old = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("PSK_")}
    os.environ["PSK_GSI_SLICE"] = "1"
    try:
        db = psk.Database()
        db.sketch_many([(n, *g) for n, g in ns["genomes"]])
        res = dict(zip([n for n, _ in ns["genomes"]], db.query_many([(n, *g) for n, g in ns["genomes"]], learned_ani=False)))
    finally:
        os.environ.pop("PSK_GSI_SLICE", None)
        os.environ.update(old)
    pick = np.random.default_rng(5)
    names = [n for n, _ in ns["genomes"] if not n.startswith("big")]
    pairs = [("big_rc", "big0"), ("mid_six", "mid0"), ("mid0", "mid_300"), ("mid_300", "mid1")] + [(names[int(i)], None) for i in pick.choice(len(names), 4, replace=False)]
    for q, r in pairs:
        hits = res[q]
        h = [x for x in hits if x.reference_name == r][0] if r else hits[int(pick.integers(0, len(hits)))]
        want = oracle.chain(oracle.Sketch(genomes[h.reference_name]), oracle.Sketch(genomes[q]))
        for f in ("n_anchors", "n_chunks", "n_intervals", "covered_query", "covered_ref", "sum_chain_anchors", "sum_chunk_seeds"):
            assert int(h._raw[f]) == int(getattr(want, f)), (q, h.reference_name, f, int(h._raw[f]), int(getattr(want, f)))
        assert abs(h.identity - want.ani) < 1e-6 and abs(h.query_fraction - want.af_query) < 1e-6 and abs(h.reference_fraction - want.af_ref) < 1e-6
