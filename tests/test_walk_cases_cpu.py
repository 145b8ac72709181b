"""CPU: every input of tests/walk_cases.py is what it claims, on the oracle and numpy alone."""
import numpy as np
import pytest

import walk_cases as W
from index_tag_cases import BSI_BLOCK, is_forward_seed


@pytest.fixture(scope="module")
def made(oracle):
    """the case, and the oracle's sketches of its references (by slot) and of the four built queries"""
    cs = W.case()
    sk = lambda g: oracle.Sketch(g, c=cs["c"], marker_c=cs["marker_c"], k=cs["k"])      # noqa: E731
    refs = [sk(g) for _, g in cs["refs"]]
    built = {n: sk(g) for n, g in cs["queries"][len(refs):]}
    return cs, refs, built


def holders(refs, v):
    """{slot: occurrences} of k-mer v among the references' seeds"""
    return {s: int((r.seeds["kmer"] == v).sum()) for s, r in enumerate(refs) if (r.seeds["kmer"] == v).any()}


def test_database_layout_families_slots_and_entries(oracle, made):
    cs, refs, built = made
    names = [n for n, _ in cs["refs"]]
    assert len(refs) == 532 and all(20000 <= len(g[0]) <= 30000 for _, g in cs["refs"])
    assert cs["queries"][:len(refs)] == cs["refs"] and [n for n, _ in cs["queries"][len(refs):]] == ["qa", "qb", "qc", "qd"]
    passing = lambda q: [s for s, r in enumerate(refs) if oracle.screen(q, r)[0]]      # noqa: E731
    for s in range(W.N_UNRELATED):
        assert passing(refs[s]) == [s]                                                   # P = 1: itself
    lo = W.N_UNRELATED
    for m in W.SMALL_FAMILIES:
        assert names[lo] == f"s{m}_0" and passing(refs[lo]) == passing(refs[lo + m - 1]) == list(range(lo, lo + m))      # entries of exactly 63, 64 and 65 pairs
        lo += m
    assert lo == W.BIG_SLOT0 == 232 and names[232] == "b0" and names[531] == "b299"
    big = list(range(232, 532))
    for q in [refs[232], refs[256], refs[511], refs[512], refs[531]] + list(built.values()):
        assert passing(q) == big
    # the two entries of a query of the 300: ranks 0..255 and 256..299, and where they lie in the index blocks
    first, second = big[:BSI_BLOCK], big[BSI_BLOCK:]
    assert [first[0] // BSI_BLOCK, first[0] % BSI_BLOCK, first[-1] // BSI_BLOCK, first[-1] % BSI_BLOCK] == [0, 232, 1, 231]
    assert [second[0] // BSI_BLOCK, second[0] % BSI_BLOCK, second[-1] // BSI_BLOCK, second[-1] % BSI_BLOCK] == [1, 232, 2, 19] and len(second) == 44
    in_b1 = [s % BSI_BLOCK for s in big if s // BSI_BLOCK == 1]
    assert in_b1 == list(range(256))                                                     # block 1: all 256 pass, local ids 0, 31, 32, 255 among them; slots 0 and 255 occur in the first entry
    assert sum(s // BSI_BLOCK == 0 for s in big) == 24 and sum(s // BSI_BLOCK == 2 for s in big) == 20


def test_planted_run_kmers_are_forward_seeds_held_by_exactly_the_stated_references(made):
    cs, refs, built = made
    b1 = BSI_BLOCK      # slot of block 1's local reference 0
    assert names_of(cs, b1) == cs["first"] == "b24"
    every = np.concatenate([r.seeds["kmer"] for r in refs]).astype(np.uint64)
    for n, v in cs["run_kmers"].items():
        assert is_forward_seed(np.array([v], np.uint64), cs["k"], cs["c"])[0]
        assert holders(refs, v) == {b1 + j: 1 for j in range(n)}, n                       # block 1's first n references, once each, and nowhere else
        for q in ("qa", "qb"):
            assert int((built[q].seeds["kmer"] == v).sum()) == 1
        # the tagged index (buckets of 256 k-mers): the k-mer's bucket holds nothing else in any block - its run has exactly n entries
        assert int(((every >> np.uint64(W.TAG_SHIFT)) == np.uint64(v >> W.TAG_SHIFT)).sum()) == n
    assert sorted(cs["run_kmers"]) == [1, 63, 64, 65, 128, 129, 256]


def names_of(cs, slot):
    return cs["refs"][slot][0]


def test_dup_kmers_are_held_twice_by_the_doubled_member(oracle, made):
    cs, refs, built = made
    b1 = BSI_BLOCK
    assert names_of(cs, b1 + 63) == cs["doubled"]
    want1 = {b1 + j: 1 for j in range(63)}; want1[b1 + 63] = 2                          # entries 63 and 64 of the run: cut by the step boundary
    want2 = {b1 + j: 1 for j in range(64)}; want2[b1] = 2                                # the doubled member first in the run
    every = np.concatenate([r.seeds["kmer"] for r in refs]).astype(np.uint64)
    for v, want in ((cs["c1"], want1), (cs["c2"], want2)):
        assert is_forward_seed(np.array([v], np.uint64), cs["k"], cs["c"])[0]
        assert holders(refs, v) == want
        assert int(((every >> np.uint64(W.TAG_SHIFT)) == np.uint64(v >> W.TAG_SHIFT)).sum()) == 65
        assert int((built["qc"].seeds["kmer"] == v).sum()) == 1
    pos = np.sort(refs[b1 + 63].seeds["pos"][refs[b1 + 63].seeds["kmer"] == cs["c1"]])
    assert int(pos[1] - pos[0]) == W.DUP_GAP
    # the pair's anchors are all (query seed, reference seed) matches: the doubled k-mer gives two
    for ref, v in ((b1 + 63, cs["c1"]), (b1, cs["c2"])):
        u, n = np.unique(refs[ref].seeds["kmer"], return_counts=True)
        held = dict(zip(u.tolist(), n.tolist()))
        assert held[v] == 2
        assert oracle.chain(refs[ref], built["qc"]).n_anchors == sum(held.get(int(x), 0) for x in built["qc"].seeds["kmer"])


def test_inserted_stretch_shares_no_kmer_and_leaves_batches_without_a_run(oracle, made):
    cs, refs, built = made
    ins = oracle.Sketch([cs["insert"]], c=cs["c"], marker_c=cs["marker_c"], k=cs["k"]).seeds["kmer"]
    every = np.concatenate([r.seeds["kmer"] for r in refs])
    assert len(ins) >= 192 and not np.isin(ins, every).any()                          # (3 kb at c = 10: ~300 seeds; 191 in a row are enough to hold two whole 64-seed batches wherever they start)
    qb = built["qb"].seeds
    assert (np.diff(qb["pos"].astype(np.int64)) > 0).all()                               # one contig: the seeds are in position order, the order the walk takes them in
    bare = ~np.isin(qb["kmer"], every)
    longest = max(len(r) for r in "".join("x" if b else " " for b in bare).split())
    assert longest >= len(ins)                                                           # the stretch's seeds, in a row, and none of them held by a reference
    # runs are per BUCKET: in block 2 (20 references) of the tagged index whole 64-seed batches of a 256-seed slice have none, and first or last lanes without a run stand beside lanes with one
    blk2 = np.concatenate([r.seeds["kmer"] for r in refs[2 * BSI_BLOCK:]])
    runs = W.run_lengths(qb["kmer"], blk2, W.TAG_SHIFT)
    batches = [runs[i:i + 64] for i in range(0, len(runs), 64)]
    assert any(len(b) == 64 and not b.any() for b in batches)
    assert any(b.any() and b[0] == 0 for b in batches) and any(len(b) == 64 and b.any() and b[63] == 0 for b in batches)


def test_short_query_is_less_than_one_slice(made):
    cs, refs, built = made
    n = len(built["qd"].seeds)
    assert 64 < n <= 200 and n % 64 != 0


def test_planted_pairs_are_pairs_of_the_case(made):
    cs, refs, built = made
    names = {n for n, _ in cs["refs"]}
    assert all(q in built and r in names for q, r in cs["planted"])
    assert {q for q, _ in cs["planted"]} == {"qa", "qb", "qc"}
