"""CPU: every input of tests/index_tag_cases.py is what it claims, on the oracle alone."""
import numpy as np
import pytest

import index_tag_cases as T


def _sketch(O, cs, contigs):
    return O.Sketch(contigs, c=cs["c"], marker_c=cs["marker_c"], k=cs["k"])


def test_block_edge_puts_a_family_astride_two_index_blocks(oracle):
    cs = T.case("block_edge")
    refs = cs["refs"]
    assert len(refs) == 320 and all(20000 <= len(g[0]) <= 30000 for _, g in refs)
    # families are contiguous in insertion order (the locality order keeps such an order), and slots 255 | 256 belong to one family
    fam = [n.split("_")[0] for n, _ in refs]
    assert fam == sorted(fam) and fam[T.BSI_BLOCK - 1] == fam[T.BSI_BLOCK] == "f3" and fam.index("f3") == 240
    last, first = _sketch(oracle, cs, refs[T.BSI_BLOCK - 1][1]), _sketch(oracle, cs, refs[T.BSI_BLOCK][1])      # local ids 255 and 0
    assert len(cs["top_tags"]) == 4 and all(x & 0xFF == 0xFF for x in cs["top_tags"])
    for s in (last, first):
        tags = set((s.seeds["kmer"] & 0xFF).tolist())
        assert 0xFF in tags and 0x00 in tags
        assert set(cs["top_tags"]) <= set(s.seeds["kmer"].tolist())      # the planted k-mers: shared, so they are anchors of the pair
    assert oracle.screen(last, first)[0] and oracle.screen(first, last)[0]
    assert oracle.chain(first, last).n_anchors > 100 and oracle.chain(last, first).n_anchors > 100
    # another family does not pass the screen: the walk of a query of f3 meets entries of f2 in block 0 only by chance
    assert not oracle.screen(last, _sketch(oracle, cs, refs[200][1]))[0]


def test_bucket_neighbours_are_seeds_of_the_planted_reference_and_change_no_anchor_count(oracle):
    cs = T.case("neighbours")
    k, c = cs["k"], cs["c"]
    q = _sketch(oracle, cs, cs["queries"][0][1])
    qk = np.unique(q.seeds["kmer"].astype(np.uint64))
    assert np.array_equal(qk, np.unique(np.array(cs["query_seeds"], np.uint64)))      # the module's k-mer arithmetic is the oracle's
    refs = dict(cs["refs"])
    planted, plain = _sketch(oracle, cs, refs["planted"]), _sketch(oracle, cs, refs["plain"])
    pk = set(planted.seeds["kmer"].tolist())
    shift_forgotten = 9      # a forced index that kept the contract job's 21 bits
    for kind in T.NEIGHBOUR_KINDS:
        v = np.array(cs["plants"][kind], np.uint64)
        assert len(v) >= T.NEIGHBOUR_MIN and len(set(v.tolist())) == len(v)
        assert all(int(x) in pk for x in v), kind                 # every plant is a seed of the reference, under the planted value
        assert not np.isin(v, qk).any()                           # ... and no seed of the query
        near = [qk[(qk ^ x) < (1 << 8)] for x in v]              # the query seeds each shares its bits above 8 with
        if kind == "low":
            assert all(len(s) and ((s & 0xFF) != (x & 0xFF)).all() for s, x in zip(near, v))      # the seed's bucket, another tag
        if kind == "mid":
            same = [qk[((qk ^ x) >> np.uint64(shift_forgotten + 6)) == 0] for x in v]             # (bits 15 and above agree)
            assert all(((s & 0xFF) == (x & 0xFF)).any() and ((s ^ x) & 0x7F00).any() for s, x in zip(same, v))
            assert all(len(s) == 0 for s in near)
        if kind == "high":
            tags = set((qk & 0xFF).tolist())
            assert all(int(x) & 0xFF in tags for x in v) and all(len(s) == 0 for s in near)       # a query seed's tag, in another bucket
    a, b = oracle.chain(planted, q), oracle.chain(plain, q)
    assert a.n_anchors == b.n_anchors > 1000


@pytest.mark.parametrize("name", ["k14", "k16"])
def test_other_k_all_vs_all(oracle, name):
    cs = T.case(name)
    assert len(cs["refs"]) == 12 and all(len(g[0]) == 100000 for _, g in cs["refs"]) and cs["k"] == int(name[1:])
    sk = [_sketch(oracle, cs, g) for _, g in cs["refs"]]
    assert all(int(s.seeds["kmer"].max()) < (1 << (2 * cs["k"])) for s in sk)
    if cs["k"] == 16:
        assert any(int(s.seeds["kmer"].max()) >= (1 << 30) for s in sk)      # 32-bit k-mers do occur
    for f in range(3):
        assert oracle.screen(sk[4 * f], sk[4 * f + 3])[0] and oracle.chain(sk[4 * f + 3], sk[4 * f]).n_anchors > 100
    assert not oracle.screen(sk[0], sk[4])[0]
