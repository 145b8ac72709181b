"""GPU: the slice join's two walks (csrc/slice_join.hip gsl_walk_kernel: the slot table a wave builds per index block, the cursor that deals a seed's run out in
steps of 64 entries) on the database of tests/walk_cases.py: entries of 1, 63, 64, 65, 256 and 44 pairs, a family astride three index blocks whose queries have
two entries (passing references below rank_lo and at or above rank_hi in the walked block), runs of planted lengths around one and two steps, hundreds of seeds
without a run, a (seed, reference) group cut by a step boundary, a query shorter than a slice. One child process runs the database under the tagged index, the
untagged index and the per-pair join; the runs are made once and shared by the tests. Every comparison is equality."""
import numpy as np
import pytest

import walk_cases as W
from rerun_cases import INT_FIELDS

pytestmark = pytest.mark.gpu
_RUNS = {}


def run(config):
    if not _RUNS:
        _RUNS.update(W.run_walk_child(["slice_tagged", "slice_untagged", "pairs_tagged"]))
    return _RUNS[config]


@pytest.fixture(scope="module")
def sketches(oracle):
    cs = W.case()
    made = {}

    def sketch(kind, n):
        if (kind, n) not in made:
            made[(kind, n)] = oracle.Sketch(dict(cs["queries"] if kind == "q" else cs["refs"])[n], c=cs["c"], marker_c=cs["marker_c"], k=cs["k"])
        return made[(kind, n)]
    return sketch


def test_tagged_untagged_and_per_pair_join_return_the_same_bytes():
    tagged, untagged, pairs = run("slice_tagged"), run("slice_untagged"), run("pairs_tagged")
    assert tagged["record_bytes"] == 80 and tagged["n_records"] >= len(W.case()["queries"])      # every query finds a relative at least
    assert tagged["digest"] == untagged["digest"] == pairs["digest"]
    assert tagged["lookups"] > 0 and untagged["lookups"] > 0                                        # the slice join ran
    assert tagged["info"][2] == 1 and tagged["info"][1] == W.TAG_SHIFT and untagged["info"][2] == 0
    assert tagged["identity"] == untagged["identity"] == 1      # insertion order = locality order: the slots, blocks and local ids are the ones the case means


def test_count_walk_visits_the_sum_of_the_run_lengths(oracle, sketches):
    """psk_ctx_join_work's index_entries_visited of query qa alone on the untagged index, against the runs restated in numpy from the sketches"""
    cs = W.case()
    untagged = run("slice_untagged")
    shift = untagged["info"][1]
    assert untagged["qa_lookups"] > 0
    qa = sketches("q", "qa")
    refs = [sketches("r", n) for n, _ in cs["refs"]]
    passing = [s for s, r in enumerate(refs) if oracle.screen(qa, r)[0]]
    assert passing == list(range(W.BIG_SLOT0, W.BIG_SLOT0 + W.BIG))
    want = W.entries_visited(qa.seeds["kmer"], [r.seeds["kmer"] for r in refs], passing, shift)
    print("index_entries_visited", untagged["qa_visited"], "restated", want, "shift", shift)
    assert untagged["qa_visited"] == want


def test_sampled_hits_and_planted_pairs_carry_the_oracles_integers(oracle, sketches):
    cs = W.case()
    recs = {(r[0], r[1]): r[2:2 + len(INT_FIELDS)] for r in run("slice_tagged")["records"]}
    keys = sorted(recs)
    pick = np.random.default_rng(11)
    pairs = [keys[int(i)] for i in pick.choice(len(keys), 6, replace=False)] + [tuple(p) for p in cs["planted"]]
    for q, r in pairs:
        assert (q, r) in recs, (q, r)
        want = oracle.chain(sketches("r", r), sketches("q", q))
        assert recs[(q, r)] == [int(getattr(want, f)) for f in INT_FIELDS], (q, r)


def test_doubled_kmer_gives_two_anchors(sketches):
    """n_anchors of qc against the member that holds the planted k-mer twice: every (query seed, reference seed) match, the doubled k-mer's two among them"""
    cs = W.case()
    recs = {(r[0], r[1]): r[2:2 + len(INT_FIELDS)] for r in run("slice_tagged")["records"]}
    qk = sketches("q", "qc").seeds["kmer"]
    for ref, v in ((cs["doubled"], cs["c1"]), (cs["first"], cs["c2"])):
        u, n = np.unique(sketches("r", ref).seeds["kmer"], return_counts=True)
        held = dict(zip(u.tolist(), n.tolist()))
        assert held[v] == 2 and int((qk == v).sum()) == 1
        assert recs[("qc", ref)][INT_FIELDS.index("n_anchors")] == sum(held.get(int(x), 0) for x in qk)
