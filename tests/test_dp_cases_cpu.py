"""No GPU: every case of dp_cases.py shows the event it was built for. The pairs' anchors are joined from the oracle's seeds in numpy and chained by a
pure-Python restatement of the rule (dp_cases.Chained); the oracle's own counts (chain roots per chunk, candidate chains) hold the restatement to it.
A case that does not show its event is a broken test: test_gpu_lane_dp.py would run the lane kernels past nothing."""
import numpy as np
import pytest

import dp_cases as D


@pytest.fixture(scope="module")
def chained(oracle):
    out = {}
    for name, ref, qry in D.cases(oracle):
        r, q = oracle.Sketch(ref), oracle.Sketch(qry)
        anchors = D.join(r.seeds, q.seeds)
        ch = D.Chained(anchors, D.BP_CHAIN_BAND // 125)
        res = oracle.chain(r, q)
        roots, ncand = oracle.last_chain_counts()
        assert res.n_anchors == len(anchors[1]), name
        assert roots.tolist() == ch.roots_per_chunk(), name
        assert ncand == ch.candidates(), name
        out[name] = (ch, anchors)
    return out


def test_the_batch_is_a_dozen_to_two_dozen_small_genomes(oracle):
    cs = D.cases(oracle)
    genomes = {tuple(ref) for _, ref, _ in cs} | {tuple(q) for _, _, q in cs}
    assert 12 <= len(genomes) <= 24
    assert all(100_000 <= sum(len(x) for x in g) <= 300_000 for g in genomes)


def test_tandem_repeat_best_predecessor_lies_beyond_the_near_evals(chained):
    ch, anchors = chained["tandem"]
    assert anchors[5].max() >= 4                                  # a query seed with four or more matches
    far = [x for x, d in enumerate(ch.pred_dist) if d > D.LANE_NEAR]
    assert far and any(ch.f[x] >= D.MIN_SCORE2 for x in far)       # ... and on a chain that counts


@pytest.mark.parametrize("n", [299, 300, 301])
def test_indel_at_the_gap_edge(chained, n):
    ch, _ = chained[f"indel_{n}"]
    gaps = {g for _, g in ch.accepted}
    if n <= D.MAX_GAP_LENGTH:
        assert n in gaps and n not in ch.refused_gap
    else:
        assert n in ch.refused_gap and max(gaps) <= D.MAX_GAP_LENGTH


@pytest.mark.parametrize("dq", [2499, 2500, 2501])
def test_neighbours_at_the_band_edge_chain_or_not(chained, dq):
    ch, _ = chained[f"reach_{dq}"]
    if dq <= D.BP_CHAIN_BAND:
        assert dq in {d for d, _ in ch.accepted}
    else:
        assert dq in ch.broke_dq and dq not in ch.reached_dq and max(d for d, _ in ch.accepted) < D.BP_CHAIN_BAND


@pytest.mark.parametrize("dq", [2499, 2500, 2501])
def test_chain_breaks_with_the_old_scores_still_in_the_window(chained, dq):
    ch, anchors = chained[f"break_{dq}"]
    qp = anchors[1]
    at = [(x, fy) for x, fy in ch.stale if qp[x] - qp[x - 1] == dq]
    assert at, "a root right behind a high-scoring anchor, that far from it"
    x = at[0][0]
    assert ch.f[x] == D.ANCHOR_SCORE2 and ch.f[x + 3] >= D.MIN_SCORE2      # the new chain starts below the old one's scores and qualifies on its own
    if dq <= D.BP_CHAIN_BAND:
        assert dq in ch.reached_dq and dq not in {d for d, _ in ch.accepted}      # within reach, refused for its gap
    else:
        assert dq in ch.broke_dq and dq not in ch.reached_dq


@pytest.mark.parametrize("n", [D.LANE_TREES, D.LANE_TREES + 1])
def test_chunk_with_that_many_qualifying_trees(chained, n):
    ch, _ = chained[f"trees_{n}"]
    counts = [len(set(ch.qualifying_roots(s, e))) for s, e in ch.chunks()]
    assert max(counts) == n and counts.count(n) == 1


def test_qualifying_anchors_alternate_between_two_trees(chained):
    ch, _ = chained["alternate"]
    back = 0
    for s, e in ch.chunks():
        seq = ch.qualifying_roots(s, e)
        back += sum(1 for i in range(2, len(seq)) if seq[i] == seq[i - 2] != seq[i - 1])
    assert back >= 10      # a root change back to a tree that holds a slot, many times over


def test_tiny_chunks_start_anywhere_in_the_anchor_array(chained):
    ch, _ = chained["tiny"]
    lens = {}
    for s, e in ch.chunks():
        lens.setdefault(e - s, []).append(s)
    for n in (1, 2, 3, 4):
        assert len(lens.get(n, [])) >= 3, (n, lens.keys())
    assert any(s % 16 for n in (1, 2, 3, 4) for s in lens[n])
    assert any(s % 16 and e - s > 16 for s, e in ch.chunks())       # ... and a long chunk that starts off a multiple of 16 (the lane kernel's aligned loads)
