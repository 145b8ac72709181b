"""CPU: every edge input of tests/sq_edges.py lands exactly on its intended oracle count (seeds, raw markers, anchors of one pair,
chain roots of one chunk, candidate chains, chunks with an estimate, hits), so that the GPU edge tests
(tests/test_gpu_small_query_edges.py) keep testing the capacity they name. A change to a generator or to the oracle that moves an
input off its edge fails here, without a GPU."""
import pytest

import sq_edges as E

CASES = [(cid, case) for cid, case in E.edge_cases() if "edge" in case]


@pytest.mark.parametrize("cid,case", CASES, ids=[cid for cid, _ in CASES])
def test_edge_input_lands_on_its_oracle_count(oracle, cid, case):
    what, want = case["edge"]
    got = E.oracle_count(oracle, what, case)
    print(f"{cid}: {what} = {got}")
    assert got == want, (cid, what, got, want)


def test_over_cap_inputs_stay_inside_the_other_capacities(oracle):
    """an over-cap input must exceed ONLY its own capacity: the at-cap/over pair differs in one count"""
    for cid, case in CASES:
        what = case["edge"][0]
        if what in ("seeds", "markers"):
            continue
        assert E.oracle_count(oracle, "seeds", case) <= E.SQ_SEEDS and E.oracle_count(oracle, "markers", case) <= E.SQ_MARKERS, cid
        if what in ("anchors", "roots", "cands"):
            for other, cap in (("anchors", E.SQ_SEEDS), ("roots", E.SQ_TREES), ("cands", E.SQ_CANDS)):
                if other != what:
                    assert E.oracle_count(oracle, other, case) <= cap, (cid, other)
    for cid, case in CASES:
        if case["edge"][0] == "seeds":
            assert E.oracle_count(oracle, "markers", case) <= E.SQ_MARKERS, cid
        if case["edge"][0] == "markers":      # (a seed overflow would raise the same stats through SQ_F_SEEDS)
            assert E.oracle_count(oracle, "seeds", case) <= E.SQ_SEEDS, cid


def test_chain_root_inputs_have_the_chunk_rows_named(oracle):
    """1, 2 and 3 chunk rows: the DP by a team of four waves, a team of two, one wave per chunk"""
    cases = [(cid, case) for cid, case in CASES if "chunks" in case]
    assert sorted({case["chunks"] for _, case in cases}) == [1, 2, 3]
    for cid, case in cases:
        assert E.oracle_count(oracle, "rows", case) == case["chunks"], cid


def test_host_gated_inputs_are_shaped_as_named():
    """the inputs the host keeps off the fused path (or admits) by shape alone: kept contigs, contig length, tiles, references"""
    d = dict(E.edge_cases())
    kept = lambda case: [x for x in case["queries"][0][1] if len(x) >= E.MIN_LENGTH_CONTIG]
    tiles = lambda case: sum(-(-len(x) // E.TILE_BASES) for x in kept(case))
    assert len(kept(d["desc_63"])) == E.SQ_MAX_DESC - 1 and len(kept(d["desc_64"])) == E.SQ_MAX_DESC
    longest = lambda case: max(len(x) for x in kept(case))
    assert longest(d["contig_at_max_length"]) == E.SQ_MAX_TILES * E.TILE_BASES and longest(d["contig_over_max_length"]) == E.SQ_MAX_TILES * E.TILE_BASES + 1
    assert tiles(d["tiles_64"]) == E.SQ_MAX_TILES and tiles(d["tiles_65"]) == E.SQ_MAX_TILES + 1
    for cid in ("tiles_64", "tiles_65"):      # only the tile count is at stake: no other shape gate applies
        assert longest(d[cid]) < E.SQ_MAX_TILES * E.TILE_BASES and len(kept(d[cid])) < E.SQ_MAX_DESC, cid
        assert sum(len(x) // 20001 + 1 for x in kept(d[cid])) <= E.SQ_ROWS, cid
    assert sorted(len(x) for x in d["tiles_around_one"]["queries"][0][1]) == [E.TILE_BASES - 1, E.TILE_BASES, E.TILE_BASES + 1]
    assert sum(len(x) // 20001 + 1 for x in kept(d["rows_over"])) == E.SQ_ROWS + 1      # (and 65 tiles: the rows gate never decides alone, gen_rows_over)
    assert len(d["refs_at_cap"]["refs"]) == len(d["refs_at_cap_dup"]["refs"]) == E.SQ_MAX_REFS and len(d["refs_over"]["refs"]) == E.SQ_MAX_REFS + 1
    assert len({n for n, _ in d["refs_at_cap_dup"]["refs"]}) == E.SQ_MAX_REFS - 1
    assert [len(x) for x in d["min_length"]["queries"][0][1]][0] == 499
