"""No GPU: every case of tier_cases.py holds what it promises, by the oracle alone - the rows, candidate chains, kept chunks and kept chains of every named
pair, the rows that keep no chain where the twins want them, the screen, the host state each batch is built for (restated from the capacity rows), the
agreement of the numpy reduce (tier_cases.reduce_ref) with the oracle's ani / ani_std for the three flag sets, and that every named slip of a reduce
kernel would move a pair's result by at least twice the tolerance. A case that does not is a broken test: test_gpu_tiers.py would run the tiers past nothing."""
import numpy as np
import pytest

import tier_cases as T

CASES = ("edges_a", "edges_b", "edges_c", "edges_d", "big", "conflicts")


@pytest.fixture(scope="module")
def cases(oracle):
    return T.cases(oracle)


def _index(ch):
    return {p: i for i, p in enumerate(ch.pairs)}


def test_the_cases_are_these(cases):
    assert tuple(cases) == CASES
    assert max(sum(len(x) for x in g) for c in cases.values() for _, g in c.refs + c.queries) < 7_000_000      # the largest genome: about 6 Mb


@pytest.mark.parametrize("name", CASES)
def test_every_named_pair_passes_the_screen_and_has_its_rows_candidates_and_kept_chains(cases, oracle, name):
    case, ch = cases[name], T.chained(oracle, cases[name])
    at = _index(ch)
    for pn, pair in case.pairs.items():
        assert pair in at, (pn, "did not pass the screen")
        ex, res, i = case.expect[pn], ch.res[pair], at[pair]
        assert (ch.rows[i], ch.cands[i], res.n_chunks, res.n_intervals) == (ex["rows"], ex["cands"], ex["m"], ex["n_intervals"]), pn
        kept = ch.chunks[pair]["contig"].tolist()
        if "rows_without_chain" in ex:      # a twin: its rows are the query's contigs 0 .. nc - 1
            assert sorted(set(range(ex["rows"])) - set(kept)) == ex["rows_without_chain"], pn
        if name == "conflicts":             # the first copy of the best score / the long candidate is the one that stays
            assert kept == [0], pn


def test_row_edges_twins_and_the_trim_threshold(cases):
    edges = cases["edges_a"].expect
    assert {edges[f"rows_{n}"]["rows"] for n in (1, 4, 5, 64, 65, 512, 513, 1024, 1025)} == {1, 4, 5, 64, 65, 512, 513, 1024, 1025}
    assert {edges[f"rows_{n}"]["m"] for n in (9, 10, 11)} == {9, 10, 11}      # m // 10 turns non-zero
    big = cases["big"].expect
    assert (big["rows_4096"]["m"], big["rows_4097"]["m"]) == (T.RED_CAP, T.RED_CAP + 1)
    assert big["rows_4097t"]["rows"] > T.RED_CAP >= big["rows_4097t"]["m"]
    for ex in [edges["rows_65t"], edges["rows_513t"], edges["rows_1025t"], big["rows_4097t"]]:
        nc, none = ex["rows"], ex["rows_without_chain"]
        assert ex["m"] == nc - len(none) <= nc - 5
        assert {0, nc - 1, 63, 64} <= set(none) and (nc < 257 or {255, 256} <= set(none))
        assert nc - ex["cands"] >= 2 and ex["cands"] - ex["m"] >= 2      # both kinds: rows without a candidate, candidates that lose
    for c in "abc":
        assert cases[f"edges_{c}"].expect.keys() >= edges.keys() - {"tiny_4r8c", "tiny_4r9c", "tiny_5r5c", "tiny_1r9c"}
    assert {(e["rows"], e["cands"]) for n, e in edges.items() if n.startswith("tiny_")} == {(4, 8), (4, 9), (5, 5), (1, 9)}
    assert all(e["n_intervals"] == e["cands"] - 1 for n, e in edges.items() if n.startswith("tiny_"))      # one conflict on the reference inside each
    assert {e["cands"] for e in edges.values()} >= {T.CSMALL, T.CSMALL + 1, T.CMAX, T.CMAX + 1}
    conf = cases["conflicts"].expect      # every candidate but the kept one overlaps it: all of them are conflicted
    assert (conf["conflicted_128"]["cands"], conf["conflicted_129"]["cands"], conf["conflicted_128"]["n_intervals"], conf["conflicted_129"]["n_intervals"]) == (128, 129, 1, 1)
    assert conf["carry_70"]["cands"] - 1 >= 65 and conf["carry_70"]["n_intervals"] == 1
    q = cases["conflicts"].queries[cases["conflicts"].pairs["conflicted_128"][0]][1]
    assert q[0] == q[1] and q[3] == q[5] and len(set(q)) == len(q) - 2      # two pairs of byte-identical copies


@pytest.mark.parametrize("name", CASES)
def test_the_batch_is_in_the_host_state_it_was_built_for(cases, oracle, name):
    case, ch = cases[name], T.chained(oracle, cases[name])
    assert [T.capacity_rows(case.queries[qi][1]) for qi, _ in ch.pairs] == ch.pair_rows
    reg = T.regime(ch.pair_rows)
    want = T.expected_stats(reg, ch.rows, ch.cands)
    launched = {k for k in T.STATS[:7] if reg[k]}
    if case.regime == "a":
        assert reg["n_pairs"] > T.LIVE_PAIRS and reg["average"] < 16
        assert launched == set(T.STATS[:7])
        assert want["live"] < reg["n_pairs"] and any(r == 0 for r in ch.rows)      # pairs without a single anchor: pair_empty_kernel has work
        assert 0 < want["rest"] < want["live"] and want["mid"] == 4 and want["big"] == 1
    elif case.regime == "b":
        assert reg["n_pairs"] <= T.LIVE_PAIRS and 16 <= reg["average"] <= 512 and reg["rows_pair_max"] > 64
        assert launched == {"reduce_small", "reduce_wave", "reduce_group", "reduce_large"} and any(r == 0 for r in ch.rows)
    elif case.regime == "c":
        assert reg["average"] > 512 and launched == {"reduce_group", "reduce_large"}
    elif case.regime == "d":
        assert reg["rows_pair_max"] <= 64 and reg["average"] < 16 and launched == {"reduce_tiny", "reduce_small"}
    elif name == "big":
        assert launched == {"reduce_group", "reduce_large"} and want["big"] == 3
    if name == "edges_a":      # the tiny selection's edges: taken by the lane kernel / left to the wave kernel
        at = _index(ch)
        left = {pn: ch.rows[at[p]] > T.TINY_ROWS or ch.cands[at[p]] > T.TINY_CANDS for pn, p in case.pairs.items()}
        assert (left["tiny_4r8c"], left["tiny_4r9c"], left["tiny_5r5c"], left["tiny_1r9c"], left["rows_4"], left["rows_5"]) == (False, True, True, True, False, True)


@pytest.mark.parametrize("flags", T.FLAGS, ids=["mean", "median", "robust"])
@pytest.mark.parametrize("name", CASES)
def test_the_numpy_reduce_agrees_with_the_oracle(cases, oracle, name, flags):
    ch = T.chained(oracle, cases[name], flags)
    assert ch.chunks
    for pair, chunks in ch.chunks.items():
        res = ch.res[pair]
        ani, std = T.reduce_ref(chunks, T.K, **flags)
        assert len(chunks) == res.n_chunks
        assert abs(std - res.ani_std) < T.TOL, pair
        if res.af_query >= 0.15 or res.af_ref >= 0.15:      # (below min_af the pair carries no ANI)
            assert abs(ani - res.ani) < T.TOL, pair
        else:
            assert res.ani == -1.0, pair


@pytest.mark.parametrize("name", CASES)
def test_every_named_slip_moves_the_result_by_twice_the_tolerance(cases, oracle, name):
    case, ch = cases[name], T.chained(oracle, cases[name])
    seen = set()
    for pn, pair in case.pairs.items():
        if case.expect[pn]["m"] < 3:
            continue
        margins = T.slip_margins(ch.chunks[pair])
        assert margins and min(margins.values()) >= 2 * T.TOL, (pn, margins)
        if case.expect[pn]["m"] >= 20:
            assert len(margins) == (7 if case.expect[pn]["m"] <= 1025 else 6), (pn, margins)
        seen |= set(margins)
    assert name == "conflicts" or {"median_index_minus_1", "median_index_plus_1", "trim_lo_plus_1", "trim_hi_minus_1"} <= seen
