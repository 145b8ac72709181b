"""CPU: every input of tests/rerun_cases.py is what it claims, on the oracle alone - the planted k-mer's count, the batch's anchor total against the
capacities the chain stage sizes its arrays for, the contig counts after the length filter. The capacities are restated in rerun_cases.py
(cap_general / cap_sparse / cap_slice / cap_onepass) from `anchor_cap_for` in pyskani_amd/csrc/chain.hip and the batch loops of
pyskani_amd/csrc/query_many.hip; the counter assertions of tests/test_gpu_reruns.py catch any drift between the two.

Out of scope: the wide format's other trigger, a reference contig number of 2^23 or more, needs a reference of at least 2^23 contigs of 500 bases (4.2 Gb)."""
import numpy as np
import pytest

import rerun_cases as RC

CASES = RC.cases()
FORMULAS = {"general": [RC.cap_general], "sparse": [RC.cap_sparse], "slice": [RC.cap_general, RC.cap_slice]}


def _word_kmer(oracle):
    base, word = RC._wide_base()
    s = oracle.Sketch([base], c=RC.CAP_C, marker_c=RC.CAP_MC).seeds
    at = s[s["pos"] == RC.WORD_POS]
    assert len(at) == 1 and base.count(word) == 1
    return int(at["kmer"][0])


def _counts(oracle, case, ref_name):
    s = oracle.Sketch(dict(case["refs"])[ref_name], c=case["c"], marker_c=case["marker_c"]).seeds
    kmers, n = np.unique(s["kmer"], return_counts=True)
    return dict(zip(kmers.tolist(), n.tolist()))


@pytest.fixture(scope="module")
def batches(oracle):
    memo = {}

    def get(case):
        key = (case["gen"][0].__name__, case["gen"][1])
        if key not in memo:
            memo[key] = RC.oracle_pairs(oracle, RC.materialise(case))
        return memo[key]
    return get


def test_the_case_list_covers_what_it_names():
    assert len(CASES) == len(RC.CAPACITY_ROUTES) + 1 + 2 * len(RC.WIDE_ROUTES) + 4 + 3 * len(RC.CONTIG_ROUTES) + len(RC.CONTIG_ROUTES)
    assert sum(c["reruns"][0] for c in CASES.values()) == len(RC.CAPACITY_ROUTES) + 1
    assert sum(c["reruns"][1] for c in CASES.values()) == len(RC.WIDE_ROUTES) + 1
    assert sum(c["reruns"][2] for c in CASES.values()) == 1 and sum(c["reruns"][3] for c in CASES.values()) == 0


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["kind"] in ("overflow", "control")])
def test_capacity_cases_overflow_with_room_to_spare_and_controls_fit(oracle, batches, name):
    case = CASES[name]
    pairs = batches(case)
    items, total = sum(p[2] for p in pairs), sum(p[3] for p in pairs)
    order = [(q, r) for q, r, _, _ in pairs]
    print(name, "pairs", len(pairs), "items", items, "anchors", total, [f(items) for f in FORMULAS[case["formula"]]])
    if case["kind"] == "control":
        assert all(total < f(items) for f in FORMULAS[case["formula"]])
        return
    for f in FORMULAS[case["formula"]]:
        assert total > f(items) + f(items) // 4, (total, f(items))      # a quarter above the capacity: no rounding of either side decides it
    assert total + total // 8 + 65536 < 0x7FFFFF00      # (chain_check's second capacity holds it)
    # honest pairs before and after the overflowing one, which holds more anchors than the whole capacity
    i = order.index(("rep", "tandem"))
    assert 0 < i < len(order) - 1 and pairs[i][3] > max(f(items) for f in FORMULAS[case["formula"]])
    assert all(p[3] <= p[2] + p[2] // 8 for j, p in enumerate(pairs) if j != i)
    cnt = _counts(oracle, RC.materialise(case), "tandem")
    kmer = _word_kmer(oracle)
    assert cnt[kmer] == case.get("copies", RC.TANDEM_COPIES)      # (the query's k-mers: once per copy)
    assert max(n for k, n in cnt.items() if k != kmer) < RC.WIDE_COUNT - 100      # no wide request unless the case plants one


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["kind"] == "wide"])
def test_wide_cases_plant_exactly_254_or_255_matches_of_one_query_seed(oracle, batches, name):
    case = RC.materialise(CASES[name])
    kmer = _word_kmer(oracle)
    cnt = _counts(oracle, case, "planted")
    assert cnt[kmer] == case["copies"]
    assert max(n for k, n in cnt.items() if k != kmer) < RC.WIDE_COUNT - 100
    for rn, _ in case["refs"]:
        if rn != "planted":
            assert max(_counts(oracle, case, rn).values()) < RC.WIDE_COUNT - 100
    q = oracle.Sketch(case["queries"][0][1], c=case["c"], marker_c=case["marker_c"]).seeds
    assert int((q["kmer"] == kmer).sum()) == 1      # the query holds it once
    pairs = batches(CASES[name])
    items, total = sum(p[2] for p in pairs), sum(p[3] for p in pairs)
    assert ("q", "planted") in [(a, b) for a, b, _, _ in pairs]
    assert total < min(RC.cap_general(items), RC.cap_sparse(items), RC.cap_slice(items)) // 2      # no capacity rerun beside it


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["kind"] == "onepass"])
def test_onepass_case_has_a_pair_that_outgrows_its_room_and_a_batch_that_fits(batches, name):
    pairs = batches(CASES[name])
    items, total = sum(p[2] for p in pairs), sum(p[3] for p in pairs)
    assert any(a > nq + nq // 8 + 8 for _, _, nq, a in pairs)      # gsi_room_kernel: a pair's room is its query seeds and an eighth
    assert any(a <= nq for _, _, nq, a in pairs)
    assert total < RC.cap_sparse(items) // 2 and total < RC.cap_onepass(items, len(pairs)) // 2


@pytest.mark.parametrize("n", [RC.CONTIG_LIMIT - 1, RC.CONTIG_LIMIT, RC.CONTIG_LIMIT + 1])
def test_contig_references_have_exactly_the_contigs_they_name(oracle, n):
    case = RC.materialise(CASES[f"contigs_{n}_contig_join"])
    contigs = dict(case["refs"])[f"contigs{n}"]
    assert min(map(len, contigs)) >= RC.MIN_LENGTH_CONTIG and max(map(len, contigs)) <= 520
    sk = oracle.Sketch(contigs, c=case["c"], marker_c=case["marker_c"])
    assert len(sk.contig_lens) == n == len(contigs)      # after the oracle's length filter
    top = int(sk.seeds["contig"].max())
    assert top == n - 1      # the highest contig number carries seeds
    # the queries reach the highest contig numbers: anchors against contigs 0, 32 766, 32 767 and (where present) 32 768
    names = [q for q, _ in case["queries"]]
    assert names == ["genome"] + [f"contig{i}" for i in (0, RC.CONTIG_LIMIT - 2, RC.CONTIG_LIMIT - 1, RC.CONTIG_LIMIT) if i < n]
    ref_kmers = {}
    for i in (0, RC.CONTIG_LIMIT - 2, RC.CONTIG_LIMIT - 1, RC.CONTIG_LIMIT):
        if i < n:
            ref_kmers[i] = set(sk.seeds["kmer"][sk.seeds["contig"] == i].tolist())
            q = oracle.Sketch(dict(case["queries"])[f"contig{i}"], c=case["c"], marker_c=case["marker_c"]).seeds
            assert len(set(q["kmer"].tolist()) & ref_kmers[i]) >= 10, i
    g = oracle.Sketch(dict(case["queries"])["genome"], c=case["c"], marker_c=case["marker_c"])
    assert len(g.contig_lens) == 200 and len(set(g.seeds["kmer"].tolist()) & ref_kmers[n - 1]) >= 10


def test_mixed_database_holds_one_reference_past_the_limit(oracle):
    case = RC.materialise(CASES["contigs_mixed_contig_join"])
    n = [len(oracle.Sketch(contigs, c=case["c"], marker_c=case["marker_c"]).contig_lens) for _, contigs in case["refs"]]
    assert n == [1, RC.CONTIG_LIMIT + 1, 1, 40]
