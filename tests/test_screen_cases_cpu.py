"""CPU: tests/screen_ref.py is the oracle's screen rule (on sketches of real sequences), and tests/screen_cases.py holds what its docstrings claim - the sizes, the
pairs astride the threshold, the seams, the buckets, the shares. tests/test_gpu_screen.py relies on both."""
import math

import numpy as np
import pytest

import screen_cases as S
import screen_ref as R
from conftest import random_genome


def substitute(rng, seq, rate):
    """every position with probability `rate` becomes ANOTHER base (conftest.mutate redraws it, so a quarter of its hits change nothing)"""
    codes = np.frombuffer(seq.translate(bytes.maketrans(b"ACGT", bytes(range(4)))), np.uint8)
    hit = rng.random(len(codes)) < rate
    return np.frombuffer(b"ACGT", np.uint8)[np.where(hit, (codes + rng.integers(1, 4, len(codes))) & 3, codes)].tobytes()


def table_of(ref_sets):
    """the inverted index of build_inverted (csrc/screen.hip), restated: sorted keys, bits, shift, the bucket of every entry"""
    keys = np.sort(np.concatenate(list(ref_sets) + [np.zeros(0, np.uint64)]))
    bits = R.inverted_bits(len(keys))
    shift = R.MARKER_BITS - bits
    return keys, bits, shift, (keys >> np.uint64(shift)).astype(np.int64)


def check_sets(sets):
    for s in sets:
        assert s.dtype == np.uint64 and s.ndim == 1
        assert (np.diff(s.astype(np.int64)) > 0).all() and (len(s) == 0 or int(s[-1]) < 1 << 42)


def test_screen_ref_is_the_oracles_rule_on_real_sketches(oracle, ecoli):
    rng = np.random.default_rng(201)
    base = random_genome(rng, 400_000)
    genomes = [[seq] for seq in ecoli] + [[substitute(rng, base, d)] for d in (0.0, 0.02, 0.04, 0.06, 0.08, 0.10, 0.12, 0.12)] + [[random_genome(rng, 6000)]]
    sk = [oracle.Sketch(g) for g in genomes]
    markers = [s.markers for s in sk]
    check_sets(markers)
    assert 0 < len(markers[-1]) < R.SMALL_MARKER_COUNT
    family = range(2, 10)
    for rescue in (False, True):
        for screen_val in (0.80, 0.90, 0.95):
            want = np.array([[oracle.screen(q, r, screen_val, rescue) for r in sk] for q in sk])      # [q][r] = (pass, shared)
            got_counts = R.count_matrix(markers, markers)
            for qi, q in enumerate(markers):
                for ri, r in enumerate(markers):
                    assert R.shared(q, r) == want[qi, ri, 1] == got_counts[qi, ri], (qi, ri)
                    assert R.passes(R.shared(q, r), len(q), len(r), screen_val, rescue) == bool(want[qi, ri, 0]), (qi, ri, screen_val, rescue)
            assert np.array_equal(R.pass_matrix(markers, markers, screen_val, rescue), want[:, :, 0].astype(bool))
            if screen_val == 0.80 and not rescue:
                fam = want[np.ix_(family, family)][:, :, 0]
                assert fam.any() and not fam.all()      # the far pairs of the family lie on both sides
    assert want[-1, :, 0].all() and want[:, -1, 0].all()      # (rescue on: the short contig passes everywhere)


@pytest.mark.parametrize("name", S.SMALL_CASES)
def test_pass_matrix_equals_the_pair_by_pair_loop(name):
    refs, queries, screen_val, rescue, _ = S.case(name)
    check_sets(refs)
    check_sets(queries)
    assert np.array_equal(R.pass_matrix(refs, queries, screen_val, rescue), R.pass_matrix_naive(refs, queries, screen_val, rescue))
    assert np.array_equal(R.pass_matrix(refs, queries, screen_val, rescue, rows=7), R.pass_matrix(refs, queries, screen_val, rescue))
    counts = R.count_matrix(refs, queries)
    assert all(counts[qi, ri] == R.shared(q, r) for qi, q in enumerate(queries) for ri, r in enumerate(refs))


def test_first_passing_is_the_rules_own_edge():
    for screen_val in (0.80, S.HALF, 0.95, 1.0):
        for small in list(S.SIZES[1:]) + [8, 9, 65536, 65537]:
            s = R.first_passing(small, screen_val)
            assert R.passes(s, small, small + 3, screen_val, False) and (s == 0 or not R.passes(s - 1, small + 3, small, screen_val, False))
    assert R.first_passing(0, 0.80) is None
    assert R.first_passing(20, 1.0) == 21 and R.first_passing(100, 0.80) == 1 and R.first_passing(1025, 0.80) == 10
    assert math.pow(1.0, 21.0) == 1.0


@pytest.mark.parametrize("sv", ["080", "half"])
def test_grid_every_pair_sits_astride_the_threshold(sv):
    refs, queries, screen_val, _, _ = S.case(f"grid-{sv}-plain")
    assert S.case(f"grid-{sv}-rescue")[0] is not refs and all(np.array_equal(a, b) for a, b in zip(S.case(f"grid-{sv}-rescue")[0], refs))      # rescue changes no set
    r_sizes, q_sizes = [len(r) for r in refs], [len(q) for q in queries]
    assert set(r_sizes) == set(S.SIZES) == set(q_sizes) and len(refs) == 42 and len(queries) == 43
    assert q_sizes[0] == 0 and q_sizes[-1] == 0 and q_sizes[21] == 0 and all(q_sizes[i] for i in (1, 20, 22, 41))
    assert any(r_sizes[i] == 0 and r_sizes[i - 1] and r_sizes[i + 1] for i in range(1, 41)) and r_sizes[0] and r_sizes[-1]
    counts = R.count_matrix(refs, queries)
    at, below = 0, 0
    for qi, nq in enumerate(q_sizes):
        for ri, nr in enumerate(r_sizes):
            small = min(nq, nr)
            if small == 0:
                assert counts[qi, ri] == 0
                continue
            edge = R.first_passing(small, screen_val)
            assert counts[qi, ri] in (edge, edge - 1), (qi, ri)
            at += counts[qi, ri] == edge
            below += counts[qi, ri] == edge - 1
    assert at + below == 40 * 40 and min(at, below) >= 0.2 * (at + below), (at, below)
    # ... and those that rescue leaves alone (small >= 20) still hold both kinds
    big = np.minimum.outer(np.array(q_sizes), np.array(r_sizes)) >= R.SMALL_MARKER_COUNT
    want = R.pass_matrix(refs, queries, screen_val, False)
    assert want[big].any() and not want[big].all()


def test_grid_rows_at_screen_val_one():
    refs, queries, screen_val, _, _ = S.case("grid-one-plain")
    assert screen_val == 1.0 and [len(r) for r in refs] == [19, 20, 64, 300] and all(np.array_equal(q, r) for q, r in zip(queries, refs))
    assert not R.pass_matrix(refs, queries, 1.0, False).any()      # identical sets: 1.0 > 1.0 is false
    with_rescue = R.pass_matrix(refs, queries, 1.0, True)
    assert with_rescue[0, 0] and not with_rescue[1, 1] and not with_rescue[2, 2] and with_rescue[4, 3] and not with_rescue[5, 3]


@pytest.mark.parametrize("kind", ["main", "tiny"])
def test_values_sit_where_the_bucket_table_turns(kind):
    refs, queries, screen_val, rescue, _ = S.values(kind)
    keys, bits, shift, bucket = table_of(refs)
    nb, width = 1 << bits, 1 << shift
    assert (bits == 4 and len(keys) < 256) if kind == "tiny" else (bits > 4 and len(keys) >= 300)
    assert not rescue and 0.499 < math.pow(screen_val, 21.0) < 0.501
    held = set(int(k) for k in keys)
    assert {0, 1, S.TOP} <= held
    occupied = np.unique(bucket)
    assert occupied[0] == 0 and occupied[-1] == nb - 1 and (np.diff(occupied) >= (3 if kind == "tiny" else 4)).sum() >= 2      # first, last, and runs of empty buckets between
    crossings = [x for x in range(1, nb) if x * width - 1 in held and x * width in held]
    assert len(crossings) >= (2 if kind == "tiny" else 6) and nb - 1 in crossings and 1 in crossings
    full = int(np.bincount(bucket).argmax())
    inside = keys[bucket == full]
    one_ref = [r for r in refs if len(r) and (r >> np.uint64(shift) == full).all()]
    assert len(one_ref) == 1 and len(np.unique(one_ref[0])) >= (100 if kind == "tiny" else 300) and len(inside) > 64
    singles = [int(q[0]) for q in queries if len(q) == 1]
    in_full = [m for m in singles if m >> shift == full]
    ranks = [int(np.searchsorted(inside, np.uint64(m))) for m in in_full if m in held]
    assert any(r < 64 for r in ranks) and any(r >= 64 for r in ranks) and any(m not in held for m in in_full)
    assert any(m >> shift not in set(occupied.tolist()) for m in singles)      # query markers in empty buckets
    assert {0, S.TOP} <= set(singles)
    assert any(len(r) == 0 for r in refs) and len(queries[0]) == 0 and len(queries[-1]) == 0 and any(len(q) == 0 for q in queries[1:-1])
    want = R.pass_matrix(refs, queries, screen_val, rescue)
    for qi, q in enumerate(queries):      # a one-marker query's row is the marker's membership
        if len(q) == 1:
            assert [bool(x) for x in want[qi]] == [bool(np.isin(q[0], r)) for r in refs]
    assert {len(q) for q in queries} >= {0, 1, 3}


def test_values_all_references_empty():
    for kind, all_pass in (("empty", False), ("empty_rescue", True)):
        refs, queries, screen_val, rescue, _ = S.values(kind)
        assert all(len(r) == 0 for r in refs) and rescue == all_pass and {len(q) for q in queries} == {0, 1, 33}
        assert (R.pass_matrix(refs, queries, screen_val, rescue) == all_pass).all()


def test_multiplicity_runs_and_shares():
    refs, queries, screen_val, rescue, _ = S.multiplicity()
    assert len(refs) == 200 and min(len(r) for r in refs) >= 20 and not rescue
    keys, bits, shift, bucket = table_of(refs)
    marks, holders = np.unique(keys, return_counts=True)
    asked = np.unique(np.concatenate(queries))
    asked_holders = holders[np.isin(marks, asked)]
    assert set(asked_holders.tolist()) == set(S.MULTIPLICITIES)      # exactly these run lengths among the markers the queries ask for
    assert (np.bincount(bucket) > 64).any()                            # ... and a bucket the wave kernel's first 64 lanes do not cover
    counts = R.count_matrix(refs, queries)
    q_sizes, r_sizes = np.array([len(q) for q in queries]), np.array([len(r) for r in refs])
    small = np.minimum.outer(q_sizes, r_sizes)
    edge = np.vectorize(lambda s: R.first_passing(int(s), screen_val))(small)
    astride = (counts == edge) | (counts == edge - 1)
    assert astride.mean() >= 0.25, astride.mean()
    assert astride[:21].all()                                          # the 21 window queries: every cell
    assert len({tuple(row) for row in counts.tolist()}) == len(queries)      # the rows differ, and within a row the references do
    assert all(len(set(row)) >= 2 for row in counts[:21].tolist())
    want = R.pass_matrix(refs, queries, screen_val, rescue)
    for i in range(21):                                                # a window query's row is its window
        k, start = S.MULTIPLICITIES[i // 3], (0, 37, 150)[i % 3]
        assert np.array_equal(want[i], (np.arange(200) - start) % 200 < k)


def test_sliced_seams():
    refs, queries, screen_val, rescue, _ = S.sliced()
    check_sets(refs)
    check_sets(queries)
    assert [len(r) for r in refs] == [70000, 25, 0] and [len(q) for q in queries] == [65537, 10, 65537, 0, 65536, 65536] and not rescue
    assert [i for i, q in enumerate(queries) if len(q) > 4 * S.SLICE] == list(S.SLICED_LARGE_QUERIES)
    assert (65537 + S.SLICE - 1) // S.SLICE == 5 and 65537 - 4 * S.SLICE == 1 and 65537 // S.SLICE == 4
    seams = [16383, 16384, 32767, 32768, 49151, 49152, 65535]
    at = lambda q: np.flatnonzero(np.isin(q, refs[0])).tolist()
    assert at(queries[0]) == seams + [65536] and at(queries[2]) == seams and at(queries[4]) == [0] + seams and at(queries[5]) == seams
    assert R.first_passing(65537, screen_val) == 8 == R.first_passing(65536, screen_val)
    want = R.pass_matrix(refs, queries, screen_val, rescue)
    assert want.astype(int).tolist() == [[1, 0, 0], [1, 0, 0], [0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 0, 0]]
    assert np.array_equal(want, R.pass_matrix_naive(refs, queries, screen_val, rescue))


def test_wide_shape_and_shares():
    refs, queries, screen_val, rescue, _, extra = S.wide()
    n = len(refs)
    assert n == S.INV_LDS_REFS == 36864 and len(queries) == 1900 and screen_val == 0.80 and rescue
    assert (1 << 26) // n == 1820 < 1900 and (1 << 24) // n == 455 and (1 << 26) // (n + 1) < 1900 and n * 1900 >= 1 << 18
    sizes = np.array([len(r) for r in refs])
    assert sizes.min() >= 20 and sizes.max() <= 24 and 20 <= len(extra) <= 24
    check_sets(refs[::97] + [extra])
    check_sets(queries)
    keys, bits, shift, bucket = table_of(refs)
    assert int(keys[-1]) < 1 << 42 and bits == 16
    marks, holders = np.unique(keys, return_counts=True)
    assert (holders > 64).sum() > 1000 and (np.bincount(bucket) > 64).sum() > 1000      # real multiplicities, real buckets
    plain = R.pass_matrix(refs, queries, screen_val, False)
    assert plain.mean() >= 0.01 and (~plain).mean() >= 0.01
    q_sizes = np.array([len(q) for q in queries])
    assert (q_sizes == 0).sum() == 3 and ((q_sizes > 0) & (q_sizes < 20)).sum() >= 10
    for row in (454, 455, 1819, 1820):      # the rows either side of a sub-launch's end are ordinary queries, and no two alike
        assert q_sizes[row] >= 20 and plain[row].any() and not plain[row].all()
    assert not np.array_equal(plain[454], plain[455]) and not np.array_equal(plain[1819], plain[1820]) and not np.array_equal(plain[0], plain[1820])
    with_extra = R.pass_matrix(refs + [extra], queries[:200], screen_val, False)
    assert with_extra[:, -1].any() and not with_extra[:, -1].all() and np.array_equal(with_extra[:, :-1], plain[:200])
