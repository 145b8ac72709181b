"""No GPU: the bootstrap interval's rule (include/pyskani_amd.h, psk_ci_opts) as tests/interval_ref.py restates it - its hash against the oracle's, the library's
host-side draw and ranks (the inline functions the kernels use) against it, the figures of the E. coli pair, and the condition that keeps test_gpu_interval.py from
comparing nothing: on its batches every pair of 8 or more values has lo < hi, and another seed moves a bound."""
import ctypes as C

import numpy as np
import pytest

import interval_cases as IC
import interval_ref as R
import tier_cases as T

EDGE_KEYS = [0, 1, 2, 0xFFFFFFFF, 0x100000000, 0x7FFFFFFFFFFFFFFF, 0x8000000000000000, 0xFFFFFFFFFFFFFFFE, 0xFFFFFFFFFFFFFFFF]
SIZES = (1, 2, 3, 64, 65, 512, 513, 4096, 4097, 2 ** 32 - 1)


@pytest.fixture(scope="module")
def lib():
    from pyskani_amd import _capi
    return _capi.load()


def test_the_numpy_hash_is_the_oracles(oracle):
    rng = np.random.default_rng(11)
    keys = np.concatenate([np.array(EDGE_KEYS, dtype=np.uint64), rng.integers(0, 2 ** 64, 2000, dtype=np.uint64)])
    want = np.array([oracle.lib().orc_mm_hash64(int(k)) for k in keys], dtype=np.uint64)
    assert np.array_equal(R.mm_hash64(keys), want)


def test_the_librarys_draw_is_the_references(lib):
    rng = np.random.default_rng(12)
    seeds = [0, 7, 2 ** 64 - 1, 2 ** 63] + [int(x) for x in rng.integers(0, 2 ** 64, 3, dtype=np.uint64)]
    for m in SIZES:
        js = sorted({0, 1, 2, 3, m - 1, m // 2, min(m - 1, 1_000_001), min(m - 1, 2 ** 32 - 2)})
        for seed in seeds:
            for b in (0, 1, 63, 64, 99, 1023):
                for j in js:
                    got = lib.psk_ci_draw(seed, b, j, m)
                    assert got == R.draw(seed, b, j, m), (seed, b, j, m)
                    assert got < m


def test_the_matrix_of_draws_is_the_scalar_draw():
    for seed, B, m in ((0, 100, 225), (7, 20, 65), (2 ** 64 - 3, 33, 1)):
        d = R.draws(seed, B, m)
        assert d.shape == (B, m) and d.min() >= 0 and d.max() < m
        for b in (0, B // 2, B - 1):
            assert d[b].tolist() == [R.draw(seed, b, j, m) for j in range(m)]


def test_the_ranks(lib):
    for it, want in ((0, (100, 5, 94)), (100, (100, 5, 94)), (20, (20, 1, 18)), (1024, (1024, 51, 972))):
        n, lo, hi = C.c_uint32(), C.c_uint32(), C.c_uint32()
        lib.psk_ci_ranks(it, C.byref(n), C.byref(lo), C.byref(hi))
        assert (n.value, lo.value, hi.value) == want == R.ranks(it)
    lib.psk_ci_ranks(0, None, None, None)      # (NULL pointers are skipped)


def test_null_arguments_are_refused_without_a_device(lib):
    from pyskani_amd import _capi
    assert lib.psk_chain_ci(None, None, 0, None, None, None, None, None, None) == _capi.PSK_EINVAL
    assert lib.psk_query_many_ci(None, None, 0, None, 0, None, None, None, None) == _capi.PSK_EINVAL
    assert lib.psk_ctx_interval_stats(None, None, None, None, 0) == _capi.PSK_EINVAL
    assert b"NULL" in lib.psk_last_error()


def test_the_ecoli_pair(oracle, ecoli):
    """query EC590, reference K12, default parameters: 225 values, ANI 0.993815; the figures the rule was checked with before it was built"""
    ec590, k12 = ecoli
    res = oracle.chain(oracle.Sketch([k12]), oracle.Sketch([ec590]))
    v = R.values_of(oracle.last_chunks(), 15)
    assert len(v) == res.n_chunks == 225 and abs(res.ani - 0.993815) < 1e-6
    for seed, want in ((0, (0.992562, 0.995075)), (7, (0.992607, 0.995030))):
        lo, hi = R.interval(v, 100, seed)
        assert abs(float(lo) - want[0]) < 1e-6 and abs(float(hi) - want[1]) < 1e-6, (seed, lo, hi)
        assert R.interval(v, 0, seed) == (lo, hi)      # (0 stands for 100)
        assert lo < np.float32(res.ani) < hi


def test_one_value_is_its_own_interval():
    for x in (1.0, 0.97123456789, 0.5):
        for it in (0, 20, 1024):
            lo, hi = R.interval([x], it, 3)
            assert lo == hi == np.float32(x)
    assert R.interval([]) == (np.float32(-1), np.float32(-1))


def test_shifted_bounds_are_clamped():
    assert R.shifted(0.98, 0.99, 0.97, 0.985) == (np.float32(0.98) + (np.float32(0.97) - np.float32(0.985)), np.float32(0.99) + (np.float32(0.97) - np.float32(0.985)))
    assert R.shifted(0.98, 0.99, 1.0, 0.9)[1] == np.float32(1.0) and R.shifted(0.05, 0.99, 0.0, 0.9)[0] == np.float32(0.0)


@pytest.mark.parametrize("name", IC.CASES)
def test_the_gpu_batches_have_real_intervals(oracle, name):
    """what keeps the GPU comparisons from being vacuous: every pair with 8 or more values has lo < hi, and seed 7 moves a bound of some pair"""
    case = IC.cases(oracle)[name]
    ch = T.chained(oracle, case)
    named = set(case.pairs.values())
    assert named <= set(ch.chunks)
    moved, wide = 0, 0
    for pair, chunks in ch.chunks.items():
        m = len(chunks)
        lo, hi = IC.reference(oracle, case, pair)
        assert lo <= hi
        if m == 1:
            assert lo == hi == np.float32(R.values_of(chunks)[0])
        if m >= 8:
            assert lo < hi, (name, pair, m)
            wide += 1
            moved += IC.reference(oracle, case, pair, 0, 7) != (lo, hi)
    assert wide and moved, (name, wide, moved)
    tiers = IC.tiers(ch)
    assert tiers == {"ci_small": (True, False, False), "edges_a": (True, True, False), "edges_b": (True, True, False), "big": (True, True, True)}[name]
    rows = {pn: (case.expect[pn]["rows"], case.expect[pn]["m"]) for pn in case.pairs}
    if name == "ci_small":
        assert [rows[f"rows_{n}"] for n in (1, 2, 30)] == [(1, 1), (2, 2), (30, 30)]
        assert any(r == 0 for r in ch.rows)      # the unrelated reference: a pair without a chunk table
    if name in ("edges_a", "edges_b"):
        assert {rows[f"rows_{n}"][0] for n in (1, 64, 65, 512, 513)} == {1, 64, 65, 512, 513}
        assert rows["rows_513t"][0] > IC.WAVE_ROWS > rows["rows_513t"][1]
    if name == "big":
        assert rows["rows_4096"] == (4096, 4096) and rows["rows_4097"] == (4097, 4097)
        assert rows["rows_4097t"][0] > IC.GROUP_VALUES >= rows["rows_4097t"][1]
