"""The batches test_interval_cpu.py and test_gpu_interval.py hold the bootstrap intervals (csrc/interval.hip) to: tier_cases' batches whose pairs sit on both sides of
the interval tiers' capacities, and one small batch of its own for the shortest tables.

The kernel's capacities are the reduce's: one wave per pair up to 64 RW_PER = 512 chunk ROWS, one workgroup per pair up to RED_CAP = 4096 KEPT values, global
memory beyond. So
  ci_small  pairs of 1, 2 and 30 rows (a world of 40 contigs), and a reference that shares nothing with the query
  edges_a   more than 4096 pairs: the live list (the pairs without a chunk table are filled by the lane kernel); rows 1 .. 64 | 65 .. 512 | 513 .. 1025
  edges_b   at most 4096 pairs, no live list: the wave tier visits every pair; the same rows, among them 512 / 513 and the twin of 513 rows (more than 512 rows,
            fewer kept values: the workgroup tier by its rows)
  big       rows 4096 / 4097 and the twin of 4097 rows whose kept count is below 4096 (workgroup tier by its kept count) - the global tier takes rows_4097 alone"""
import numpy as np

import interval_ref as R
import tier_cases as T

CASES = ("ci_small", "edges_a", "edges_b", "big")
WAVE_ROWS, GROUP_VALUES = 64 * T.RW_PER, T.RED_CAP
_built = {}
_ref = {}


def cases(oracle):
    if not _built:
        w = T.World(oracle, 4303, 40, 1000, 2000)
        case = T.Case("ci_small")
        qi = case.qry("q40", w.query)
        for n in (1, 2, 30):
            g, ex = w.primary(n)
            case.pair(f"rows_{n}", qi, case.ref(f"rows_{n}", g), ex)
        case.ref("unrelated", [T._enc(T._rand(np.random.default_rng(5), 1500))])
        _built["ci_small"] = case
        for name in CASES[1:]:
            _built[name] = T.cases(oracle)[name]
    return _built


def tiers(ch):
    """which of the three tiers the host launches for the batch (csrc/interval.hip interval_launch), from the capacity rows"""
    rpm = max(ch.pair_rows)
    return (True, rpm > WAVE_ROWS, rpm > GROUP_VALUES)


def reference(oracle, case, pair, iterations=0, seed=0):
    """(lo, hi) of a pair of the case by interval_ref on the oracle's chunks; computed once"""
    key = (case.name, pair, iterations, seed)
    if key not in _ref:
        ch = T.chained(oracle, case)
        _ref[key] = R.interval(R.values_of(ch.chunks[pair]), iterations, seed) if pair in ch.chunks else (np.float32(-1), np.float32(-1))
    return _ref[key]
