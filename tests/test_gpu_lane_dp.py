"""GPU: the lane-per-chunk chaining DP (csrc/dp.hip chain_lane_body) on the cases of dp_cases.py - each built for one decision of the kernel: the far part
of the band and its bound, the gap and band-in-bases edges, a chain that breaks with its scores still in the window, four and five qualifying trees per
chunk, trees that alternate, chunks of one to four anchors anywhere in the anchor array (test_dp_cases_cpu.py holds every case to its event).
The batch is every case's reference and query, all against all, with the lane kernel forced at 64 and at 8 rows per wave, behind the slice join (8-byte
anchors) and the per-pair join (16-byte records), at c = 125 (band 20 = the window: behind the slice join the instance without a distance test, behind
the per-pair join the one with it), c = 250 (band 10: the instance with the test for both) and c = 110 (band 22: the 24-deep window). Every run checks
through the context's join counter that the join it asked for is the one that ran. The 80-byte hit records must equal, byte for byte, those of the lane-serial restatement of the oracle
(PSK_CHAIN_SERIAL=1) and of the wave-per-chunk kernel (PSK_CHAIN_LANE=0); the cases' own pairs are held to the oracle's integers."""
import ctypes as C
import os

import numpy as np
import pytest

import dp_cases as D

pytestmark = pytest.mark.gpu
INT_FIELDS = ("n_anchors", "n_chunks", "n_intervals", "covered_query", "covered_ref", "sum_chain_anchors", "sum_chunk_seeds")


@pytest.fixture(scope="module")
def batch(oracle):
    """the distinct genomes of the cases, and for every case the indices of its (query, reference)"""
    genomes, index, pairs = [], {}, {}
    for name, ref, qry in D.cases(oracle):
        for g in (ref, qry):
            if tuple(g) not in index:
                index[tuple(g)] = len(genomes)
                genomes.append((f"g{len(genomes)}", g))
        pairs[name] = (index[tuple(qry)], index[tuple(ref)])
    return genomes, pairs


def _records(genomes, c, env):
    import pyskani_amd as psk
    old = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("PSK_")}
    os.environ.update(env)
    try:
        db = psk.Database(compression=c)
        db.sketch_many([(n, *g) for n, g in genomes])
        lookups = C.c_uint64()
        assert db._lib.psk_ctx_join_work(db._ctx._h, None, None, None, None, 1) == 0
        recs, offs = db.query_handles(db.sketch_handles(), len(genomes), learned_ani=False, raw=True)
        assert db._lib.psk_ctx_join_work(db._ctx._h, C.byref(lookups), None, None, None, 0) == 0
        assert (lookups.value > 0) == (env["PSK_GSI_SLICE"] == "1"), (env, lookups.value)      # seed-index lookups: the slice join ran, or did not
    finally:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update(old)
    return recs, offs


_serial = {}


def _reference_run(genomes, c, gsl):
    """the records of the lane-serial path, once per (c, join)"""
    if (c, gsl) not in _serial:
        _serial[(c, gsl)] = _records(genomes, c, {"PSK_GSI_SLICE": gsl, "PSK_CHAIN_SERIAL": "1"})
    return _serial[(c, gsl)]


@pytest.mark.parametrize("gsl", ["1", "0"])
@pytest.mark.parametrize("c", [125, 250, 110])
def test_lane_kernels_equal_the_serial_and_wave_kernels_byte_for_byte(batch, c, gsl):
    genomes, pairs = batch
    want, want_offs = _reference_run(genomes, c, gsl)
    assert len(want) >= len(pairs) and want.dtype.itemsize == 80
    wave, _ = _records(genomes, c, {"PSK_GSI_SLICE": gsl, "PSK_CHAIN_LANE": "0"})
    assert wave.tobytes() == want.tobytes()
    for rows in ("64", "8"):
        got, offs = _records(genomes, c, {"PSK_GSI_SLICE": gsl, "PSK_CHAIN_LANE": rows})
        assert np.array_equal(offs, want_offs), (c, gsl, rows)
        assert got.tobytes() == want.tobytes(), (c, gsl, rows, [n for n in got.dtype.names if not np.array_equal(got[n], want[n])])


@pytest.mark.parametrize("gsl", ["1", "0"])
def test_every_case_pair_equals_the_oracle(batch, oracle, gsl):
    genomes, pairs = batch
    got, offs = _records(genomes, 125, {"PSK_GSI_SLICE": gsl, "PSK_CHAIN_LANE": "64"})
    for name, (qi, ri) in pairs.items():
        mine = got[offs[qi]:offs[qi + 1]]
        hit = mine[mine["ref_index"] == ri]
        assert len(hit) == 1, name
        want = oracle.chain(oracle.Sketch(genomes[ri][1]), oracle.Sketch(genomes[qi][1]))
        for f in INT_FIELDS:
            assert int(hit[0][f]) == int(getattr(want, f)), (name, f, int(hit[0][f]), int(getattr(want, f)))
        assert abs(float(hit[0]["ani"]) - want.ani) < 1e-6, name
