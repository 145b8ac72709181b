"""GPU: the chain stage's rerun paths and the seed indexes' contig limit, on the inputs of tests/rerun_cases.py (held to what they claim by
tests/test_rerun_cases_cpu.py). A batch is sent round again when its anchors exceed the optimistically sized arrays, when a query seed has 255 or
more matches in a reference (the wide join format), or when a pair outgrows its room in the one-walk index join; while such an attempt is doomed
every emit kernel has to stay inside the capacity on its own and every pair has to be left empty - a slip is a write out of bounds that shows, if
at all, as a wrong hit of a neighbouring pair. psk_ctx_rerun_stats tells "rerun and right" from "never rerun".

Whether a batch overflows depends on what the process's anchor arrays grew to earlier, so every case runs in a fresh process, one at a time: the
database, the query once with the case's switches (counters, index lookups, records), the same query again. The parent holds, per case:
  - the first run's counters to the case's expectation exactly, and its index lookups to "walked" / "never walked" where the case says which;
  - the hits to the oracle: same hit sets, every chaining integer bit-exact, ANI and aligned fractions within 1e-6;
  - the records byte-identical to those of a second fresh process with PSK_CHAIN_SERIAL=1 (the lane-serial DP, whose capacity is reached by the
    same route: same counters);
  - the second run in the same process to identical records and NO capacity rerun (the arrays have grown); a wide request or an outgrown pair's
    room is a property of the input, not of the arrays, and comes again.

Out of scope: the wide format's other trigger, a reference contig number of 2^23 or more, needs a reference of at least 4.2 Gb."""
import subprocess

import pytest

import rerun_cases as RC

pytestmark = pytest.mark.gpu
CASES = RC.cases()


def _child(name, extra=None):
    """a child that died or hung ends the whole run: nothing more is started on a device that may have faulted"""
    try:
        return RC.run_child(name, extra)
    except (subprocess.CalledProcessError, subprocess.TimeoutExpired) as e:
        pytest.exit(f"{name}: the child process failed ({e}); no further case is started", returncode=1)


@pytest.mark.parametrize("name", list(CASES))
def test_rerun_case(oracle, name):
    case = RC.materialise(CASES[name])
    got = _child(name)
    first, second = got["first"], got["second"]
    print(name, "reruns (cap, wide, onepass, refit)", first["reruns"], "lookups", first["lookups"], "second run", second["reruns"], "hits", [len(r) for r in first["records"]])
    assert tuple(first["reruns"]) == case["reruns"], (name, first["reruns"], case["reruns"])
    if case["lookups"] is not None:
        assert (first["lookups"] > 0) == case["lookups"], (name, first["lookups"])
    want = RC.oracle_records(oracle, case)
    for (qn, _), recs in zip(case["queries"], first["records"]):
        g = {r[0]: r for r in recs}
        w = want[qn]
        assert len(g) == len(recs) and set(g) == set(w), (name, qn, sorted(set(g) ^ set(w)))
        for rn, res in w.items():
            for i, f in enumerate(RC.INT_FIELDS):
                assert g[rn][1 + i] == getattr(res, f), (name, qn, rn, f, g[rn][1 + i], getattr(res, f))
            fl = dict(zip(RC.FLOAT_FIELDS, map(float, g[rn][1 + len(RC.INT_FIELDS):])))
            assert abs(fl["ani"] - res.ani) < 1e-6 and abs(fl["af_query"] - res.af_query) < 1e-6 and abs(fl["af_ref"] - res.af_ref) < 1e-6, (name, qn, rn, fl)
    assert any(first["records"]), name
    assert second["records"] == first["records"], name
    assert tuple(second["reruns"]) == (0,) + case["reruns"][1:], (name, second["reruns"])
    serial = _child(name, {"PSK_CHAIN_SERIAL": "1"})["first"]
    assert tuple(serial["reruns"]) == case["reruns"], (name, serial["reruns"])
    assert serial["records"] == first["records"], name
