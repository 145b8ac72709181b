"""GPU: the tagged blocked seed index (csrc/seed_index.hip, csrc/slice_join.hip) against the untagged one and the per-pair join, on the inputs of
tests/index_tag_cases.py: a family astride two index blocks (local reference ids 255 and 0 beside tags 0xFF and 0x00), a reference that holds bucket neighbours
of the query's seeds (same bucket and another tag, same tag and another bucket, and what a forced index that forgot to refine its buckets would mistake for the
seed), and all-vs-alls at k = 14 and k = 16. Every case runs in one process of its own, a fresh database per setting ($PSK_BSI_TAG is read when an index is built); a case's runs are
made once and shared by the tests."""
import numpy as np
import pytest

import index_tag_cases as T
from rerun_cases import INT_FIELDS

pytestmark = pytest.mark.gpu
CASES = ["block_edge", "neighbours", "k14", "k16"]
_RUNS = {}


def run(name, config):
    """one child process per case runs all of the case's configurations, a fresh database for each"""
    if name not in _RUNS:
        configs = ["slice_tagged", "slice_untagged", "pairs_tagged", "slice_default"] + (["contig_tagged", "contig_untagged"] if name == "neighbours" else [])
        _RUNS[name] = T.run_child(name, configs)
    return _RUNS[name][config]


@pytest.mark.parametrize("name", CASES)
def test_tagged_untagged_and_per_pair_join_return_the_same_bytes(name):
    tagged, untagged, pairs = run(name, "slice_tagged"), run(name, "slice_untagged"), run(name, "pairs_tagged")
    assert tagged["record_bytes"] == 80 and tagged["n_records"] >= len(T.case(name)["queries"])      # every query finds a relative at least
    assert tagged["digest"] == untagged["digest"] == pairs["digest"]
    assert tagged["lookups"] > 0 and untagged["lookups"] > 0                                             # the slice join ran


@pytest.mark.parametrize("name", CASES)
def test_index_info_reports_what_was_forced_and_small_databases_stay_untagged(name):
    cs = T.case(name)
    tagged, untagged = run(name, "slice_tagged"), run(name, "slice_untagged")
    assert tagged["info_before"] == [0, 0, 0]                      # nothing is built by asking
    bits, shift, is_tagged = tagged["info"]
    assert is_tagged == 1 and shift <= 8 and bits + shift == 2 * cs["k"] and bits >= 2 * cs["k"] - 8
    bits0, shift0, is_tagged0 = untagged["info"]
    assert is_tagged0 == 0 and bits0 + shift0 == 2 * cs["k"] and bits0 < bits
    default = run(name, "slice_default")
    assert default["info"] == untagged["info"]                        # the sizes alone: these databases are too small to pay for finer buckets
    assert default["lookups"] > 0 and default["digest"] == tagged["digest"]
    if name == "block_edge":
        assert tagged["identity"] == 1                                # insertion order = locality order: slots 255 | 256 are the references the case means


@pytest.mark.parametrize("name", CASES)
def test_sampled_hits_and_planted_pairs_carry_the_oracles_integers(oracle, name):
    cs = T.case(name)
    recs = {(r[0], r[1]): r[2:2 + len(INT_FIELDS)] for r in run(name, "slice_tagged")["records"]}
    keys = sorted(recs)
    pick = np.random.default_rng(11)
    pairs = [keys[int(i)] for i in pick.choice(len(keys), min(6, len(keys)), replace=False)] + [tuple(p) for p in cs["planted"]]
    genomes = dict(cs["refs"])
    queries = dict(cs["queries"])
    sk = {}

    def sketch(kind, n):
        if (kind, n) not in sk:
            sk[(kind, n)] = oracle.Sketch((queries if kind == "q" else genomes)[n], c=cs["c"], marker_c=cs["marker_c"], k=cs["k"])
        return sk[(kind, n)]
    for q, r in pairs:
        assert (q, r) in recs, (q, r)
        want = oracle.chain(sketch("r", r), sketch("q", q))
        assert recs[(q, r)] == [int(getattr(want, f)) for f in INT_FIELDS], (q, r)
    if name == "neighbours":
        assert recs[("q", "planted")][0] == recs[("q", "plain")][0]      # n_anchors: no planted neighbour became an anchor


def test_contig_join_masks_the_tag_byte():
    """gsi_join_kernel on the blocked index (rerun_cases' bsi_two_pass switches) reads keys and values: the values' tag byte is there whether or not the index is
    tagged, the finer buckets only when it is."""
    tagged, untagged = run("neighbours", "contig_tagged"), run("neighbours", "contig_untagged")
    assert tagged["info"][2] == 1 and untagged["info"][2] == 0
    assert tagged["lookups"] > 0 and untagged["lookups"] > 0
    assert tagged["digest"] == untagged["digest"] == run("neighbours", "slice_tagged")["digest"]
