"""GPU: the fused small-query path (csrc/small_query.hip) at each of its fixed capacities and one past it (inputs:
tests/sq_edges.py, their oracle counts checked on CPU by tests/test_small_query_edges_cpu.py). Every query is held to the oracle
(hit set, every chain integer, ANI / AF at 1e-6) and to the general path over the same bytes (bit for bit), and the change of
psk_ctx_small_query_stats says which path answered: (1,0,0) taken, (0,1,1) flagged and rerun, (0,0,1) never tried - an at-cap
input that slid onto the general path, or an over-cap input the kernel did not flag, fails here.

The PSK_SQ_* switches are read once per process, so each setting runs the whole set (edges + fuzz) in a child process of its
own; every setting must give the default's digest."""
import hashlib
import os
import subprocess
import sys

import pytest

import sq_edges as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FUZZ = 100
CASES = E.edge_cases()


@pytest.fixture(scope="module")
def psk():
    import pyskani_amd
    return pyskani_amd


@pytest.mark.parametrize("cid", [cid for cid, _ in CASES])
def test_edge(psk, oracle, cid):
    case = dict(CASES)[cid]
    paths, _ = E.run_case(psk, oracle, case)
    assert paths == [case["path"]] * len(case["queries"])


def test_fuzz_of_the_fused_path(psk, oracle):
    """random small queries biased toward the edges: each is taken or flagged and rerun (never silently left on the general
    path) and matches the oracle; at least half of them are taken"""
    taken = 0
    for seed in range(N_FUZZ):
        paths, _ = E.run_case(psk, oracle, E.fuzz_case(seed), expect_path=False)
        assert paths[0] in ("taken", "rerun"), (seed, paths)
        taken += paths[0] == "taken"
    assert 2 * taken >= N_FUZZ, taken


CHILD = r"""
import hashlib, sys
sys.path[:0] = [%r, %r]
import pyskani_amd as psk
from oracle import oracle as O
import sq_edges as E
O.build()
h = hashlib.sha256(); n = taken = 0
for cid, case in E.edge_cases():
    paths, rows = E.run_case(psk, O, case)
    h.update(repr((cid, paths, rows)).encode()); n += len(rows)
for seed in range(%d):
    paths, rows = E.run_case(psk, O, E.fuzz_case(seed), expect_path=False)
    assert paths[0] in ("taken", "rerun"), (seed, paths)
    taken += paths[0] == "taken"
    h.update(repr((seed, paths, rows)).encode()); n += len(rows)
assert 2 * taken >= %d, taken
print(n, h.hexdigest())
""" % (ROOT, os.path.join(ROOT, "tests"), N_FUZZ, N_FUZZ)

SETTINGS = [{}, {"PSK_SQ_TEAM": "0"}, {"PSK_SQ_GRID": "1"}, {"PSK_SQ_ZEROCOPY": "0"}, {"PSK_SQ_PREFILTER": "0"}]


def test_switch_settings_give_the_default_digest(oracle):
    """PSK_SQ_TEAM=0 (one wave per chunk: the single-wave DP for pairs of one or two chunks), PSK_SQ_GRID=1 (one workgroup walks the
    whole shortlist: LDS state reset between pairs), PSK_SQ_ZEROCOPY=0 (the 257-hit case takes the second download),
    PSK_SQ_PREFILTER=0 (rescued contigs chained without the seed prefilter): each in a fresh process, every PSK_* variable
    stripped, each checking itself against the oracle; all print the default's digest. (The `oracle` fixture builds the oracle once,
    before the children start.)"""
    base = {k: v for k, v in os.environ.items() if not k.startswith("PSK_")}
    procs = [subprocess.Popen([sys.executable, "-c", CHILD], env={**base, **extra}, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
             for extra in SETTINGS]
    outs = []
    try:
        for p in procs:
            out, err = p.communicate(timeout=900)
            outs.append((p.returncode, out.decode().split(), err.decode()[-3000:]))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for extra, (rc, out, err) in zip(SETTINGS, outs):
        assert rc == 0, (extra, rc, err)
    digests = [tuple(out) for _, out, _ in outs]
    assert int(digests[0][0]) > 700
    for extra, d in zip(SETTINGS, digests):
        assert d == digests[0], extra
