"""CPU: triangle mode's host side - `triangle_matrix`, the two entry points in header / binding / ffi.rs, and the sharded all-vs-all handing the library's
triangle arguments (keys = the round's global query indices, ref_base = the shard's first global index) to its local database, over a two-rank gloo world."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _records(dtype, rows):
    from pyskani_amd import _capi
    recs = np.zeros(len(rows), np.dtype(dtype))
    qf = "query" if "query" in recs.dtype.names else "reserved"
    for k, (q, r, ani, afq, afr, learned) in enumerate(rows):
        recs[k]["ani"], recs[k]["af_query"], recs[k]["af_ref"], recs[k]["ref_index"] = ani, afq, afr, r
        if qf == "query":
            recs[k]["query"] = q | (0x80000000 if learned else 0)      # (bit 31 rides along in psk_hit_min and is no part of the index)
        else:
            recs[k]["reserved"], recs[k]["learned"] = q, int(learned)
    return recs


@pytest.mark.parametrize("kind", ["HitMin", "Hit"])
def test_triangle_matrix(kind):
    from pyskani_amd import _capi
    from pyskani_amd.database import triangle_matrix
    rows = [(0, 1, 0.99, 0.9, 0.8, False), (0, 3, 0.95, 0.5, 0.25, True), (2, 3, 0.875, 0.75, 0.125, True)]
    n = 6                                                   # larger than any index: genomes 4 and 5 have no hit at all
    ani, af = triangle_matrix(_records(getattr(_capi, kind), rows), n)
    assert ani.dtype == np.float32 and af.dtype == np.float32 and ani.shape == af.shape == (n, n)
    assert np.array_equal(ani, ani.T)
    want_ani, want_af = np.zeros((n, n), np.float32), np.zeros((n, n), np.float32)
    for q, r, a, afq, afr, _ in rows:
        want_ani[q, r] = want_ani[r, q] = a
        want_af[q, r], want_af[r, q] = afq, afr           # af[x, y]: the fraction of x aligned to y
    np.fill_diagonal(want_ani, 1.0); np.fill_diagonal(want_af, 1.0)
    assert np.array_equal(ani, want_ani) and np.array_equal(af, want_af)
    assert ani[0, 2] == 0.0 and af[2, 0] == 0.0 and ani[4, 5] == 0.0 and ani[5, 5] == 1.0      # absent pairs, the diagonal
    assert af[0, 3] == np.float32(0.5) and af[3, 0] == np.float32(0.25)
    lower = np.tril(ani)                                   # the layout skani prints
    assert lower[3, 0] == np.float32(0.95) and lower[0, 3] == 0.0
    e_ani, e_af = triangle_matrix(_records(getattr(_capi, kind), []), 3)
    assert np.array_equal(e_ani, np.eye(3, dtype=np.float32)) and np.array_equal(e_af, np.eye(3, dtype=np.float32))
    with pytest.raises(ValueError):
        triangle_matrix(_records(getattr(_capi, kind), rows), 3)


def test_entry_points_are_declared_everywhere_and_the_abi_revision_stays():
    from pyskani_amd import _capi
    header = open(os.path.join(ROOT, "include", "pyskani_amd.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "ffi.rs")).read()
    for name in ("psk_query_many_tri", "psk_query_many_tri_min"):
        assert re.search(r"\bpsk_status %s\s*\(" % name, header), name
        assert name in _capi.SYMBOLS
        assert re.search(r"pub fn %s\s*\(" % name, ffi), name
    assert re.search(r"^#define PSK_ABI_VERSION 7$", header, re.M) and _capi.ABI_VERSION == 7
    # the arguments the header gives the two calls: those of psk_query_many(_min) with the key array and the base after n_queries
    def args(nm):
        inner = re.search(r"psk_status %s\s*\(([^)]*)\)" % nm, header).group(1)
        return [(" ".join(a.split()[:-1]), a.split()[-1]) for a in inner.split(",")]
    for name, base in (("psk_query_many_tri", "psk_query_many"), ("psk_query_many_tri_min", "psk_query_many_min")):
        a_new, a_old = args(name), args(base)
        assert a_new[3:5] == [("const int64_t*", "query_key"), ("uint64_t", "ref_base")], a_new
        assert [t for t, _ in a_new[:3] + a_new[5:]] == [t for t, _ in a_old], (a_new, a_old)


def test_query_handles_checks_the_keys_before_any_library_call():
    """`keys` of the wrong length: ValueError, raised before the database is borrowed or the library entered (no GPU is needed to get there)."""
    from pyskani_amd.database import Database

    class Lib:
        def __getattr__(self, name): raise AssertionError("the library was called: " + name)
    db = Database.__new__(Database)
    db._lib, db._h = Lib(), None
    db._opts = lambda *a: None
    for keys in ([0, 1], [0, 1, 2, 3], [[0, 1, 2]]):
        with pytest.raises(ValueError):
            Database.query_handles(db, None, 3, keys=keys)
    with pytest.raises(ValueError):
        Database.query_handles(db, None, 3, keys=[0, 1, 2], ref_base=-1)


WORKER = r"""
import os, sys, numpy as np
sys.path.insert(0, %r)
import ctypes as C, threading
import torch.distributed as dist
from pyskani_amd.parallel import ShardedDatabase, TorchComm, shard_bounds, HIT_MIN_DTYPE, HIT_DTYPE, QUERY_MASK
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
N, BATCH = 11, 2
class Lib:
    freed = 0
    def psk_sketch_free_many(self, handles, n): Lib.freed += n
class ALocal:
    # stand-in local database: a genome's "handle" is 1000 + its global index; (q, r) is a hit iff (q + r) %% 3 == 0 - and, with keys, iff ref_base + r > key
    _device = 0; _ctx = None
    def __init__(self, lo, hi, triangle): self.lo, self.hi, self._lib, self.round, self.triangle, self.seen = lo, hi, Lib(), 0, triangle, 0
    def __len__(self): return self.hi - self.lo
    def sketch_handles(self): return (C.c_void_p * max(1, self.hi - self.lo))(*[1000 + g for g in range(self.lo, self.hi)])
    def query_handles(self, handles, total, raw=False, **kw):
        self.round += 1
        glob = [handles[qi] - 1000 for qi in range(total)]
        if self.triangle:
            assert set(kw) == {"keys", "ref_base"}, sorted(kw)
            assert [int(k) for k in kw["keys"]] == glob, (list(kw["keys"]), glob)      # the round's global query indices
            assert kw["ref_base"] == self.lo, (kw["ref_base"], self.lo)                  # the shard's first global index
            keys, base = [int(k) for k in kw["keys"]], int(kw["ref_base"])
        else:
            assert kw == {}, sorted(kw)                                                  # neither keyword
            keys, base = [-1] * total, 0
        self.seen += 1
        dt = HIT_DTYPE if raw else HIT_MIN_DTYPE
        rows, offs = [], [0]
        for qi, q in enumerate(glob):
            for r in range(self.hi - self.lo):
                if (q + self.lo + r) %% 3 == 0 and (keys[qi] < 0 or base + r > keys[qi]):
                    rec = np.zeros(1, dt)
                    rec["ani"], rec["af_query"], rec["af_ref"], rec["ref_index"] = 0.5 + q / 100 + (self.lo + r) / 10000, 0.25, 0.75, r
                    if raw: rec["learned"] = q %% 2
                    else: rec["query"] = qi | ((q %% 2) << 31)
                    rows.append(rec)
            offs.append(len(rows))
        return (np.concatenate(rows) if rows else np.zeros(0, dt)), np.array(offs, np.int64)
class AComm(TorchComm):
    def gather_sketch_handles(self, ctx, handles, dev):
        box = [None] * self.world
        self.dist.all_gather_object(box, [int(h) for h in handles])
        flat = [h for part in box for h in part]
        return (C.c_void_p * max(1, len(flat)))(*flat), [len(part) for part in box]
for raw in (False, True):
    for triangle in (True, False):
        lo, hi = shard_bounds(N, rank, world)
        loc = ALocal(lo, hi, triangle)
        sdb = ShardedDatabase(dist, local=loc, comm=AComm(dist), raw=raw)
        sdb.adopt_local(["g%%d" %% i for i in range(N)])
        Lib.freed = 0
        recs = sdb.all_vs_all_records(batch=BATCH, triangle=True) if triangle else sdb.all_vs_all_records(batch=BATCH)
        assert loc.seen == 3 and Lib.freed == N, (loc.seen, Lib.freed)      # three rounds of two genomes per rank, every one through the stand-in's checks
        want = [(q, r) for q in range(N) for r in range(N) if (q + r) %% 3 == 0 and (r > q or not triangle)]
        qs = (recs["reserved"] if raw else recs["query"] & QUERY_MASK).tolist()
        got = list(zip(qs, recs["ref_index"].tolist()))
        assert got == want, (raw, triangle, got[:8], want[:8])
        assert np.allclose(recs["ani"], [0.5 + q / 100 + r / 10000 for q, r in want], atol=1e-6)
        learned = (recs["learned"] != 0) if raw else ((recs["query"] >> 31) != 0)
        assert learned.tolist() == [q %% 2 == 1 for q, r in want]
# the Hit form: a genome's hits against later genomes only
lo, hi = shard_bounds(N, rank, world)
sdb = ShardedDatabase(dist, local=ALocal(lo, hi, True), comm=AComm(dist))
sdb.adopt_local(["g%%d" %% i for i in range(N)])
by_name = sdb.all_vs_all(batch=BATCH, triangle=True)
assert {q: [h.reference_name for h in hs] for q, hs in by_name.items()} == {"g%%d" %% q: ["g%%d" %% r for r in range(q + 1, N) if (q + r) %% 3 == 0] for q in range(N)}
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_sharded_triangle_world2_gloo():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, "-c", WORKER % ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert "rank 0 ok" in outs[0] and "rank 1 ok" in outs[1]
