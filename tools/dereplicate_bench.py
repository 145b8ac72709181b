#!/usr/bin/env python3
"""What dereplication costs beside the all-vs-all that feeds it: `Database.triangle_records()` and then `cluster_records` over its records, both linkages.

    python tools/dereplicate_bench.py [--families 100] [--members 100] [--length 50000] [--step 0.0005] [--commit ID] [--out FILE]

The database is `families(F, M, L, step)`: F random ancestors of L bases, M members each, member j mutated at rate step * j from its ancestor (the generator of
tests/test_gpu_triangle.py), F * M = 10 000 genomes by default, sketched once at c = 30 / marker c = 200. Every stage is timed on its SECOND call (the first warms
scratch, indexes and the locality order up). One JSON line: the stage times in ms, the record count, the edge count, the greedy rounds that decided a vertex, the
hook passes of single linkage, the representative counts, and the cluster stage's share of the triangle step. No time is required of anything: the line is a
measurement (append it to a file with --out). The greedy representatives are checked against the sequential walk below, so a line is never the time of a wrong
answer."""
import argparse
import ctypes as C
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LUT = np.frombuffer(b"ACGT", np.uint8)


def families(F, M, L, step, seed=123):
    rng = np.random.default_rng(seed)

    def mutate(a, d):
        b = a.copy(); m = rng.random(len(a)) < d; b[m] = (b[m] + rng.integers(1, 4, int(m.sum()), dtype=np.uint8)) & 3; return b
    anc = [rng.integers(0, 4, L, dtype=np.uint8) for _ in range(F)]
    return [(f"f{f}_m{j}", LUT[mutate(anc[f], step * j)].tobytes()) for f in range(F) for j in range(M)]


def greedy_numpy(recs, n, min_ani, min_af):
    """the greedy representatives in insertion order, sequentially (the check of the timed result; tests/dereplicate_ref.py is the full restatement)"""
    q, r = (recs["query"] & np.uint32(0x7FFFFFFF)).astype(np.int64), recs["ref_index"].astype(np.int64)
    ok = (q != r) & (recs["ani"] >= np.float32(min_ani)) & (recs["af_query"] >= np.float32(min_af)) & (recs["af_ref"] >= np.float32(min_af))
    nb = [[] for _ in range(n)]
    for a, b in zip(q[ok].tolist(), r[ok].tolist()):
        nb[a].append(b); nb[b].append(a)
    rep = np.zeros(n, bool)
    for v in range(n):
        rep[v] = not any(rep[u] for u in nb[v])
    return rep


def timed(fn):
    fn()
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=100)
    ap.add_argument("--members", type=int, default=100)
    ap.add_argument("--length", type=int, default=50_000)
    ap.add_argument("--step", type=float, default=0.0005)
    ap.add_argument("--min-ani", type=float, default=0.95)
    ap.add_argument("--min-af", type=float, default=0.5)
    ap.add_argument("--commit", default="", help="the commit that was built (recorded in the line)")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    args = ap.parse_args()
    import pyskani_amd
    g = families(args.families, args.members, args.length, args.step)
    n = len(g)
    db = pyskani_amd.Database(compression=30, marker_compression=200)
    t0 = time.perf_counter()
    db.sketch_many(g)
    sketch_ms = (time.perf_counter() - t0) * 1e3
    del g
    (recs, _), tri_ms = timed(lambda: db.triangle_records(learned_ani=False))
    lib, ctx = db._lib, db._ctx

    def stats():
        e, r, h = C.c_uint64(), C.c_uint64(), C.c_uint64()
        assert lib.psk_ctx_cluster_stats(ctx._h, C.byref(e), C.byref(r), C.byref(h)) == 0
        return e.value, r.value, h.value
    out = {}
    for linkage in ("greedy", "single"):
        (rep_of, _), ms = timed(lambda: pyskani_amd.cluster_records(recs, n, min_ani=args.min_ani, min_af=args.min_af, linkage=linkage))
        edges, rounds, hooks = stats()
        out[linkage] = {"ms": ms, "representatives": int((rep_of == np.arange(n)).sum()), "edges": edges, "rounds": rounds, "hook_passes": hooks}
        if linkage == "greedy" and not np.array_equal(rep_of == np.arange(n), greedy_numpy(recs, n, args.min_ani, args.min_af)):
            raise SystemExit("the greedy representatives are not the sequential walk's")
    line = json.dumps({"genomes": n, "families": args.families, "members": args.members, "length": args.length, "step": args.step, "min_ani": args.min_ani, "min_af": args.min_af,
                       "host": platform.node(), "commit": args.commit, "sketch_ms": sketch_ms, "triangle_ms": tri_ms, "records": int(len(recs)),
                       "edges": out["greedy"]["edges"], "greedy_ms": out["greedy"]["ms"], "greedy_rounds": out["greedy"]["rounds"],
                       "greedy_representatives": out["greedy"]["representatives"], "single_ms": out["single"]["ms"], "single_hook_passes": out["single"]["hook_passes"],
                       "single_representatives": out["single"]["representatives"], "greedy_over_triangle": out["greedy"]["ms"] / tri_ms,
                       "single_over_triangle": out["single"]["ms"] / tri_ms, "timed": "the second call of each stage; cluster times include the records' upload and the result's download"})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
