#!/usr/bin/env python3
"""What the linkage forest costs beside the all-vs-all that feeds it and beside single linkage at one cut: `Database.triangle_records()`, then `forest_records` and
`cluster_records(linkage="single")` over the same records in the same process.

    python tools/forest_bench.py [--families 100] [--members 100] [--length 50000] [--step 0.0005] [--min-ani 0.80] [--commit ID] [--out FILE]

The database is tools/dereplicate_bench.py's: `families(F, M, L, step)`, F * M = 10 000 genomes by default, sketched once at c = 30 / marker c = 200. Every stage is
timed on its SECOND call (the first warms scratch, indexes and the locality order up). One JSON line: the stage times in ms, the record count, the edge count, the
forest's edge count, the Boruvka rounds that hooked a component, the pointer-jump launches, and the forest's time over single linkage's - the one comparison worth
recording: one forest answers every cut from its floor up, single linkage answers one. No time is required of anything: the line is a measurement (append it to a file
with --out). The forest is checked edge for edge against the sequential Kruskal below, so a line is never the time of a wrong answer."""
import argparse
import ctypes as C
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

from dereplicate_bench import families, timed      # noqa: E402  (the same generator, the same timing rule)


def kruskal_numpy(recs, n, min_ani, min_af):
    """(edges, a, b, ani): the edge count and the forest, sequentially - the edges deduplicated to their largest qualifying ani, sorted by (ani descending, a, b), a
    union-find walk (the check of the timed result; tests/forest_ref.py is the full restatement)"""
    q, r = (recs["query"] & np.uint32(0x7FFFFFFF)).astype(np.int64), recs["ref_index"].astype(np.int64)
    ok = (q != r) & (recs["ani"] >= np.float32(min_ani)) & (recs["af_query"] >= np.float32(min_af)) & (recs["af_ref"] >= np.float32(min_af))
    a, b, w = np.minimum(q, r)[ok], np.maximum(q, r)[ok], recs["ani"][ok]
    o = np.lexsort((-w.astype(np.float64), b, a))
    a, b, w = a[o], b[o], w[o]
    first = np.ones(len(a), bool)
    first[1:] = (a[1:] != a[:-1]) | (b[1:] != b[:-1])
    a, b, w = a[first], b[first], w[first]
    o = np.lexsort((b, a, -w.astype(np.float64)))
    a, b, w = a[o], b[o], w[o]
    parent = list(range(n))
    keep = np.zeros(len(a), bool)
    for i, (x, y) in enumerate(zip(a.tolist(), b.tolist())):
        while parent[x] != x:
            parent[x] = parent[parent[x]]; x = parent[x]
        while parent[y] != y:
            parent[y] = parent[parent[y]]; y = parent[y]
        if x != y:
            parent[max(x, y)] = min(x, y)
            keep[i] = True
    return len(a), a[keep].astype(np.uint32), b[keep].astype(np.uint32), w[keep]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=100)
    ap.add_argument("--members", type=int, default=100)
    ap.add_argument("--length", type=int, default=50_000)
    ap.add_argument("--step", type=float, default=0.0005)
    ap.add_argument("--min-ani", type=float, default=0.80, help="the forest's floor, and the cut single linkage is timed at")
    ap.add_argument("--min-af", type=float, default=0.5)
    ap.add_argument("--commit", default="", help="the commit that was built (recorded in the line)")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    args = ap.parse_args()
    if args.min_ani <= 0 or args.min_af <= 0:
        raise SystemExit("--min-ani and --min-af must be positive (the check below takes them as they are)")
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
    forest, forest_ms = timed(lambda: pyskani_amd.forest_records(recs, n, min_ani=args.min_ani, min_af=args.min_af))
    e, r, j = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert lib.psk_ctx_forest_stats(ctx._h, C.byref(e), C.byref(r), C.byref(j)) == 0
    (rep_of, _), single_ms = timed(lambda: pyskani_amd.cluster_records(recs, n, min_ani=args.min_ani, min_af=args.min_af, linkage="single"))
    n_edges, a, b, w = kruskal_numpy(recs, n, args.min_ani, args.min_af)
    if not (np.array_equal(forest.a, a) and np.array_equal(forest.b, b) and forest.ani.tobytes() == w.tobytes()):
        raise SystemExit("the forest is not the sequential Kruskal's")
    if e.value != n_edges or not np.array_equal(forest.labels(args.min_ani), rep_of):
        raise SystemExit("the forest's graph or its components at the floor are not single linkage's")
    line = json.dumps({"genomes": n, "families": args.families, "members": args.members, "length": args.length, "step": args.step, "min_ani": args.min_ani, "min_af": args.min_af,
                       "host": platform.node(), "commit": args.commit, "sketch_ms": sketch_ms, "triangle_ms": tri_ms, "records": int(len(recs)), "edges": e.value,
                       "forest_ms": forest_ms, "forest_edges": len(forest), "forest_rounds": r.value, "forest_jump_launches": j.value, "single_ms": single_ms,
                       "single_clusters": int((rep_of == np.arange(n)).sum()), "forest_over_single": forest_ms / single_ms, "forest_over_triangle": forest_ms / tri_ms,
                       "timed": "the second call of each stage; forest and single-linkage times include the records' upload and the result's download"})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
