#!/usr/bin/env python3
"""The all-vs-all of bench.py's family model as n independent queries (`full`) and in triangle mode (`triangle`: every unordered pair once, no genome against
itself): what chaining half the pairs buys.

    python tools/triangle_bench.py [--refs 10000] [--steps 5] [--warmup 2] [--legs full,triangle] [--commit ID] [--out FILE]

Each leg runs in a fresh child process (its own `timeout`; the parent stops at the first non-zero exit) on the same genomes, sketched and added to a database once;
a step is the QUERY alone (psk_query_many_min / psk_query_many_tri_min over the database's own sketches, the records on the host when it ends). A leg prints one
JSON line: ms per step (mean and min), the chain stage's work per step (psk_ctx_work pairs / items / anchors, psk_ctx_join_work lookups / visited), the number of
hits, the host's name and the commit, `hits_digest` = bench.records_digest of its records and `triangle_digest` = the same digest of the records with
ref_index > query (the full leg: its records filtered on the host; the triangle leg: all of its records). The parent requires the two legs' `triangle_digest`
to be equal and the triangle leg to have chained (pairs of the full leg - n) / 2 pairs; no ratio of the times is required."""
import argparse
import ctypes as C
import json
import os
import platform
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(args):
    import numpy as np
    import torch
    from bench import family_layout, make_genomes, Engine, timed_loop, records_digest
    n = args.refs
    dev = torch.device("cuda", 0)
    n_fam = max(1, n // 100)
    anc_lens, fam_of = family_layout(3, n, n_fam)
    ids = list(range(n))
    buf, offs, lens = make_genomes(torch, dev, 3, 31, ids, fam_of, anc_lens)
    torch.cuda.synchronize()
    eng = Engine(0)
    names = (C.c_char_p * n)(*[f"g{i}".encode() for i in ids])
    c_off, c_len, gfc, _ = eng.layout(offs, lens)
    handles = eng.sketch_device_c(buf.data_ptr(), c_off, c_len, gfc, n)
    db = eng.make_db(names, handles, n)
    eng.sync(); torch.cuda.synchronize()
    del buf      # (the ASCII has been sketched: its 50 GB go back before the query's scratch is sized)
    torch.cuda.empty_cache()
    triangle = args.child == "triangle"
    keys = (C.c_int64 * n)(*range(n))
    opts = eng.capi.QueryOpts(0, 0, 0, 0, 0.0, 0.0, None)
    last = {}

    def step():
        hits_p = C.POINTER(eng.capi.HitMin)()
        offsets = (C.c_uint64 * (n + 1))()
        if triangle:
            eng.capi.check(eng.lib.psk_query_many_tri_min(db, handles, n, keys, 0, C.byref(opts), C.byref(hits_p), offsets))
        else:
            eng.capi.check(eng.lib.psk_query_many_min(db, handles, n, C.byref(opts), C.byref(hits_p), offsets))
        try:
            nh = int(offsets[n])
            last["recs"] = eng.capi.hit_records(hits_p, 0, nh, eng.hit_min_dtype)      # (the records on the host, as a caller receives them: part of the step in both legs)
        finally:
            if hits_p:
                eng.lib.psk_free(hits_p)
        return nh

    def fence():
        eng.sync(); torch.cuda.synchronize()
    try:
        dt, n_hits, _, work, _ = timed_loop(eng, step, args.steps, args.warmup, fence)
        step_ms = list(timed_loop.last_step_ms)
        recs = last["recs"]
        q = recs["query"] & np.uint32(0x7FFFFFFF)
        upper = recs[recs["ref_index"] > q]
        print(json.dumps({"leg": args.child, "refs": n, "host": platform.node(), "commit": args.commit, "ms_per_step_mean": dt / args.steps * 1e3, "ms_per_step_min": min(step_ms),
                          "step_ms": step_ms, "steps": args.steps, "warmup": args.warmup, "step": "query only (database sketched and built once, before the warm-up)",
                          "hits": int(n_hits), "chained_pairs_per_step": work["chained_pairs"], "items_per_step": work["items"], "anchors_per_step": work["anchors"],
                          "index_lookups_per_step": work["index_lookups"], "index_entries_visited_per_step": work["index_entries_visited"],
                          "hits_digest": records_digest(recs), "triangle_hits": int(len(upper)), "triangle_digest": records_digest(upper)}))
    finally:
        eng.lib.psk_db_destroy(db)
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="full,triangle")
    ap.add_argument("--timeout", type=int, default=540, help="seconds per child")
    ap.add_argument("--commit", default="", help="the commit that was built (recorded in every line)")
    ap.add_argument("--out", default=None, help="append the children's JSON lines to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    lines = {}
    for leg in args.legs.split(","):
        if leg not in ("full", "triangle"):
            raise SystemExit(f"unknown leg {leg!r}")
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", leg, "--refs", str(args.refs), "--steps", str(args.steps),
               "--warmup", str(args.warmup), "--commit", args.commit]
        p = subprocess.run(cmd, stdout=subprocess.PIPE)
        if p.returncode != 0:
            raise SystemExit(f"the {leg} leg ended with status {p.returncode}")
        line = p.stdout.decode().strip().splitlines()[-1]
        print(line, flush=True)
        lines[leg] = json.loads(line)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    if len(lines) == 2:
        f, t = lines["full"], lines["triangle"]
        if f["triangle_digest"] != t["triangle_digest"] or t["hits_digest"] != t["triangle_digest"]:
            raise SystemExit(f'the triangle\'s records ({t["hits_digest"]}, {t["hits"]} hits) are not the full run\'s records with ref_index > query ({f["triangle_digest"]}, {f["triangle_hits"]} hits)')
        if 2 * t["chained_pairs_per_step"] != f["chained_pairs_per_step"] - f["refs"]:
            raise SystemExit(f'the triangle chained {t["chained_pairs_per_step"]} pairs per step, the full run {f["chained_pairs_per_step"]}: not (full - n) / 2')
        print(json.dumps({"full_over_triangle_mean": f["ms_per_step_mean"] / t["ms_per_step_mean"], "full_over_triangle_min": f["ms_per_step_min"] / t["ms_per_step_min"]}), flush=True)


if __name__ == "__main__":
    main()
