#!/usr/bin/env python3
"""The all-vs-all of bench.py's family model with the genomes inserted family by family and in a random order: what the insertion order costs.

    python tools/insertion_order_bench.py [--refs 10000] [--steps 5] [--warmup 2] [--locality 0|1] [--orders sorted,shuffled,shuffled:0] [--commit ID] [--out FILE]

Each leg runs in a fresh child process (its own `timeout`; the parent stops at the first non-zero exit) and prints one JSON line: ms per step (mean and min),
index lookups and visited entries per step (psk_ctx_join_work), index blocks per query, the locality order's n_groups / is_identity, the host's name and the
commit, and two digests that must be the same for every leg, since the shuffled job holds the same genomes (bench.make_genomes builds a genome from its global
index): `names_digest` over (query name, reference name, ani, af_query, af_ref) sorted by names, and `hits_digest` = bench.records_digest of the records keyed
by GLOBAL genome index and sorted by (query, reference) - for 10 000 genomes the `hits_digest` that `python bench.py --gpus 1` prints.
--locality 0 sets PSK_LOCALITY=0 in every child (insertion order kept: the behaviour without the order); a leg written `shuffled:0` sets it for that leg alone."""
import argparse
import ctypes as C
import hashlib
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
    if args.child == "shuffled":
        ids = [int(x) for x in np.random.default_rng(args.seed).permutation(n)]
    buf, offs, lens = make_genomes(torch, dev, 3, 31, ids, fam_of, anc_lens)
    torch.cuda.synchronize()
    eng = Engine(0)
    names_py = [f"g{i}" for i in ids]
    names = (C.c_char_p * n)(*[s.encode() for s in names_py])
    c_off, c_len, gfc, _ = eng.layout(offs, lens)
    last = {}

    def step():
        out = eng.sketch_device_c(buf.data_ptr(), c_off, c_len, gfc, n)
        db = eng.make_db(names, out, n)
        try:
            nh, (recs, qoffs) = eng.query_many(db, out, n, keep=True)
            last["recs"] = recs
            return nh
        finally:
            eng.lib.psk_db_destroy(db)

    def fence():
        eng.sync(); torch.cuda.synchronize()
    dt, n_hits, _, work, _ = timed_loop(eng, step, args.steps, args.warmup, fence)
    step_ms = list(timed_loop.last_step_ms)
    recs = last["recs"]
    # the order and its groups, from a database built for the purpose (outside the timed loop: counting the groups is a grouping pass of its own)
    out = eng.sketch_device_c(buf.data_ptr(), c_off, c_len, gfc, n)
    db = eng.make_db(names, out, n)
    try:
        slot_of = np.empty(n, np.uint32); g, ident = C.c_uint32(), C.c_uint32()
        eng.capi.check(eng.lib.psk_db_locality(db, slot_of.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(g), C.byref(ident)))
        groups, ident = g.value, ident.value
    finally:
        eng.lib.psk_db_destroy(db)
    # index blocks (256 slots) that hold one of a query's hits, mean over the queries
    q = (recs["query"] & np.uint32(0x7FFFFFFF)).astype(np.int64)
    blk = (slot_of[recs["ref_index"]] >> 8).astype(np.int64)
    blocks_per_query = len(np.unique(q * (1 << 24) + blk)) / max(1, len(np.unique(q)))
    qn = np.array(names_py)[q]; rn = np.array(names_py)[recs["ref_index"]]
    order = np.lexsort((rn, qn))
    h = hashlib.sha256()
    h.update("\n".join(f"{a} {b}" for a, b in zip(qn[order], rn[order])).encode())
    for f in ("ani", "af_query", "af_ref"):
        h.update(np.ascontiguousarray(recs[f][order]).tobytes())
    gid = np.asarray(ids, dtype=np.uint32)      # the records keyed by global genome index, in (query, reference) order: what the sorted job returns as it is
    glob = recs.copy()
    glob["query"] = gid[q]; glob["ref_index"] = gid[recs["ref_index"]]
    glob = glob[np.lexsort((glob["ref_index"], glob["query"]))]
    print(json.dumps({"order": args.child, "refs": n, "host": platform.node(), "commit": args.commit, "hits_digest": records_digest(glob), "locality_switch": os.environ.get("PSK_LOCALITY", "1"), "ms_per_step_mean": dt / args.steps * 1e3, "ms_per_step_min": min(step_ms),
                      "step_ms": step_ms, "steps": args.steps, "warmup": args.warmup, "hits": int(n_hits), "index_lookups_per_step": work["index_lookups"],
                      "index_entries_visited_per_step": work["index_entries_visited"], "visited_per_lookup": work["index_entries_visited"] / max(1.0, work["index_lookups"]),
                      "index_blocks_per_query": blocks_per_query, "n_groups": groups, "is_identity": ident, "names_digest": h.hexdigest()[:16]}))
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=17)
    ap.add_argument("--locality", choices=("0", "1"), default="1")
    ap.add_argument("--orders", default="sorted,shuffled")
    ap.add_argument("--timeout", type=int, default=540, help="seconds per child")
    ap.add_argument("--commit", default="", help="the commit that was built (recorded in every line)")
    ap.add_argument("--out", default=None, help="append the children's JSON lines to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    lines = []
    for leg in args.orders.split(","):
        order, _, loc = leg.partition(":")
        env = dict(os.environ)
        if (loc or args.locality) == "0":
            env["PSK_LOCALITY"] = "0"
        else:
            env.pop("PSK_LOCALITY", None)
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", order, "--refs", str(args.refs), "--steps", str(args.steps),
               "--warmup", str(args.warmup), "--seed", str(args.seed), "--commit", args.commit]
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE)
        if p.returncode != 0:
            raise SystemExit(f"the {order} run ended with status {p.returncode}")
        line = p.stdout.decode().strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(json.loads(line))
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    if len({(x["names_digest"], x["hits_digest"]) for x in lines}) > 1:
        raise SystemExit("the legs disagree: " + ", ".join(f'{x["order"]}={x["names_digest"]}/{x["hits_digest"]}' for x in lines))


if __name__ == "__main__":
    main()
