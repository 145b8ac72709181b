#!/usr/bin/env python3
"""What the bootstrap confidence intervals cost beside the all-vs-all they annotate: `Database.query_handles` (psk_query_many_min) against
`Database.query_handles_ci` (psk_query_many_ci) over the same database in the same process.

    python tools/interval_bench.py [--genomes 1000] [--iterations 100] [--reps 3] [--commit ID] [--out FILE]

The database is the family model of bench.py's all-vs-all, restated here: ancestors of iid ACGT with L ~ U[4.5, 5.5] Mb, families of 100, every member with
independent substitutions at a rate cycled from (0.0005, 0.002, 0.005, 0.01, 0.02, 0.04, 0.07, 0.10); built on the GPU, sketched once at the default parameters
(c = 125, marker c = 1000, k = 15). Each call is timed `--reps` times after one warm-up call (scratch, indexes, locality order); the line holds the median. The
kernels' own time comes from ONE more call with the timers on, run as a single chain of launches (PSK_PIPELINE=0: with two batches in flight a bracket's duration
says little about the kernels inside it): the "interval" bracket of psk_ctx_timing, and psk_ctx_interval_stats' pairs and draws, hence draws per second.
One JSON line; nothing is required of any number (append it to a file with --out). The two calls' shared fields are checked to be equal, so a line is never the
time of a different answer."""
import argparse
import ctypes as C
import json
import os
import platform
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIVERGENCE = (0.0005, 0.002, 0.005, 0.01, 0.02, 0.04, 0.07, 0.10)
FAMILY = 100


def family_genomes(torch, device, n, seed=3):
    """(ASCII buffer on the device, offsets, lengths) of n genomes in families of 100 on ancestors of 4.5 - 5.5 Mb"""
    rng = np.random.default_rng(seed)
    n_fam = max(1, n // FAMILY)
    anc_len = [int(rng.integers(4_500_000, 5_500_001)) for _ in range(n_fam)]
    fam_of = [min(i // FAMILY, n_fam - 1) for i in range(n)]
    offs, lens, total = [], [], 0
    for i in range(n):
        offs.append(total); lens.append(anc_len[fam_of[i]]); total += (anc_len[fam_of[i]] + 31) & ~15
    buf = torch.zeros(total + 64, dtype=torch.uint8, device=device)
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=device)
    g = torch.Generator(device=device)
    anc, anc_f = None, -1
    for i in range(n):
        f = fam_of[i]
        if f != anc_f:
            g.manual_seed(seed * 1_000_003 + f)
            anc, anc_f = torch.randint(0, 4, (anc_len[f],), generator=g, device=device, dtype=torch.uint8), f
        g.manual_seed(31 * 1_000_003 + i)
        mut = torch.rand(anc.shape, generator=g, device=device) < DIVERGENCE[i % len(DIVERGENCE)]
        shift = torch.randint(1, 4, anc.shape, generator=g, device=device, dtype=torch.uint8)
        buf[offs[i]:offs[i] + lens[i]] = lut[torch.where(mut, (anc + shift) & 3, anc).long()]
    torch.cuda.synchronize()
    return buf, offs, lens


def timed(fn, reps):
    fn()
    out, ms = None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, statistics.median(ms), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=1000)
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--rng-seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--commit", default="", help="the commit that was built (recorded in the line)")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    args = ap.parse_args()
    import torch      # (before the library: torch brings its own HIP runtime)
    import pyskani_amd
    n = args.genomes
    buf, offs, lens = family_genomes(torch, "cuda:0", n)
    db = pyskani_amd.Database()
    t0 = time.perf_counter()
    db.sketch_many_device([f"g{i}" for i in range(n)], buf.data_ptr(), offs, lens)
    sketch_ms = (time.perf_counter() - t0) * 1e3
    del buf
    torch.cuda.empty_cache()
    handles = db.sketch_handles()
    lib, ctx = db._lib, db._ctx._h
    (mn, moffs), min_ms, min_all = timed(lambda: db.query_handles(handles, n, learned_ani=False), args.reps)
    (ci, coffs), ci_ms, ci_all = timed(lambda: db.query_handles_ci(handles, n, iterations=args.iterations, rng_seed=args.rng_seed, learned_ani=False), args.reps)
    if not (np.array_equal(moffs, coffs) and all(ci[f].tobytes() == mn[f].tobytes() for f in mn.dtype.names)):
        raise SystemExit("the interval call's records are not the plain call's")
    if not ((ci["ci_lo"] <= ci["ci_hi"]).all() and (ci["ci_lo"] <= ci["ani"]).mean() > 0.9):
        raise SystemExit("the bounds do not bracket the ANI")
    # the kernels' own time: one call as a single chain of launches, timers on
    pairs, draws, tiers, ms, launches = C.c_uint64(), C.c_uint64(), (C.c_uint64 * 3)(), C.c_double(), C.c_uint64()
    had = os.environ.get("PSK_PIPELINE")
    os.environ["PSK_PIPELINE"] = "0"
    try:
        assert lib.psk_ctx_set_timing(ctx, 1) == 0 and lib.psk_ctx_timing(ctx, b"reset", None, None) == 0
        assert lib.psk_ctx_interval_stats(ctx, None, None, None, 1) == 0
        db.query_handles_ci(handles, n, iterations=args.iterations, rng_seed=args.rng_seed, learned_ani=False)
        assert lib.psk_ctx_timing(ctx, b"interval", C.byref(ms), C.byref(launches)) == 0
        assert lib.psk_ctx_interval_stats(ctx, C.byref(pairs), C.byref(draws), tiers, 0) == 0
        reduce_ms = C.c_double()
        assert lib.psk_ctx_timing(ctx, b"pair_reduce", C.byref(reduce_ms), None) == 0
    finally:
        lib.psk_ctx_set_timing(ctx, 0)
        if had is None:
            del os.environ["PSK_PIPELINE"]
        else:
            os.environ["PSK_PIPELINE"] = had
    width = (ci["ci_hi"] - ci["ci_lo"]).astype(np.float64)
    line = json.dumps({"genomes": n, "iterations": args.iterations, "rng_seed": args.rng_seed, "host": platform.node(), "commit": args.commit, "sketch_ms": sketch_ms,
                       "records": int(len(mn)), "query_many_min_ms": min_ms, "query_many_min_ms_all": min_all, "query_many_ci_ms": ci_ms, "query_many_ci_ms_all": ci_all,
                       "ci_over_min": ci_ms / min_ms, "interval_bracket_ms": ms.value, "interval_brackets": launches.value,
                       "pair_reduce_bracket_ms": reduce_ms.value, "pairs": pairs.value, "draws": draws.value, "tier_launches": list(tiers),
                       "draws_per_second": draws.value / (ms.value * 1e-3) if ms.value > 0 else None, "median_width": float(np.median(width)) if len(width) else None,
                       "timed": "median of --reps calls after one warm-up call; the brackets come from one more call with PSK_PIPELINE=0 and the timers on"})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
