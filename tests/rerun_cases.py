"""Inputs that send a batch of the chain stage round again, one cause at a time, and inputs that sit on the seed indexes' contig limit.
Plain module: tests/test_rerun_cases_cpu.py checks on the oracle alone that every input is what it claims, tests/test_gpu_reruns.py runs every
case in a process of its own (the anchor arrays a process has grown decide whether a batch overflows) and holds the hits to the oracle.

The chain stage sizes its anchor arrays optimistically (`anchor_cap_for`, csrc/chain.hip) and reads one status block per batch; `chain_check`
sends the batch round again when the anchor total exceeds the capacity (psk_ctx_rerun_stats: `cap`), when a query seed has 255 or more matches in
a reference (`wide`), and the batch loop of query_many does so when a pair outgrows its room in the one-walk index join (`onepass`); the two-lane
pipeline hands a batch it cannot finish back to the one-chain loop (`refit`).

A case is a dict:
  c, marker_c     the database's parameters
  refs            [(name, [contig, ...])]
  queries         [(name, [contig, ...])]      one query_many call, in this order
  env             the switches that route it
  reruns          (cap, wide, onepass, refit) psk_ctx_rerun_stats must report for the first run in a fresh process
  lookups         None, or whether the seed indexes must have been walked (True: lookups > 0, False: lookups == 0)
  kind            "overflow" / "control" / "wide" / "onepass" / "contigs": what the CPU test checks on the oracle
Every generator is deterministic (fixed seeds); WORD_POS was found once by scanning the oracle's seeds of the sequence it indexes."""
import json
import os
import subprocess
import sys

import numpy as np

from sq_edges import mutate, random_genome

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_LENGTH_CONTIG = 500
K_MARKER = 21             # a seed's position is the last base of the 21-base window its 15-mer sits in the middle of
GSI_CONTIG_BITS = 15      # csrc/common.h: a seed-index entry holds 15 bits of contig number
WIDE_COUNT = 255          # csrc/join.hip: the packed join record's 8-bit count is full
INT_FIELDS = ("n_anchors", "n_chunks", "n_intervals", "covered_query", "covered_ref", "sum_chain_anchors", "sum_chunk_seeds")
FLOAT_FIELDS = ("ani", "af_query", "af_ref", "ani_std")


# the capacities anchor_cap_for (csrc/chain.hip) and the batch loops of csrc/query_many.hip size a batch's anchor arrays for, in a process
# whose arrays are still small (`items` = (pair, query seed) items of the batch)
def cap_general(items):
    return items + items // 4 + 65536


def cap_sparse(items):
    return items // 2 + 65536


def cap_slice(items):
    return min(cap_general(items), items // 4 * 3 + 65536)


def cap_onepass(items, pairs):
    return max(cap_sparse(items), items + items // 8 + 8 * (pairs + 1) + 64)


# ---------------------------------------------------------------------------------------------------------------- capacity
TANDEM_COPIES = 20
CAP_C, CAP_MC = 10, 40


def _planted(word, n, seed):
    """n copies of `word`, 25 random bases before each"""
    rng = np.random.default_rng(seed)
    return b"".join(random_genome(rng, 25) + word for _ in range(n))


WORD_POS = 20021      # a seed of default_rng(301)'s 60 000 bases at c = 10 whose 15-mer occurs once in them


def _wide_base():
    a = random_genome(np.random.default_rng(301), 60000)
    return a, a[WORD_POS - (K_MARKER - 1):WORD_POS + 1]


def gen_capacity(copies=TANDEM_COPIES, planted=0):
    """three queries against four references; in pair order (query, then reference) the overflowing pair rep x tandem sits between honest
    ones: pre x once, pre x mut, rep x once, REP x TANDEM, rep x mut, post x once, post x mut. `planted`: the tandem also holds the word of
    _wide_base (which rep holds once) that many more times"""
    rng = np.random.default_rng(4300)
    a = random_genome(rng, 60000)
    a2 = random_genome(rng, 20000)
    base, word = _wide_base()
    rep = base[15000:35000] + random_genome(rng, 80000)      # (the word once, inside)
    once = a[:30000] + rep + a[30000:]
    tandem = a2[:5000] + rep * copies + (_planted(word, planted, 77) if planted else b"") + a2[5000:]
    refs = [("once", [once]), ("tandem", [tandem]), ("mut", [mutate(rng, once, 0.02)]), ("none", [random_genome(rng, 50000)])]
    queries = [("pre", [a[2000:14000]]), ("rep", [rep]), ("post", [a[40000:52000]])]
    return dict(c=CAP_C, marker_c=CAP_MC, refs=refs, queries=queries)


# the switches that reach each emit path with a capacity guard of its own (profiles/r6/paths.md has the table of guard sites)
CAPACITY_ROUTES = [
    ("default", {}, "general"),                                                                   # anchor_join4 + scan + anchor_emit_packed4 (few pairs of ~5 000 seeds: chunk_hops)
    ("chunk_heads", {"PSK_CHUNK_HOPS": "0"}, "general"),                                          # ... with chunk_heads_kernel behind it
    ("emit_expand", {"PSK_EMIT_EXPAND": "1"}, "general"),                                         # anchor_emit_expand
    ("emit_pairs", {"PSK_EMIT_PAIRS": "1"}, "general"),                                           # anchor_emit_pairs, chunk table by pointer chase
    ("emit_pairs_heads", {"PSK_EMIT_PAIRS": "1", "PSK_CHUNK_HOPS": "0"}, "general"),              # ... chunk table written by the emit
    ("join_pairs", {"PSK_JOIN_PAIRS": "1"}, "general"),                                           # anchor_join_pairs + anchor_emit_packed4
    ("join_pairs_probe", {"PSK_JOIN_PAIRS": "1", "PSK_PROBE": "1", "PSK_GSI_JOIN": "0"}, "sparse"),   # anchor_join_probe + anchor_emit_packed4 at the pairs' starts
    ("wide", {"PSK_JOIN": "wide"}, "general"),                                                    # anchor_count + anchor_emit
    ("hops_items", {"PSK_CHUNK_HOPS": "1", "PSK_HOPS_ITEMS": "1"}, "general"),                    # chunk_hops_items beside anchor_emit_packed4
    ("gsi_two_pass", {"PSK_PROBE": "1", "PSK_JOIN_PAIRS": "1", "PSK_GSI_ONEPASS": "0", "PSK_BSI_SMALL": "0"}, "sparse"),   # gsi_join_kernel, database-wide index
    ("bsi_two_pass", {"PSK_PROBE": "1", "PSK_JOIN_PAIRS": "1", "PSK_GSI_ONEPASS": "0"}, "sparse"),                         # gsi_join_kernel, blocked index
    ("slice", {"PSK_GSI_SLICE": "1", "PSK_PIPELINE": "0"}, "slice"),                              # slice join, one chain
    ("slice_pipeline", {"PSK_GSI_SLICE": "1", "PSK_PIPELINE": "1"}, "slice"),                     # slice join, two lanes
]


# ---------------------------------------------------------------------------------------------------------------- wide format
def gen_wide(n_copies):
    """the word of _wide_base `n_copies` times in the reference "planted" (once in its homologous stretch, the rest planted behind it); the
    query holds it once, inside 20 000 homologous bases; "plain" holds the stretch without extra copies"""
    rng = np.random.default_rng(4400)
    base, word = _wide_base()
    planted = base + _planted(word, n_copies - 1, 78) + random_genome(rng, 2000)
    refs = [("plain", [mutate(rng, base, 0.01)]), ("planted", [planted]), ("other", [random_genome(rng, 40000)])]
    return dict(c=CAP_C, marker_c=CAP_MC, refs=refs, queries=[("q", [base[15000:35000]])])


WIDE_ROUTES = [
    ("join4", {}),                                                                        # anchor_join4_kernel raises need_wide
    ("join_pairs", {"PSK_JOIN_PAIRS": "1"}),                                              # anchor_join_pairs_kernel
    ("join_probe", {"PSK_JOIN_PAIRS": "1", "PSK_PROBE": "1", "PSK_GSI_JOIN": "0"}),       # anchor_join_probe_kernel
]


# ---------------------------------------------------------------------------------------------------------------- one-pass index join
def gen_onepass():
    """the input of test_gpu_fuzz.py::test_index_join_reruns_with_its_count_pass_when_a_reference_repeats_the_query"""
    rng = np.random.default_rng(4242)
    unit = random_genome(rng, 4000)
    a = random_genome(rng, 60000)
    refs = [("tandem", [a[:20000] + unit * 7 + a[20000:]]), ("once", [a[:30000] + unit + a[30000:]]),
            ("mut", [mutate(rng, a[:10000] + unit * 2 + a[10000:], 0.02)]), ("none", [random_genome(rng, 50000)])]
    queries = [("unit", [unit]), ("unit_mut", [mutate(rng, unit, 0.03)]), ("flank", [a[15000:27000]]), ("two", [unit * 2])]
    return dict(c=30, marker_c=200, refs=refs, queries=queries)


# ---------------------------------------------------------------------------------------------------------------- contig numbers
CONTIG_LIMIT = 1 << GSI_CONTIG_BITS


def contig_reference(n_contigs, seed):
    """n_contigs contigs of 500 - 520 random bases (~17 Mb at 32 768)"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(MIN_LENGTH_CONTIG, 521, n_contigs)
    bases = random_genome(rng, int(lens.sum()))
    offs = np.concatenate([[0], np.cumsum(lens)])
    return [bases[int(offs[i]):int(offs[i + 1])] for i in range(n_contigs)]


def gen_contigs(n_contigs, mixed=False):
    """one reference of n_contigs contigs; queries: a genome of the reference's last 150 and first 50 contigs (mutated; 200 contigs), and one
    contig each of numbers 0, 32 766, 32 767 and - where the reference has it - 32 768. mixed: ordinary references beside it"""
    contigs = contig_reference(n_contigs, 4500 + n_contigs)
    rng = np.random.default_rng(4600 + n_contigs)
    refs = [(f"contigs{n_contigs}", contigs)]
    if mixed:
        g = random_genome(rng, 120000)
        refs = [("g0", [g]), refs[0], ("g1", [mutate(rng, g, 0.02)]), ("few", [mutate(rng, x, 0.01) for x in contigs[-40:]])]
    genome = [mutate(rng, x, 0.02) for x in contigs[-150:] + contigs[:50]]
    queries = [("genome", genome)]
    for i in (0, CONTIG_LIMIT - 2, CONTIG_LIMIT - 1, CONTIG_LIMIT):
        if i < n_contigs:
            queries.append((f"contig{i}", [mutate(rng, contigs[i], 0.01)]))
    if mixed:
        queries.append(("g", [mutate(rng, refs[0][1][0][20000:90000], 0.01)]))
    return dict(c=CAP_C, marker_c=CAP_MC, refs=refs, queries=queries)


CONTIG_ROUTES = [("contig_join", {"PSK_PROBE": "1", "PSK_JOIN_PAIRS": "1"}), ("slice_join", {"PSK_GSI_SLICE": "1"})]


# ---------------------------------------------------------------------------------------------------------------- the cases
def _case(gen, kind, env, reruns, lookups=None, **extra):
    return dict(gen=gen, kind=kind, env=dict(env), reruns=tuple(reruns), lookups=lookups, **extra)


def cases():
    """{name: case}; the inputs are generated on demand (`materialise`): the contig references are 17 Mb each"""
    out = {}
    for name, env, formula in CAPACITY_ROUTES:
        out[f"capacity_{name}"] = _case((gen_capacity, ()), "overflow", env, (1, 0, 0, 0), formula=formula)
    out["capacity_control"] = _case((gen_capacity, (1,)), "control", {}, (0, 0, 0, 0), formula="general")      # the same shape, one copy: fits
    for name, env in WIDE_ROUTES:
        out[f"wide_254_{name}"] = _case((gen_wide, (WIDE_COUNT - 1,)), "wide", env, (0, 0, 0, 0), copies=WIDE_COUNT - 1)
        out[f"wide_255_{name}"] = _case((gen_wide, (WIDE_COUNT,)), "wide", env, (0, 1, 0, 0), copies=WIDE_COUNT)
    # the wide format first (chain_check looks at it first), then the capacity in that format: two retries, inside the limit of three
    out["wide_then_capacity"] = _case((gen_capacity, (TANDEM_COPIES, WIDE_COUNT - TANDEM_COPIES)), "overflow", {}, (1, 1, 0, 0), formula="general", copies=WIDE_COUNT)
    # the index joins keep no 8-bit count (an index entry is a whole match; slice_join.hip and gsi_join_kernel never touch need_wide): 255 matches
    # of one seed ask for nothing - no wide request, hence no refit of the pipeline's batch either
    out["wide_255_slice_pipeline"] = _case((gen_wide, (WIDE_COUNT,)), "wide", {"PSK_GSI_SLICE": "1", "PSK_PIPELINE": "1"}, (0, 0, 0, 0), lookups=True, copies=WIDE_COUNT)
    out["onepass"] = _case((gen_onepass, ()), "onepass", {"PSK_PROBE": "1", "PSK_JOIN_PAIRS": "1"}, (0, 0, 1, 0), lookups=True)
    out["onepass_off"] = _case((gen_onepass, ()), "onepass", {"PSK_PROBE": "1", "PSK_JOIN_PAIRS": "1", "PSK_GSI_ONEPASS": "0"}, (0, 0, 0, 0), lookups=True)
    for n in (CONTIG_LIMIT - 1, CONTIG_LIMIT, CONTIG_LIMIT + 1):
        for rname, env in CONTIG_ROUTES:
            out[f"contigs_{n}_{rname}"] = _case((gen_contigs, (n,)), "contigs", env, (0, 0, 0, 0), lookups=n <= CONTIG_LIMIT, n_contigs=n)
    for rname, env in CONTIG_ROUTES:
        out[f"contigs_mixed_{rname}"] = _case((gen_contigs, (CONTIG_LIMIT + 1, True)), "contigs", env, (0, 0, 0, 0), lookups=False, n_contigs=CONTIG_LIMIT + 1)
    return out


_MADE = {}


def materialise(case):
    """the case with its refs / queries / c / marker_c (generated once per generator call and process)"""
    fn, args = case["gen"]
    key = (fn.__name__, args)
    if key not in _MADE:
        if fn is gen_contigs:      # (17 Mb each: keep one)
            for k in [k for k in _MADE if k[0] == "gen_contigs"]:
                del _MADE[k]
        _MADE[key] = fn(*args)
    return {**case, **_MADE[key]}


# ---------------------------------------------------------------------------------------------------------------- oracle side
def oracle_pairs(O, case):
    """the batch as the oracle sees it: [(query, reference, query seeds, anchors)] of every pair that passes the screen, in pair order"""
    c, mc = case["c"], case["marker_c"]
    osk = [(n, O.Sketch(contigs, c=c, marker_c=mc)) for n, contigs in case["refs"]]
    out = []
    for qn, contigs in case["queries"]:
        q = O.Sketch(contigs, c=c, marker_c=mc)
        for rn, r in osk:
            if O.screen(q, r)[0]:
                out.append((qn, rn, len(q.seeds), int(O.chain(r, q).n_anchors)))
    return out


def oracle_records(O, case):
    """{query: {reference: Result}} of the oracle's screen + chain loop"""
    c, mc = case["c"], case["marker_c"]
    osk = [(n, O.Sketch(contigs, c=c, marker_c=mc)) for n, contigs in case["refs"]]
    return {qn: dict(O.query(osk, O.Sketch(contigs, c=c, marker_c=mc))) for qn, contigs in case["queries"]}


# ---------------------------------------------------------------------------------------------------------------- GPU side
def child_main(name):
    """(in a process of its own) the case's database, the query twice; one JSON line: counters, index lookups and records of both runs"""
    import ctypes as C
    import pyskani_amd as psk
    case = materialise(cases()[name])
    db = psk.Database(compression=case["c"], marker_compression=case["marker_c"])
    db.sketch_many([(n, *contigs) for n, contigs in case["refs"]])
    queries = [(n, *contigs) for n, contigs in case["queries"]]

    def counters():
        v = [C.c_uint64() for _ in range(4)]
        lk = C.c_uint64()
        assert db._lib.psk_ctx_rerun_stats(db._ctx._h, *[C.byref(x) for x in v], 1) == 0
        assert db._lib.psk_ctx_join_work(db._ctx._h, C.byref(lk), None, None, None, 1) == 0
        return [x.value for x in v], lk.value

    def run():
        counters()
        res = db.query_many(queries, learned_ani=False)
        cnt, lk = counters()
        recs = [[[h.reference_name] + [int(h._raw[f]) for f in INT_FIELDS] + [repr(float(h._raw[f])) for f in FLOAT_FIELDS] for h in hs] for hs in res]
        return dict(reruns=cnt, lookups=lk, records=recs)
    first = run()
    second = run()
    print(json.dumps(dict(first=first, second=second)))


def run_child(name, extra_env=None, timeout=900):
    case = cases()[name]
    env = {k: v for k, v in os.environ.items() if not k.startswith("PSK_")}
    env.update(case["env"])
    env.update(extra_env or {})
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import rerun_cases; rerun_cases.child_main(%r)" % (ROOT, os.path.join(ROOT, "tests"), name)
    out = subprocess.check_output([sys.executable, "-c", code], env=env, timeout=timeout).decode().strip().splitlines()[-1]
    return json.loads(out)
