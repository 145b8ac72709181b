"""Batches built for the size tiers of the chain selection (csrc/select.hip) and of the per-pair reduce (csrc/reduce.hip), a restatement of the
host's launch predicates (csrc/chain.hip chain_run) from the capacity rows alone, and a plain numpy reference of the reduce. Used by
test_tier_cases_cpu.py (every case holds its promises with the oracle alone; no GPU) and test_gpu_tiers.py (every case through query_many).

The lever is a query of many short contigs: a chunk row is a run of anchors on one query contig, so a query of N contigs of 1 000 - 2 000 bases, each a
mutated copy of its own reference segment, has N rows and N candidate chains against the reference that holds all N segments, and n of each against
a reference that holds n of them. Everything is at c = 30, marker_c = 200, k = 15 (a 250-base piece still carries a candidate chain; a genome below
4 000 bases has fewer than 20 markers and is rescued against everything).

A world (World) is one such query with a few special contigs:
  dup       a second, more diverged copy of a segment another contig (its primary) copies: its candidate loses on the reference, its row keeps no chain
  piece     (made on the reference side) a reference that holds only 60 bases of a contig: the row has one or two anchors, no candidate
A reference is a choice of segments, so the rows of a pair are the query's contigs whose segment it holds, in the query's order. The primaries
(`n` rows) hold n ordinary segments: rows = candidates = kept = n. The twins (`n t`) hold the segments of query positions 0 .. n - 1 with dups at
rows 0, 32, 64, 255, 512, 1024 (4096) and pieces at rows 1, 63, 256 and n - 2: rows without a kept chain at the first row, the last row and on both
sides of rows 63 / 64 and 255 / 256, so that the kept count m is below the row count nc.

Cases (cases(oracle) -> {name: Case}); every case is ONE call of query_many = one batch of the chain stage:
  edges_a   n_pairs > 4096, capacity average < 16: the live list, the lane kernels (select_tiny, pair_empty, pair_reduce_tiny), and every wave /
            workgroup tier behind them. Holds the tiny selection's candidate edges (tiny_4r8c, tiny_4r9c, tiny_5r5c, tiny_1r9c).
  edges_b   n_pairs <= 4096, 16 <= average <= 512, rows_pair_max > 64: small and wave reduce, no live list, empty records by the small kernel
  edges_c   average > 512: the workgroup kernels alone
  edges_d   rows_pair_max <= 64, average < 16: no workgroup launch at all (pairs of 1, 4, 5, 64 rows)
  big       rows 4096, 4097 and the twin of 4097 (nc > 4096 >= m): the LDS sort's capacity and the global sort beyond it
  conflicts 128 / 129 mutually conflicting candidates (rank sort / bitonic sort of the conflicted list; two copies byte-identical: equal scores fall to
            generation order), and one long candidate whose reference span holds 70 later, mutually disjoint short ones (only the running maximum
            carried across a 64-lane group marks those beyond the first 64 as conflicted)"""
import numpy as np

C, MARKER_C, K = 30, 200, 15
FRAGMENT_LENGTH = 20000
SMALL_MARKER_COUNT = 20
MIN_ANCHORS = 3
TINY_ROWS, TINY_CANDS = 4, 8            # select_tiny_kernel
CSMALL, CMAX = 512, 1024                # select_kernel / select_mid_kernel
RW_PER, RED_SMALL, RED_CAP = 8, 1024, 4096
LIVE_PAIRS = 4096                       # the live list is used beyond this many pairs
FLAGS = ({}, {"median": True}, {"robust": True})
TOL = 1e-6                              # the suite's tolerance on ani / af / ani_std (test_gpu_parity.py)
LUT = np.frombuffer(b"ACGT", np.uint8)
# psk_ctx_tier_stats, in its order
STATS = ("select_tiny", "pair_empty", "reduce_tiny", "reduce_small", "reduce_wave", "reduce_group", "reduce_large", "live", "rest", "mid", "big")

DUPS = {0: 2, 32: 30, 64: 60, 255: 250, 512: 508, 1024: 1020, 4096: 4090}      # query position of a dup -> of its primary


def _enc(a):
    return LUT[a].tobytes()


def _rand(rng, n):
    return rng.integers(0, 4, n, dtype=np.uint8)


def _mutate(rng, a, d):
    b = a.copy()
    m = rng.random(len(a)) < d
    b[m] = (b[m] + rng.integers(1, 4, int(m.sum()), dtype=np.uint8)) & 3
    return b


def sketch(oracle, contigs):
    return oracle.Sketch(contigs, c=C, marker_c=MARKER_C, k=K)


# ---- the reduce, restated (oracle/skani_oracle.c orc_chain pass 3; csrc/reduce.hip)

def chunk_values(chunks, k=K):
    a, s = chunks["anchors"].astype(np.float64), chunks["seeds"].astype(np.float64)
    return np.minimum(a / np.maximum(s - 1, 1), 1.0) ** (1.0 / k)


def _mean(v):
    return float(np.sum(v.astype(np.longdouble)) / len(v))


def _trim(m):
    return (m // 10, m - m // 10) if m - 2 * (m // 10) > 0 else (0, m)


def reduce_ref(chunks, k=K, median=False, robust=False):
    """(ani, ani_std) of a pair from the oracle's records of its chunks that kept a chain (oracle.last_chunks(), chunk order)"""
    v = chunk_values(chunks, k)
    m = len(v)
    if m == 0:
        return -1.0, 0.0
    s = np.sort(v)
    if median:
        ani = float(s[m // 2])
    elif robust:
        lo, hi = _trim(m)
        ani = _mean(s[lo:hi])
    else:
        ani = _mean(v)
    mean = np.sum(v.astype(np.longdouble)) / m
    ssq = np.sum((v.astype(np.longdouble) - mean) ** 2)
    return ani, float(np.sqrt(ssq / (m - 1))) if m > 1 else 0.0


def slip_margins(chunks, k=K):
    """how far each named slip of a reduce kernel moves the pair's result: {slip: |wrong - right|} for the slips the pair's m allows"""
    return value_margins(chunk_values(chunks, k))


def value_margins(v):
    v = np.asarray(v, np.float64)
    m = len(v)
    out = {}
    if m < 3:
        return out
    s = np.sort(v)
    out["median_index_minus_1"] = abs(float(s[m // 2 - 1] - s[m // 2]))
    if m // 2 + 1 < m:
        out["median_index_plus_1"] = abs(float(s[m // 2 + 1] - s[m // 2]))
    lo, hi = _trim(m)
    right = _mean(s[lo:hi])
    for name, a, b in (("trim_lo_plus_1", lo + 1, hi), ("trim_lo_minus_1", lo - 1, hi), ("trim_hi_minus_1", lo, hi - 1), ("trim_hi_plus_1", lo, hi + 1)):
        if 0 <= a < b <= m:
            out[name] = abs(_mean(s[a:b]) - right)
    if m <= 1025:
        mean = np.sum(v.astype(np.longdouble)) / m
        ssq = np.sum((v.astype(np.longdouble) - mean) ** 2)
        out["std_over_m"] = abs(float(np.sqrt(ssq / m)) - float(np.sqrt(ssq / (m - 1))))
    return out


# ---- the host's launch predicates, restated from the capacity rows (csrc/chain.hip make_desc, chain_run)

def capacity_rows(contigs):
    """chunk-table rows the host reserves for every pair of a query that has seeds: chunk heads on one contig are more than FRAGMENT_LENGTH apart"""
    return sum(len(x) // (FRAGMENT_LENGTH + 1) + 1 for x in contigs)


def regime(pair_rows, mean=True, off=()):
    """pair_rows: the capacity rows of every pair of the batch -> which kernels the host launches. off: the switches set against their tiers, of
    PSK_REDUCE_TINY=0 ("reduce_tiny"), PSK_REDUCE_SMALL=0 ("reduce_small"), PSK_REDUCE_WAVE=0 ("reduce_wave"), PSK_SELECT_TINY=0 ("select_tiny")
    and PSK_CHAIN_SERIAL=1 ("serial")"""
    n_pairs, n_rows, rpm = len(pair_rows), sum(pair_rows), max(pair_rows)
    avg = n_rows // n_pairs
    live = n_pairs > LIVE_PAIRS
    wave = "reduce_wave" not in off and "reduce_small" not in off and rpm > 64 and avg <= 64 * RW_PER
    small = "reduce_small" not in off and (avg < 16 or wave)
    return {"n_pairs": n_pairs, "n_rows": n_rows, "rows_pair_max": rpm, "average": avg, "serial": "serial" in off,
            "select_tiny": live and avg < 16 and "select_tiny" not in off and "serial" not in off, "pair_empty": live,
            "reduce_tiny": small and mean and avg < 16 and "reduce_tiny" not in off, "reduce_small": small, "reduce_wave": wave,
            "reduce_group": not ((small and rpm <= 64) or (small and wave and rpm <= 64 * RW_PER)),
            "reduce_large": n_rows > RED_SMALL and rpm > RED_SMALL}


SWITCHES = {"PSK_REDUCE_TINY": ("0", "reduce_tiny"), "PSK_REDUCE_SMALL": ("0", "reduce_small"), "PSK_REDUCE_WAVE": ("0", "reduce_wave"),
            "PSK_SELECT_TINY": ("0", "select_tiny"), "PSK_CHAIN_SERIAL": ("1", "serial")}


def expected_stats(reg, rows, cands):
    """psk_ctx_tier_stats after one run of the batch: launches as 0 / 1, then the pairs of the lists; rows / cands: actual rows and candidates of every pair.
    (The lane-serial selection of PSK_CHAIN_SERIAL=1 takes every pair in the first tier: nothing is passed on.)"""
    live = [i for i, r in enumerate(rows) if r > 0]
    after_tiny = [i for i in live if rows[i] > TINY_ROWS or cands[i] > TINY_CANDS] if reg["select_tiny"] else live
    return {**{k: int(reg[k]) for k in STATS[:7]},
            "live": len(live) if reg["pair_empty"] else 0, "rest": len(after_tiny) if reg["select_tiny"] else 0,
            "mid": 0 if reg["serial"] else sum(1 for i in after_tiny if cands[i] > CSMALL), "big": 0 if reg["serial"] else sum(1 for i in after_tiny if cands[i] > CMAX)}


# ---- worlds

class World:
    """a query of n short contigs over its own segments, with dups at the positions of DUPS; no k-mer is shared between a contig and another's segment"""

    def __init__(self, oracle, seed, n, lo, hi):
        rng = np.random.default_rng(seed)
        self.n = n
        self.dups = {d: p for d, p in DUPS.items() if d < n}
        self.special = set(self.dups) | set(self.dups.values())
        self.seg = [None] * n
        self.qry = [None] * n
        self.rate = [0.0] * n

        def draw(i):
            if i in self.dups:
                self.seg[i], self.rate[i] = self.seg[self.dups[i]], 0.06
            else:
                self.seg[i] = _rand(rng, int(rng.integers(lo, hi)))
                self.rate[i] = 0.01 if i in self.special else float(rng.uniform(0, 0.08))
            self.qry[i] = _mutate(rng, self.seg[i], self.rate[i])
        for i in sorted(range(n), key=lambda i: i in self.dups):      # (primaries before their dups)
            draw(i)
        own = np.arange(n)
        for d, p in self.dups.items():
            own[d] = p
        # Seeds are the k-mers whose hash falls in 1 / c of the range, so two unrelated seeds are equal 30 times as often as two unrelated 15-mers: a 2 Mb
        # query has dozens of chance matches with foreign segments, each one a row of one anchor. The base in the middle of such a query seed is changed
        # (in the contig and in its segment) until none is left.
        for _ in range(20):
            rs = sketch(oracle, [_enc(s) for s in self.seg]).seeds
            qs = sketch(oracle, [_enc(q) for q in self.qry]).seeds
            order = np.argsort(rs["kmer"], kind="stable")
            rk, rc = rs["kmer"][order], rs["contig"][order].astype(np.int64)
            a, b = np.searchsorted(rk, qs["kmer"], "left"), np.searchsorted(rk, qs["kmer"], "right")
            bad = [int(j) for j in np.nonzero(b > a)[0] if np.any(own[rc[a[j]:b[j]]] != own[int(qs["contig"][j])])]
            if not bad:
                break
            for j in bad:
                i, at = int(qs["contig"][j]), int(qs["pos"][j]) - 10      # (a seed's `pos` is the end of the 21-base window its 15-mer is centred in: bases pos - 17 .. pos - 3)
                self.qry[i][at] = (self.qry[i][at] + 1 + rng.integers(0, 3)) & 3
                if self.seg[i] is self.seg[own[i]] and i != own[i]:      # (a dup shares its segment with the primary: the dup alone changes)
                    continue
                self.seg[i][at] = self.qry[i][at]
        else:
            raise AssertionError("chance matches did not go away")
        self._seeds = np.unique(qs["kmer"])
        # a row's value depends on its contig and segment alone: one chain against every segment gives the value of every ordinary contig
        oracle.chain(sketch(oracle, [_enc(self.seg[i]) for i in range(n) if i not in self.dups]), sketch(oracle, [_enc(q) for q in self.qry]))
        ch = oracle.last_chunks()
        self.val = dict(zip(ch["contig"].tolist(), chunk_values(ch).tolist()))
        self.ordinary = [i for i in range(n) if i not in self.special]
        self.query = [_enc(q) for q in self.qry]
        self._rng = rng
        self._oracle = oracle

    def _weak(self, kept):
        """the contig among `kept` whose value makes a slip invisible (a tie beside the median, mostly), or None when every slip moves the result by 2 TOL"""
        v = np.array([self.val[i] for i in kept])
        low = [k for k, d in value_margins(v).items() if d < 2 * TOL]
        if not low:
            return None
        m, order = len(v), np.argsort(v, kind="stable")
        lo, hi = _trim(m)
        return kept[int(order[m // 2 if low[0].startswith(("median", "std")) else lo if "lo" in low[0] else hi - 1])]

    def chosen(self, n):
        """n ordinary contigs: the first n, a weak one replaced by the next spare one until none is weak"""
        kept, spare = self.ordinary[:n], iter(self.ordinary[n:])
        while (i := self._weak(kept)) is not None:
            kept[kept.index(i)] = next(spare)
        return sorted(kept)

    def primary(self, n):
        """(reference contigs, expect) of n rows = n candidates = n kept chains"""
        return [_enc(self.seg[i]) for i in self.chosen(n)], {"rows": n, "cands": n, "m": n, "n_intervals": n}

    def subquery(self, n):
        """the query's contigs of primary(n), as a query of its own"""
        return [self.query[i] for i in self.chosen(n)]

    def _junk(self, n):
        """n random bases none of whose seeds is a seed of the query"""
        while True:
            x = _rand(self._rng, n)
            if not np.isin(sketch(self._oracle, [_enc(np.concatenate([x, x[:K]]))]).seeds["kmer"], self._seeds).any():
                return x

    def _piece(self, i):
        """a reference contig that holds 60 bases of contig i, with one or two of its seeds inside, between unrelated flanks"""
        qs = sketch(self._oracle, [self.query[i]]).seeds
        pos = np.sort(qs["pos"].astype(np.int64))
        for a in range(0, len(self.qry[i]) - 60):
            inside = int(((pos - 17 >= a + 2) & (pos - 3 < a + 58)).sum())
            near = int(((pos - 3 >= a) & (pos - 17 < a + 60)).sum())
            if 1 <= inside <= 2 and near == inside:
                return _enc(np.concatenate([self._junk(300), self.qry[i][a:a + 60], self._junk(300)]))
        raise AssertionError(f"contig {i}: no 60-base piece with one or two seeds")

    def twin(self, nc):
        """(reference contigs, expect) of nc rows, the rows of query positions 0 .. nc - 1, of which the dups and four pieces keep no chain"""
        assert all(p < nc for d, p in self.dups.items() if d < nc) and nc - 1 in self.dups
        dups = [d for d in self.dups if d < nc]
        pieces = sorted({1, 63, 256, nc - 2} & set(range(nc)))
        assert not (set(pieces) & self.special)
        while (i := self._weak([i for i in range(nc) if i not in self.dups and i not in pieces])) is not None:      # (a weak contig becomes one more piece)
            assert i not in self.special
            pieces = sorted(pieces + [i])
        ref = [_enc(self.seg[i]) if i not in pieces else self._piece(i) for i in range(nc) if i not in self.dups]
        none = sorted(dups + pieces)
        return ref, {"rows": nc, "cands": nc - len(pieces), "m": nc - len(none), "n_intervals": nc - len(none), "rows_without_chain": none}


class Case:
    def __init__(self, name):
        self.name = name
        self.refs, self.queries = [], []           # [(name, [contigs])]
        self.pairs = {}                            # pair name -> (query index, reference index)
        self.expect = {}                           # pair name -> {"rows", "cands", "m", "n_intervals"}
        self.regime = None                         # the host state the case is built for ("a" .. "d"), or None

    def ref(self, name, contigs):
        self.refs.append((name, contigs))
        return len(self.refs) - 1

    def qry(self, name, contigs):
        self.queries.append((name, contigs))
        return len(self.queries) - 1

    def pair(self, name, qi, ri, expect):
        self.pairs[name] = (qi, ri)
        self.expect[name] = expect


class Chained:
    """the oracle's account of every pair of a case's batch (the pairs that pass the screen, query-major), for one flag set"""

    def __init__(self, oracle, case, flags):
        rs = [sketch(oracle, g) for _, g in case.refs]
        self.pairs, self.res, self.rows, self.cands, self.chunks, self.pair_rows = [], {}, [], [], {}, []
        for qi, (_, g) in enumerate(case.queries):
            q = sketch(oracle, g)
            cap = capacity_rows(g) if len(q.seeds) else 0
            for ri, r in enumerate(rs):
                if not oracle.screen(q, r)[0]:
                    continue
                res = oracle.chain(r, q, **flags)
                roots, nc = oracle.last_chain_counts()
                self.pairs.append((qi, ri))
                self.res[(qi, ri)] = res
                self.rows.append(len(roots) if res.n_anchors >= MIN_ANCHORS else 0)      # (fewer anchors cannot chain: the pair gets no chunk table)
                self.cands.append(int(nc))
                self.pair_rows.append(cap)
                if res.n_chunks:
                    self.chunks[(qi, ri)] = oracle.last_chunks()

    def hits(self, qi):
        """the references the query hits, in database order, as oracle.query has them (lib.rs:654)"""
        return [ri for (q, ri) in self.pairs if q == qi and self.res[(q, ri)].ani > 0.1]


_cache = {}


def chained(oracle, case, flags=()):
    key = (case.name, tuple(sorted(dict(flags).items())))
    if key not in _cache:
        _cache[key] = Chained(oracle, case, dict(flags))
    return _cache[key]


def _shorts(rng, n_refs, n_queries):
    """short references and queries, all rescued: query i is a copy of reference i % n_refs while i < 2 n_refs, unrelated to everything after that"""
    refs = [_rand(rng, int(rng.integers(1200, 2500))) for _ in range(n_refs)]
    qs = [_mutate(rng, refs[i % n_refs], float(rng.uniform(0, 0.05))) if i < 2 * n_refs else _rand(rng, int(rng.integers(1200, 2500))) for i in range(n_queries)]
    return [[_enc(x)] for x in refs], [[_enc(x)] for x in qs]


def _tiny_cands(oracle, rng, case):
    """the tiny selection's candidate edges: (rows, candidates) = (4, 8), (4, 9), (5, 5), (1, 9). A contig of several 600-base pieces, each a copy of a
    different segment, has that many candidates in its one row; in every case one piece copies a segment that an earlier, less diverged piece copies too:
    a conflict on the reference that the later one loses."""
    segs = [_rand(rng, 600) for _ in range(12)]
    ri = case.ref("tiny_ref", [_enc(s) for s in segs])
    rs = sketch(oracle, case.refs[ri][1])

    def contig(ids, dup_last):
        return _enc(np.concatenate([_mutate(rng, segs[s], 0.08 if (dup_last and j == len(ids) - 1) else 0.004 + 0.007 * s) for j, s in enumerate(ids)]))
    layouts = {"tiny_4r8c": [[0, 1], [2, 3], [4, 5], [6, 0]], "tiny_4r9c": [[0, 1], [2, 3], [4, 5], [6, 7, 0]],
               "tiny_5r5c": [[0], [1], [2], [3], [0]], "tiny_1r9c": [[0, 1, 2, 3, 4, 5, 6, 7, 0]]}
    for name, lay in layouts.items():
        nc = sum(len(x) for x in lay)
        while True:      # (a diverged 600-base piece now and then has too few anchors for a candidate: mutate again)
            g = [contig(ids, k == len(lay) - 1) for k, ids in enumerate(lay)]
            oracle.chain(rs, sketch(oracle, g))
            if oracle.last_chain_counts()[1] == nc and all(d >= 2 * TOL for d in slip_margins(oracle.last_chunks()).values()):      # (... or two rows of one value)
                break
        qi = case.qry(name, g)
        kept_rows = len(lay) - (1 if len(lay[-1]) == 1 else 0)      # (tiny_5r5c: the last contig is nothing but the losing copy)
        case.pair(name, qi, ri, {"rows": len(lay), "cands": nc, "m": kept_rows, "n_intervals": nc - 1})


_built = {}


def cases(oracle):
    """{name: Case}; deterministic; built once per process"""
    if _built:
        return _built
    w = World(oracle, 4301, 1100, 1000, 2000)
    edge_refs = []      # (name, contigs, expect)
    for n in (1, 4, 5, 9, 10, 11, 64, 65, 512, 513, 1024, 1025):
        edge_refs.append((f"rows_{n}", *w.primary(n)))
        if n in (65, 513, 1025):
            edge_refs.append((f"rows_{n}t", *w.twin(n)))
    rng = np.random.default_rng(977)
    for reg in "abcd":
        case = Case(f"edges_{reg}")
        case.regime = reg
        if reg == "d":
            qi = case.qry("q64", w.subquery(64))
            for name, g, ex in edge_refs:
                if ex["rows"] <= 64 and not name.endswith("t") and ex["rows"] not in (9, 10, 11):
                    case.pair(name, qi, case.ref(name, g), ex)
            sr, sq = _shorts(rng, 10, 30)
        else:
            qi = case.qry("q1100", w.query)
            for name, g, ex in edge_refs:
                case.pair(name, qi, case.ref(name, g), ex)
            sr, sq = {"a": (40, 120), "b": (0, 30), "c": (0, 0)}[reg]
            sr, sq = _shorts(rng, sr, sq)
        for i, g in enumerate(sr):
            case.ref(f"sr{i}", g)
        for i, g in enumerate(sq):
            case.qry(f"sq{i}", g)
        if reg == "a":
            _tiny_cands(oracle, rng, case)
        _built[case.name] = case
    # rows 4096 / 4097 / the twin of 4097
    w2 = World(oracle, 4302, 4200, 1400, 1600)
    case = Case("big")
    qi = case.qry("q4200", w2.query)
    for n in (4096, 4097):
        g, ex = w2.primary(n)
        case.pair(f"rows_{n}", qi, case.ref(f"rows_{n}", g), ex)
    g, ex = w2.twin(4097)
    case.pair("rows_4097t", qi, case.ref("rows_4097t", g), ex)
    _built[case.name] = case
    # conflicted candidates
    case = Case("conflicts")
    rng = np.random.default_rng(31)
    z = _rand(rng, 1500)
    ri = case.ref("z", [_enc(z), _enc(_rand(rng, 1500))])
    for n in (128, 129):
        copies = [_mutate(rng, z, 0.0005 * j) for j in range(n)]
        copies[5] = copies[3].copy()                 # byte-identical: equal scores, the earlier one first
        copies[1] = copies[0].copy()                 # (rate 0: the best score twice; generation order decides which one is kept)
        case.pair(f"conflicted_{n}", case.qry(f"x{n}", [_enc(x) for x in copies]), ri, {"rows": n, "cands": n, "m": 1, "n_intervals": 1})
    g = _rand(rng, 25_000)
    long_one = _mutate(rng, g[:19_800], 0.003)
    ri = case.ref("g", [_enc(g)])
    gs, pieces = sketch(oracle, [_enc(g)]), []
    at = 300
    while len(pieces) < 70:      # (every piece carries one candidate chain of its own; a stretch of the reference with too few seeds is passed over)
        x = np.concatenate([_rand(rng, 150), _mutate(rng, g[at:at + 240], 0.003), _rand(rng, 150)])
        oracle.chain(gs, sketch(oracle, [_enc(x)]))
        ok = oracle.last_chain_counts()[1] == 1
        if ok:
            pieces.append(x)
        at += 260 if ok else 20
    assert at <= 19_700
    case.pair("carry_70", case.qry("carry", [_enc(long_one)] + [_enc(x) for x in pieces]), ri, {"rows": 71, "cands": 71, "m": 1, "n_intervals": 1})
    _built[case.name] = case
    return _built
