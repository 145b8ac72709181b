"""Inputs that put the fused small-query path (pyskani_amd/csrc/small_query.hip) exactly at, or one past, each of its fixed
capacities (SQ_* in csrc/common.h). Plain module: tests/test_small_query_edges_cpu.py checks every input's oracle count without a
GPU, tests/test_gpu_small_query_edges.py runs them through Database.query.

Every generator is deterministic: a fixed seed, plus a length or copy count found once by searching with the oracle (the search
is `search_knob` below; the constants it found are the *_KNOB values). A case is a dict:
  c, marker_c         the database's parameters
  refs                [(name, [contig, ...])]
  queries             [(name, [contig, ...], query keyword arguments)]
  path                "taken" (1,0,0), "rerun" (0,1,1) or "untried" (0,0,1): the change of psk_ctx_small_query_stats per query
  edge                (what the oracle counts, the value the input must land on): checked by the CPU test
  chunks              (chain-root cases) the chunk rows of the pair, which decide the DP's form: checked by the CPU test
"""
import numpy as np

SQ_SEEDS, SQ_MARKERS, SQ_TREES, SQ_CANDS, SQ_ROWS = 3072, 2048, 128, 256, 64
SQ_MAX_DESC, SQ_MAX_TILES, TILE_BASES, SQ_MAX_REFS, SQ_HITS_FIRST = 64, 64, 16384, 24 * 1024, 256
MIN_LENGTH_CONTIG = 500
LUT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def random_genome(rng, length):
    return LUT[rng.integers(0, 4, length)].tobytes()


def mutate(rng, seq, rate):
    a = np.frombuffer(seq, dtype=np.uint8).copy()
    m = rng.random(len(a)) < rate
    a[m] = LUT[rng.integers(0, 4, int(m.sum()))]
    return a.tobytes()


def revcomp(seq):
    return seq[::-1].translate(COMP)


def dense_unit(seed, draw, length=40):
    """the `draw`-th random unit of default_rng(seed): a period-`length` repeat of it selects a few k-mers over and over"""
    rng = np.random.default_rng(seed)
    for _ in range(draw):
        random_genome(rng, length)
    return random_genome(rng, length)


def shuffled_blocks(rng, seq, block):
    """seq cut into blocks of `block` bases, in random order: every block a chain tree of its own against seq"""
    parts = [seq[i:i + block] for i in range(0, len(seq), block)]
    order = rng.permutation(len(parts))
    return b"".join(parts[i] for i in order)


# ---------------------------------------------------------------------------------------------------------------- generators
# Each takes the knob the search tunes (a length, in bases, unless said otherwise) and returns a case.

def gen_seeds(knob):
    """query seeds: random stretch + a dense repeat trimmed to `knob` bases (c = 30, marker_c = 200: seeds > bases / c, markers few)"""
    rng = np.random.default_rng(101)
    a = random_genome(rng, 60000)
    rep = (dense_unit(1, 3) * 2000)[:knob]
    q = a[10000:22000] + rep
    refs = [("a", [a]), ("b", [mutate(rng, a, 0.02)]), ("other", [random_genome(rng, 40000)])]
    return dict(c=30, marker_c=200, refs=refs, queries=[("q", [q], {})])


def gen_markers(knob):
    """raw query markers: marker_c = c = 30, so every seed is a marker; a dense repeat trimmed to `knob` bases after a random stretch"""
    rng = np.random.default_rng(102)
    a = random_genome(rng, 60000)
    rep = (dense_unit(1, 0) * 2000)[:knob]
    q = a[5000:11000] + rep
    refs = [("a", [a]), ("b", [mutate(rng, a, 0.03)]), ("other", [random_genome(rng, 40000)])]
    return dict(c=30, marker_c=30, refs=refs, queries=[("q", [q], {})])


def gen_anchors(knob):
    """anchors of one pair: the reference "tandem" holds copies of the query's stretch, trimmed to `knob` bases (one anchor per
    copy and query seed); "plain" and "mut" are ordinary relatives that the same call must still answer correctly"""
    rng = np.random.default_rng(103)
    a = random_genome(rng, 80000)
    q = a[20000:38000]
    tandem = (q * 6)[:knob]
    refs = [("plain", [a]), ("tandem", [tandem]), ("mut", [mutate(rng, a, 0.02)])]
    return dict(c=30, marker_c=200, refs=refs, queries=[("q", [q], {})])


def gen_roots(knob, n_rows=1):
    """chain roots in one chunk: query contig 0 against a reference made of its 100-base blocks shuffled, trimmed to `knob` bases;
    `n_rows` - 1 more query contigs (one chunk each) that the reference holds plainly (few roots)"""
    rng = np.random.default_rng(104 + n_rows)
    q = [random_genome(rng, 19500)] + [random_genome(rng, 6000) for _ in range(n_rows - 1)]
    ref = shuffled_blocks(rng, q[0], 100)[:knob] + b"".join(mutate(rng, x, 0.01) for x in q[1:])
    refs = [("blocks", [ref]), ("other", [random_genome(rng, 30000)])]
    return dict(c=30, marker_c=200, refs=refs, queries=[("q", q, {})])


def gen_cands(knob):
    """candidate chains of one pair: three query contigs (three chunks, fewer than 128 roots each) against one reference of all
    their 150-base blocks shuffled, trimmed to `knob` bases"""
    rng = np.random.default_rng(108)
    q = [random_genome(rng, 19500) for _ in range(3)]
    ref = shuffled_blocks(rng, b"".join(q), 150)[:knob]
    refs = [("blocks", [ref]), ("other", [random_genome(rng, 30000)])]
    return dict(c=30, marker_c=200, refs=refs, queries=[("q", q, {})])


# the knobs the search found (search_knob): (at cap, over cap)
SEEDS_KNOB = (52379, 52391)
MARKERS_KNOB = (18366, 18380)
ANCHORS_KNOB = (93057, 93112)
ROOTS_KNOB = {1: (17625, 17725), 2: (17838, 18039), 3: (17820, 17944)}
CANDS_KNOB = (52249, 52451)


def family(rng, n_refs, length, rate=0.01):
    """an ancestor and n_refs relatives of it"""
    anc = random_genome(rng, length)
    return anc, [(f"f{j}", [mutate(rng, anc, rate * (j % 4))]) for j in range(n_refs)]


def gen_rows(m, kw=None):
    """m chunks with a chain each (m <= 64): m short contigs, or 62 short + one of 21 000 bases (two chunks) for m = 64; the
    contigs diverge by different amounts so that the per-chunk identities differ"""
    rng = np.random.default_rng(200 + m)
    anc = random_genome(rng, 120000)
    if m <= 63:
        q = [mutate(rng, anc[i * 4000:i * 4000 + 3000], 0.01 * i) for i in range(m)] if m <= 2 else \
            [mutate(rng, anc[i * 1500:i * 1500 + 900], 0.005 * (i % 7)) for i in range(m)]
    else:
        q = [mutate(rng, anc[i * 1500:i * 1500 + 700], 0.005 * (i % 7)) for i in range(62)] + [mutate(rng, anc[95000:116000], 0.01)]
    refs = [("anc", [anc]), ("mut", [mutate(rng, anc, 0.02)])]
    return dict(c=30, marker_c=200, refs=refs, queries=[(f"rows{m}", q, dict(kw or {}))])


def gen_rows_over():
    """62 short contigs + one of 40 002 bases: 65 estimated rows, never tried. The host's rows gate (rows > SQ_ROWS) cannot decide
    a query on its own: a contig's estimated rows L / 20 001 + 1 never exceed its tiles ceil(L / 16 384), so a query inside the tile
    gate has at most 64 rows. This one has 65 tiles as well, and the tile gate turns it away first."""
    rng = np.random.default_rng(265)
    anc = random_genome(rng, 140000)
    q = [anc[i * 1500:i * 1500 + 700] for i in range(62)] + [anc[95000:135002]]
    return dict(c=125, marker_c=1000, refs=[("anc", [anc])], queries=[("rows65", q, {})])


def gen_desc(n_kept, n_short=3):
    """n_kept contigs of >= 500 bases (and n_short of 499, which do not count)"""
    rng = np.random.default_rng(300 + n_kept)
    anc = random_genome(rng, 120000)
    q = [anc[i * 1800:i * 1800 + 600 + (i % 5) * 100] for i in range(n_kept)] + [anc[110000 + 600 * i:110000 + 600 * i + 499] for i in range(n_short)]
    refs = [("anc", [anc]), ("mut", [mutate(rng, anc, 0.02)])]
    return dict(c=30, marker_c=200, refs=refs, queries=[(f"desc{n_kept}", q, {})])


def gen_tiles(lengths, c=500, marker_c=1000):
    """contigs of the given lengths out of one ancestor; tiles = sum of ceil(L / 16 384)"""
    rng = np.random.default_rng(400 + len(lengths))
    total = sum(lengths)
    anc = random_genome(rng, total + 1000)
    q, off = [], 0
    for L in lengths:
        q.append(mutate(rng, anc[off:off + L], 0.01)); off += L
    refs = [("anc", [anc]), ("mut", [mutate(rng, anc, 0.03)])]
    return dict(c=c, marker_c=marker_c, refs=refs, queries=[(f"tiles{len(lengths)}_{total}", q, {})])


def gen_min_length():
    """contigs of 499 (dropped, lib.rs:156), 500 and 501 bases, alone and together"""
    rng = np.random.default_rng(500)
    anc = random_genome(rng, 60000)
    refs = [("anc", [anc]), ("mut", [mutate(rng, anc, 0.02)])]
    qs = [(f"len{L}", [anc[10000:10000 + L], anc[30000:40000]], {}) for L in (499, 500, 501)]
    qs.append(("len_all", [anc[1000:1499], anc[2000:2500], anc[3000:3501]], {}))
    return dict(c=30, marker_c=200, refs=refs, queries=qs)


def gen_refs(n_refs, dup=False):
    """n_refs small genomes (1 200 bases each, every one with seeds and markers), a family of four among them; dup: the last
    entry re-uses the name of a family member"""
    rng = np.random.default_rng(600)
    anc = random_genome(rng, 20000)
    fam = [(f"fam{j}", mutate(rng, anc, 0.01 * j)) for j in range(4)]
    bulk = random_genome(rng, 1200 * n_refs)
    refs = [(f"s{i}", [bulk[1200 * i:1200 * (i + 1)]]) for i in range(n_refs - 4 - int(dup))]
    refs[100:100] = [(n, [x]) for n, x in fam]
    if dup:
        refs.append(("fam1", [mutate(rng, anc, 0.005)]))
    return dict(c=30, marker_c=30, refs=refs, queries=[("q", [mutate(rng, anc[2000:14000], 0.01)], dict(faster_small=True))])


def gen_hits(n_hits):
    """n_hits relatives of the query's genome (and a few unrelated references): n_hits records come back"""
    rng = np.random.default_rng(700)
    anc, refs = family(rng, n_hits, 12000)
    refs += [(f"u{i}", [random_genome(rng, 12000)]) for i in range(5)]
    return dict(c=30, marker_c=200, refs=refs, queries=[(f"hits{n_hits}", [mutate(rng, anc[1000:11000], 0.01)], {})])


def gen_band(c):
    """chain band = clamp(2 500 / c, 1, 100) anchors: c = 8, 25 (100), 1 250 (2), 5 000 (1); the query as long as the seed and
    tile capacities allow"""
    rng = np.random.default_rng(800 + c)
    L = {8: 18000, 25: 60000}.get(c, SQ_MAX_TILES * TILE_BASES)
    anc = random_genome(rng, L + 20000)
    refs = [("anc", [anc]), ("mut", [mutate(rng, anc, 0.02)]), ("rc", [revcomp(mutate(rng, anc, 0.01))])]
    q = mutate(rng, anc[10000:10000 + L], 0.01)
    kws = [{}, dict(median=True), dict(robust=True)]
    return dict(c=c, marker_c=max(c * 4, 200) if c < 1000 else 2 * c, refs=refs, queries=[(f"band{c}_{i}", [q], kw) for i, kw in enumerate(kws)])


def edge_cases():
    """every edge: (id, case) with case["path"] the path each of its queries must take and, where the oracle counts the edge,
    case["edge"] = (what, value)"""
    out = []

    def add(cid, case, path, edge=None):
        case["path"] = path
        if edge:
            case["edge"] = edge
        out.append((cid, case))
    add("seeds_at_cap", gen_seeds(SEEDS_KNOB[0]), "taken", ("seeds", SQ_SEEDS))
    add("seeds_over", gen_seeds(SEEDS_KNOB[1]), "rerun", ("seeds", SQ_SEEDS + 1))
    add("markers_at_cap", gen_markers(MARKERS_KNOB[0]), "taken", ("markers", SQ_MARKERS))
    add("markers_over", gen_markers(MARKERS_KNOB[1]), "rerun", ("markers", SQ_MARKERS + 1))
    add("anchors_at_cap", gen_anchors(ANCHORS_KNOB[0]), "taken", ("anchors", SQ_SEEDS))
    add("anchors_over", gen_anchors(ANCHORS_KNOB[1]), "rerun", ("anchors", SQ_SEEDS + 1))
    for n in (1, 2, 3):
        add(f"roots{n}row_at_cap", gen_roots(ROOTS_KNOB[n][0], n), "taken", ("roots", SQ_TREES))
        add(f"roots{n}row_over", gen_roots(ROOTS_KNOB[n][1], n), "rerun", ("roots", SQ_TREES + 1))
        out[-2][1]["chunks"] = out[-1][1]["chunks"] = n      # chunk rows of the pair: team of 4, team of 2, one wave per chunk
    add("cands_at_cap", gen_cands(CANDS_KNOB[0]), "taken", ("cands", SQ_CANDS))
    add("cands_over", gen_cands(CANDS_KNOB[1]), "rerun", ("cands", SQ_CANDS + 1))
    for m in (1, 2, 10, 11, 63, 64):
        for kw in ({}, dict(median=True), dict(robust=True)):
            add(f"rows{m}_{'_'.join(kw) or 'mean'}", gen_rows(m, kw), "taken", ("valid_rows", m))
    add("rows_over", gen_rows_over(), "untried")
    add("desc_63", gen_desc(SQ_MAX_DESC - 1), "taken")
    add("desc_64", gen_desc(SQ_MAX_DESC), "untried")
    # the per-contig length gate (one contig of at most SQ_MAX_TILES * TILE_BASES bases) ...
    add("contig_at_max_length", gen_tiles([SQ_MAX_TILES * TILE_BASES]), "taken")
    add("contig_over_max_length", gen_tiles([SQ_MAX_TILES * TILE_BASES + 1]), "untried")
    # ... and the tile-count gate over several contigs, each far below that length: 31 x 2 + 2 = 64 tiles taken, 32 x 2 + 1 = 65 untried
    add("tiles_64", gen_tiles([TILE_BASES + 1] * 31 + [TILE_BASES] * 2), "taken")
    add("tiles_65", gen_tiles([TILE_BASES + 1] * 32 + [TILE_BASES]), "untried")
    add("tiles_around_one", gen_tiles([TILE_BASES - 1, TILE_BASES, TILE_BASES + 1], c=30, marker_c=200), "taken")
    add("min_length", gen_min_length(), "taken")
    add("refs_at_cap", gen_refs(SQ_MAX_REFS), "taken")
    add("refs_at_cap_dup", gen_refs(SQ_MAX_REFS, dup=True), "taken")
    add("refs_over", gen_refs(SQ_MAX_REFS + 1), "untried")
    add("hits_256", gen_hits(SQ_HITS_FIRST), "taken", ("hits", SQ_HITS_FIRST))
    add("hits_257", gen_hits(SQ_HITS_FIRST + 1), "taken", ("hits", SQ_HITS_FIRST + 1))
    for c in (8, 25, 1250, 5000):
        add(f"band_c{c}", gen_band(c), "taken")
    return out


# ---------------------------------------------------------------------------------------------------------------- fuzz
def fuzz_case(seed):
    """a random small query biased toward the fused path's edges: 1-63 contigs, lengths near 500 and near multiples of 16 384,
    repeats, reverse strands, c covering both band extremes, marker_c close to c, random query options"""
    rng = np.random.default_rng(9000 + seed)
    c = int(rng.choice([8, 20, 25, 30, 60, 125, 400, 1250, 2500]))
    marker_c = int(c * rng.choice([1, 1, 2, 4, 8]))
    budget = int(min(2200 * c, SQ_MAX_TILES * TILE_BASES, 1500 * marker_c))      # inside the host gate's expected counts
    anc = random_genome(rng, budget + 60000)
    if rng.random() < 0.3:                                                     # a repeat family in the ancestor
        unit = random_genome(rng, int(rng.integers(200, 3000)))
        pos = sorted(int(x) for x in rng.integers(0, len(anc), int(rng.integers(2, 6))))
        anc = b"".join(p + mutate(rng, unit, 0.01) for p in (anc[a:b] for a, b in zip([0] + pos, pos + [len(anc)])))
    n = int(rng.integers(1, 64)) if rng.random() < 0.5 else int(rng.integers(1, 4))
    lens = []
    for _ in range(n):
        r = rng.random()
        if r < 0.3:
            L = int(rng.integers(495, 506))
        elif r < 0.5:
            L = int(TILE_BASES * rng.integers(1, 4) + rng.integers(-3, 4))
        else:
            L = int(rng.integers(500, 40000))
        lens.append(L)
    lens[0] = max(MIN_LENGTH_CONTIG, min(lens[0], budget))
    kept = lambda: [L for L in lens if L >= MIN_LENGTH_CONTIG]
    while len(lens) > 1 and (sum(lens) > budget or sum(-(-L // TILE_BASES) for L in kept()) > SQ_MAX_TILES
                             or sum(L // 20001 + 1 for L in kept()) > SQ_ROWS):      # inside the host gate's shape limits
        lens.pop()
    q = []
    for L in lens:
        st = int(rng.integers(0, len(anc) - L))
        x = mutate(rng, anc[st:st + L], float(rng.uniform(0, 0.05)))
        q.append(revcomp(x) if rng.random() < 0.3 else x)
    refs = [(f"r{j}", [mutate(rng, anc, 0.01 * j)]) for j in range(3)]
    refs.append(("rc", [revcomp(mutate(rng, anc, 0.02))]))
    refs.append(("other", [random_genome(rng, 50000)]))
    kw = {}
    if rng.random() < 0.3:
        kw["median"] = True
    elif rng.random() < 0.3:
        kw["robust"] = True
    if rng.random() < 0.5:
        kw["faster_small"] = True
    if rng.random() < 0.3:
        kw["cutoff"] = float(rng.choice([0.7, 0.9, 0.95]))
    return dict(c=c, marker_c=marker_c, refs=refs, queries=[(f"fz{seed}", q, kw)])


# ---------------------------------------------------------------------------------------------------------------- GPU runner
PATHS = {"taken": (1, 0, 0), "rerun": (0, 1, 1), "untried": (0, 0, 1)}


def run_case(psk, O, case, expect_path=True):
    """Database.query of every query of the case, each held to the oracle and to the general path; returns
    ([path of every query], [hit tuples]) - the path asserted against case["path"] when expect_path"""
    from test_gpu_small_query import check_against_oracle, same_records, stats
    c, mc = case["c"], case["marker_c"]
    db = psk.Database(compression=c, marker_compression=mc)
    db.sketch_many([(n, *contigs) for n, contigs in case["refs"]])
    osk = [(n, O.Sketch(contigs, c=c, marker_c=mc)) for n, contigs in case["refs"]]
    paths, rows = [], []
    for qname, contigs, kw in case["queries"]:
        s0 = stats(db)
        hits = db.query(qname, *contigs, learned_ani=False, **kw)
        s1 = stats(db)
        d = tuple(b - a for a, b in zip(s0, s1))
        path = {v: k for k, v in PATHS.items()}.get(d, str(d))
        if expect_path:
            assert path == case["path"], (qname, d, case["path"])
        n = check_against_oracle(O, osk, hits, contigs, c, mc, **kw)
        if "edge" in case and case["edge"][0] == "hits":
            assert n == case["edge"][1], (qname, n)
        if "edge" in case and case["edge"][0] == "valid_rows":
            assert all(h._raw["n_chunks"] == case["edge"][1] for h in hits) and hits, (qname, [h._raw["n_chunks"] for h in hits])
        same_records(db, qname, contigs, hits, learned_ani=False, **kw)
        paths.append(path)
        for h in hits:
            r = h._raw
            rows.append((qname, h.reference_name, int(r["n_anchors"]), int(r["n_chunks"]), int(r["n_intervals"]), int(r["covered_query"]),
                         int(r["sum_chain_anchors"]), int(r["sum_chunk_seeds"]), float(r["ani"]), float(r["af_query"]), float(r["af_ref"]),
                         float(r["ani_std"])))
    return paths, rows
# ---------------------------------------------------------------------------------------------------------------- oracle counts
def oracle_count(O, what, case):
    """the count `what` of a case's first query, from the oracle"""
    c, mc = case["c"], case["marker_c"]
    qs = O.Sketch(case["queries"][0][1], c=c, marker_c=mc)
    if what == "seeds":
        return len(qs.seeds)
    if what == "markers":
        return qs.n_markers_raw
    if what in ("hits", "valid_rows"):
        osk = [(n, O.Sketch(contigs, c=c, marker_c=mc)) for n, contigs in case["refs"]]
        hits = O.query(osk, qs, **case["queries"][0][2])
        if what == "hits":
            return len(hits)
        ns = {h.n_chunks for _, h in hits}
        return ns.pop() if len(ns) == 1 else sorted(ns)
    ref = O.Sketch(_pair_ref(case), c=c, marker_c=mc)
    res = O.chain(ref, qs)
    if what == "anchors":
        return res.n_anchors
    roots, n_cands = O.last_chain_counts()
    if what == "roots":
        return int(roots.max()) if len(roots) else 0
    if what == "cands":
        return n_cands
    if what == "rows":
        return len(roots)
    raise KeyError(what)


def _pair_ref(case):
    names = [n for n, _ in case["refs"]]
    for want in ("tandem", "blocks"):
        if want in names:
            return case["refs"][names.index(want)][1]
    return case["refs"][0][1]


def search_knob(O, gen, what, target, lo, hi):
    """the smallest knob in [lo, hi] whose case lands on `target` (counts grow with the knob, about one per step)"""
    while hi - lo > 64:
        mid = (lo + hi) // 2
        if oracle_count(O, what, gen(mid)) < target:
            lo = mid
        else:
            hi = mid
    for k in range(max(0, lo - 64), hi + 64):
        if oracle_count(O, what, gen(k)) == target:
            return k
    return None
