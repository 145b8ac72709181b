"""Genome pairs built for the decisions of the lane-per-chunk chaining DP (csrc/dp.hip chain_lane_body), and a pure-Python restatement of the chaining
rule that says which of those decisions a pair really reaches. Used by test_dp_cases_cpu.py (every case shows its event; no GPU) and
test_gpu_lane_dp.py (every case through the lane kernels, both joins).

A case is (name, reference contigs, query contigs). The events, all at c = 125 (band 20):
  tandem          a tandem repeat of six units: a query seed has six anchors, the best predecessor of a collinear one lies more than LANE_NEAR back
  indel_299/300/301   a deletion of that many bases: a gap at the MAX_GAP_LENGTH edge between neighbours of one chunk
  reach_2499/2500/2501   two neighbouring anchors that far apart on the query, gap <= MAX_GAP_LENGTH: the BP_CHAIN_BAND edge of the pair test
  break_2499/2500/2501   the same distance with a gap of ~500: the chain breaks and a new one starts while the old one's scores are still in the window
  trees_4, trees_5    one chunk of LANE_TREES / LANE_TREES + 1 qualifying trees (blocks of the reference in shuffled order)
  alternate       a segment the reference holds twice: the qualifying anchors of one chunk alternate between two trees
  tiny            contigs of 1, 2, 3 and 4 anchors behind a long one: chunks that start anywhere in the anchor array"""
import numpy as np

K = 15
FRAGMENT_LENGTH = 20000
MAX_GAP_LENGTH = 300
BP_CHAIN_BAND = 2500
ANCHOR_SCORE2 = 40
MIN_SCORE2 = 90
MIN_ANCHORS = 3
LANE_TREES = 4
LANE_NEAR = 3
LUT = np.frombuffer(b"ACGT", np.uint8)


def _enc(a):
    return LUT[a].tobytes()


def _rand(rng, n):
    return rng.integers(0, 4, n, dtype=np.uint8)


def _mutate(rng, a, d):
    b = a.copy()
    m = rng.random(len(a)) < d
    b[m] = (b[m] + rng.integers(1, 4, int(m.sum()), dtype=np.uint8)) & 3
    return b


def _seed_pos(oracle, a, c=125):
    return np.sort(oracle.Sketch([_enc(a)], c=c).seeds["pos"].astype(np.int64))


def _lonely_pair(pos, lo, hi, start):
    """seeds a < b of one sequence, lo <= b - a <= hi, with no other seed within 3 K behind a or before b, a >= start"""
    for i in range(len(pos) - 1):
        a = int(pos[i])
        if a < start or pos[i + 1] - a <= 3 * K:
            continue
        for j in range(i + 1, len(pos)):
            b = int(pos[j])
            if b - a > hi:
                break
            if b - a >= lo and b - pos[j - 1] > 3 * K:
                return a, b
    raise AssertionError("no such pair of seeds")


def _spliced(rng, g, a, b, dq):
    """g with what lies between the seeds at a and b replaced by random bases, so that the two seeds end up dq apart (their k-mers and 2 K around them stay)"""
    return np.concatenate([g[:a + 2 * K], _rand(rng, dq - 4 * K), g[b - 2 * K:]])


def cases(oracle):
    """[(name, [reference contigs], [query contigs])], bytes; deterministic"""
    rng = np.random.default_rng(8125)
    out = []
    # tandem repeat
    g = _rand(rng, 120_000)
    unit = _rand(rng, 500)
    t = np.concatenate([g[:60_000]] + [unit] * 6 + [g[60_000:]])
    out.append(("tandem", [_enc(t)], [_enc(_mutate(rng, t, 0.002))]))
    # indels at the gap edge
    g = _rand(rng, 150_000)
    for n in (299, 300, 301):
        out.append((f"indel_{n}", [_enc(g)], [_enc(np.concatenate([g[:70_000], g[70_000 + n:]]))]))
    # two neighbouring anchors at the BP_CHAIN_BAND edge: chainable (gap <= 150) / not (gap ~ 500)
    g = _rand(rng, 150_000)
    pos = _seed_pos(oracle, g)
    for kind, lo, hi in (("reach", 2350, 2450), ("break", 1950, 2050)):
        for i, dq in enumerate((2499, 2500, 2501)):
            a, b = _lonely_pair(pos, lo, hi, 50_000 + 20_000 * i)      # (mid-chunk: the chain before it has scores to leave behind)
            out.append((f"{kind}_{dq}", [_enc(g)], [_enc(_spliced(rng, g, a, b, dq))]))
    # one chunk of n qualifying trees: n blocks of the reference in shuffled order on one short contig, behind a long contig (the pair must pass the screen)
    g = _rand(rng, 200_000)
    pos = _seed_pos(oracle, g)
    for n in (LANE_TREES, LANE_TREES + 1):
        blocks = []
        at = 100_000
        while len(blocks) < n:
            if ((pos >= at + K) & (pos < at + 1500 - 2 * K)).sum() >= 5:
                blocks.append(g[at:at + 1500])
            at += 15_000 if len(blocks) % 2 else 11_000
        order = rng.permutation(n)
        while n > 1 and np.all(order == np.arange(n)):
            order = rng.permutation(n)
        short = np.concatenate([np.concatenate([blocks[int(i)], _rand(rng, 800)]) for i in order])
        out.append((f"trees_{n}", [_enc(g)], [_enc(g[:100_000]), _enc(short)]))
    # a segment held twice by the reference, once by the query
    g = _rand(rng, 150_000)
    seg = _rand(rng, 3_000)
    ref = np.concatenate([g[:60_000], seg, g[60_000:110_000], _mutate(rng, seg, 0.005), g[110_000:]])
    out.append(("alternate", [_enc(ref)], [_enc(np.concatenate([g[:60_000], seg, g[60_000:]]))]))
    # contigs of 1 .. 4 seeds behind a long one
    g = _rand(rng, 150_000)
    pos = _seed_pos(oracle, g)
    tiny = []
    ref_sk = oracle.Sketch([_enc(g)], c=125).seeds
    i = int(np.searchsorted(pos, 110_000))
    for rep in range(3):
        for n in (1, 2, 3, 4):
            while True:      # a window that holds exactly seeds i .. i + n - 1 with room around them, padded to a contig the sketcher keeps (>= 500 bases)
                lo, hi = int(pos[i]) - 2 * K, int(pos[i + n - 1]) + 2 * K
                ok = pos[i - 1] < lo - K and pos[i + n] > hi + K
                if ok:
                    piece = np.concatenate([_rand(rng, 300), g[lo:hi], _rand(rng, 300)])
                    ok = len(join(ref_sk, oracle.Sketch([_enc(piece)], c=125).seeds)[1]) == n
                i += n + 1 if ok else 1
                if ok:
                    break
            tiny.append(_enc(piece))
    out.append(("tiny", [_enc(g)], [_enc(g[:100_000])] + tiny))
    return out


# ---- the chaining rule, restated (oracle/skani_oracle.c orc_chain pass 1; csrc/dp.hip chain_chunk_serial)

def join(ref_seeds, qry_seeds):
    """the pair's anchors (qc, qp, rc, rp, rev) in the order the oracle makes them: query seeds in (contig, pos) order, each one's matches in the reference's"""
    order = np.lexsort((ref_seeds["pos"], ref_seeds["contig"], ref_seeds["kmer"]))
    rs = ref_seeds[order]
    lo = np.searchsorted(rs["kmer"], qry_seeds["kmer"], "left")
    hi = np.searchsorted(rs["kmer"], qry_seeds["kmer"], "right")
    cnt = hi - lo
    qi = np.repeat(np.arange(len(qry_seeds)), cnt)
    ri = np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)]) if len(qi) else np.zeros(0, np.int64)
    q, r = qry_seeds[qi], rs[ri.astype(np.int64)]
    return (q["contig"].astype(np.int64), q["pos"].astype(np.int64), r["contig"].astype(np.int64), r["pos"].astype(np.int64),
            (q["canon"] != r["canon"]).astype(np.int64), cnt)


class Chained:
    """what the rule makes of a pair's anchors, and what it met on the way"""

    def __init__(self, anchors, band):
        qc, qp, rc, rp, rev, _ = anchors
        n = len(qp)
        self.f = f = [0] * n
        self.root = root = list(range(n))
        self.depth = depth = [1] * n
        self.pred_dist = [0] * n            # distance to the chosen predecessor (0: a root)
        self.chunk_start = []
        self.accepted = []                  # (dq, gap) of every chosen predecessor
        self.refused_gap = set()            # gaps of pairs that passed every other test but gap <= MAX_GAP_LENGTH
        self.reached_dq = set()             # dq of every pair that got past the band-in-bases test ...
        self.broke_dq = set()               # ... and of those that ended the walk there
        self.stale = []                     # (x, f of the predecessor that was out of reach or refused) for roots that follow a high-scoring neighbour
        s = 0
        while s < n:
            e = s
            while e < n and qc[e] == qc[s] and qp[e] <= qp[s] + FRAGMENT_LENGTH:
                e += 1
            self.chunk_start.append(s)
            for x in range(s, e):
                bs, bp = ANCHOR_SCORE2, x
                y = x
                while y > s and x - (y - 1) <= band:
                    y -= 1
                    if rc[y] != rc[x] or rev[y] != rev[x]:
                        continue
                    dq = qp[x] - qp[y]
                    if dq > BP_CHAIN_BAND:
                        self.broke_dq.add(int(dq))
                        break
                    self.reached_dq.add(int(dq))
                    dr = rp[y] - rp[x] if rev[x] else rp[x] - rp[y]
                    if dq <= 0 or dr <= 0:
                        continue
                    gap = abs(dq - dr)
                    if gap > MAX_GAP_LENGTH:
                        self.refused_gap.add(int(gap))
                        continue
                    sc = f[y] + ANCHOR_SCORE2 - gap
                    if sc > bs:
                        bs, bp = sc, y
                f[x] = int(bs)
                if bp != x:
                    root[x], depth[x] = root[bp], depth[bp] + 1
                    self.pred_dist[x] = x - bp
                    self.accepted.append((int(qp[x] - qp[bp]), int(abs((qp[x] - qp[bp]) - (rp[bp] - rp[x] if rev[x] else rp[x] - rp[bp])))))
                elif x > s and f[x - 1] >= 10 * ANCHOR_SCORE2:
                    self.stale.append((x, f[x - 1]))
            s = e
        self.chunk_start.append(n)

    def chunks(self):
        return list(zip(self.chunk_start[:-1], self.chunk_start[1:]))

    def roots_per_chunk(self):
        return [sum(1 for x in range(s, e) if self.root[x] == x) for s, e in self.chunks()]

    def qualifying_roots(self, s, e):
        """roots of the chunk's anchors that the lane kernel gives a tree slot, in the order they ask: an anchor with f >= MIN_SCORE2 (its depth is >= MIN_ANCHORS)"""
        return [self.root[x] for x in range(s, e) if self.f[x] >= MIN_SCORE2]

    def candidates(self):
        n = 0
        for s, e in self.chunks():
            best = {}
            for x in range(s, e):
                b = best.get(self.root[x])
                if b is None or self.f[x] > self.f[b]:
                    best[self.root[x]] = x
            n += sum(1 for b in best.values() if self.depth[b] >= MIN_ANCHORS and self.f[b] >= MIN_SCORE2)
        return n
