"""Hand-made marker sets for the marker screen (csrc/screen.hip): no sequences, the markers are chosen directly, below 2^42, deterministic from a seed. Every
case is (ref_sets, query_sets, screen_val, rescue, note): lists of sorted distinct uint64 arrays. tests/test_screen_cases_cpu.py asserts on the cases themselves
what each docstring claims; tests/test_gpu_screen.py runs them through every path of the screen against tests/screen_ref.py.

  grid          43 queries x 42 references of the sizes where strides, unroll remainders and binary searches turn; every non-rescued pair shares exactly the
                smallest passing count or one fewer
  values        markers at the ends of the value range and of the inverted index's bucket table; one-marker queries, so a row is that marker's membership
  multiplicity  200 references; markers held by 1, 63, 64, 65, 127, 128, 129 and 200 of them (runs of equal keys in the inverted index)
  sliced        queries of 65 536 and 65 537 markers: the second is cut into five slices, its shared markers sit on the seams
  wide          36 864 references (+ 1) x 1 900 queries: the LDS / HBM switch of the inverted path and the sub-launch splits"""
import functools

import numpy as np

import screen_ref as R

PARAMS = (125, 1000, 15)
HALF = 0.5 ** (1.0 / 21.0)      # pow(HALF, 21) is 0.5 to within an ulp or two - which side, the rule itself decides (screen_ref.first_passing)
SIZES = (0, 1, 2, 3, 19, 20, 21, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1025)
MULTIPLICITIES = (1, 63, 64, 65, 127, 128, 129, 200)
SLICE = 16384
INV_LDS_REFS = 36 * 1024
TOP = (1 << R.MARKER_BITS) - 1


def distinct(rng, n, avoid=None):
    """n distinct random markers (unsorted), none of `avoid`"""
    got = np.zeros(0, np.uint64)
    while len(got) < n:
        draw = np.unique(rng.integers(0, 1 << R.MARKER_BITS, int(1.1 * (n - len(got))) + 16, dtype=np.uint64))
        if avoid is not None:
            draw = np.setdiff1d(draw, avoid)
        got = np.union1d(got, draw)
    return rng.permutation(got)[:n]


def as_set(*parts):
    out = np.unique(np.concatenate([np.asarray(p, np.uint64).ravel() for p in parts] + [np.zeros(0, np.uint64)]))
    assert out.size == sum(np.asarray(p).size for p in parts), "the parts of a set overlap"
    return out


# ------------------------------------------------------------------ grid
def grid_sizes():
    """(reference sizes, query sizes): every size of SIZES twice on either side; an empty reference between non-empty ones; empty queries first, in the middle, last"""
    rng = np.random.default_rng(101)
    nz = [s for s in SIZES if s]
    refs = [int(x) for x in rng.permutation(nz + nz)]
    refs[13:13] = [0]
    refs[30:30] = [0]
    qs = [int(x) for x in rng.permutation(nz + nz)]
    queries = [0] + qs[:20] + [0] + qs[20:] + [0]
    return refs, queries


@functools.lru_cache(maxsize=None)
def grid(screen_val, rescue):
    """One pool P in a fixed (random) order; a set of s markers is the first c of P and s - c markers of its own, c = first_passing(s) or one fewer. Two sets then
    share min(c, c') markers, and since first_passing grows with s that is first_passing(small) or one fewer for EVERY pair: a miscount by one, either way, in
    any cell on the wrong side flips it.
    screen_val = 1.0 gives the extra rows instead: identical sets of 19, 20, 64 and 300 markers (pow is exactly 1.0: `>` fails them all; rescue passes the 19)."""
    rng = np.random.default_rng(102)
    if screen_val == 1.0:
        sets = [np.sort(distinct(rng, n)) for n in (19, 20, 64, 300)]
        return sets, [s.copy() for s in sets] + [sets[3][:19].copy(), sets[3][:20].copy()], 1.0, rescue, "identical sets at screen_val 1.0"
    r_sizes, q_sizes = grid_sizes()
    pool = distinct(rng, max(SIZES))
    private = distinct(rng, sum(r_sizes) + sum(q_sizes), avoid=pool)
    used = 0

    def make(s):
        nonlocal used
        if s == 0:
            return np.zeros(0, np.uint64)
        c = R.first_passing(s, screen_val) - int(rng.integers(0, 2))
        assert 0 <= c <= s
        out = as_set(pool[:c], private[used:used + s - c])
        used += s - c
        return out
    return [make(s) for s in r_sizes], [make(s) for s in q_sizes], screen_val, rescue, f"grid at {screen_val:.6f}"


# ------------------------------------------------------------------ values
def _values_sets(kind, shift):
    """the sets of `values` for a bucket width of 2^shift markers; their sizes do not depend on shift"""
    nb = 1 << (R.MARKER_BITS - shift)
    width = 1 << shift
    if kind == "tiny":      # fewer than 256 markers in all: a 16-bucket table (bits = 4), one bucket of 100 entries, the last and the first occupied
        full = 5
        bucket = np.uint64(full * width) + np.arange(100, dtype=np.uint64) * np.uint64(width // 128)
        refs = [as_set(bucket),
                as_set([0, 1, width - 1, width, 2 * width - 1, (nb - 1) * width - 1, (nb - 1) * width, TOP]),
                np.zeros(0, np.uint64),
                as_set([1, width, full * width - 1, bucket[3], bucket[70], bucket[99], (full + 1) * width, TOP - 1, TOP])]
        present, absent = [bucket[3], bucket[70], bucket[99]], [bucket[3] + np.uint64(1), bucket[99] + np.uint64(1), np.uint64(9 * width + 5)]
    else:                   # one reference fills one bucket with 320 keys; the others sit at bucket edges, in the first and the last bucket, far apart
        full = nb // 3
        bucket = np.uint64(full * width) + np.arange(320, dtype=np.uint64) * np.uint64(width // 512) + np.uint64(7)
        edges = [x * width - d for x in (1, 2, full, full + 1, nb // 2, nb - 1) for d in (1, 0)]
        refs = [as_set(bucket),
                as_set([0, 1, TOP], edges),
                np.zeros(0, np.uint64),
                as_set([0, TOP - 1, TOP], edges[::2], bucket[::5]),
                as_set([2, TOP - 2], edges[1::2], bucket[1::7], [(nb - 1) * width + 77, (nb // 2) * width + 99])]
        present = [bucket[10], bucket[63], bucket[64], bucket[65], bucket[200], bucket[319]]
        absent = [bucket[10] + np.uint64(1), bucket[200] + np.uint64(1), np.uint64(full * width + 1), np.uint64((full + 1) * width - 2),      # inside the full bucket
                  np.uint64((nb // 4) * width + 3), np.uint64((nb - 2) * width + 9), np.uint64(3 * width)]                                    # in empty buckets
    held = np.unique(np.concatenate(refs))
    assert not np.isin(np.array(absent, np.uint64), held).any()
    singles = [np.array([m], np.uint64) for m in list(held[np.isin(held, refs[1])][:40]) + present + absent]
    # three markers at a threshold of one half: two shared pass, one fails - a marker counted twice shows
    a0, a1 = np.uint64(absent[0]), np.uint64(absent[1])
    triples = [as_set([present[0], a0, a1]), as_set([present[0], present[1], a0]), as_set([0, TOP, a0]), as_set([TOP - 1, TOP, a1])]
    copies = [r.copy() for r in refs if len(r)]
    union = [held.copy(), as_set(held[::3], absent)]
    empty = np.zeros(0, np.uint64)
    return refs, [empty] + singles + triples + [empty] + copies + union + [empty]


@functools.lru_cache(maxsize=None)
def values(kind="main"):
    """kind: "main" / "tiny" (marker total < 256: bits = 4) / "empty" (every reference empty: no inverted index, the lane kernel) / "empty_rescue" (the same, rescued).
    Threshold one half, no rescue: a one-marker query passes exactly the references that hold the marker."""
    if kind.startswith("empty"):
        refs = [np.zeros(0, np.uint64)] * 3
        rng = np.random.default_rng(103)
        queries = [np.zeros(0, np.uint64), np.sort(distinct(rng, 1)), np.sort(distinct(rng, 33)), np.zeros(0, np.uint64)]
        return refs, queries, HALF, kind == "empty_rescue", "every reference empty"
    refs, _ = _values_sets(kind, 30)
    bits = R.inverted_bits(sum(len(r) for r in refs))
    refs, queries = _values_sets(kind, R.MARKER_BITS - bits)
    assert R.inverted_bits(sum(len(r) for r in refs)) == bits
    return refs, queries, HALF, False, f"values ({kind}), bucket table of 2^{bits}"


# ------------------------------------------------------------------ multiplicity
@functools.lru_cache(maxsize=None)
def multiplicity():
    """200 references. Six markers are held by all of them; for every k of MULTIPLICITIES but 200 three markers are held by k consecutive references (mod 200) from
    three different starts. A query of 9 markers = four of the all-held ones, one marker of multiplicity k and four nobody holds: at a threshold of one half a
    reference passes with 5 shared of 9 and fails with 4, so the row is the marker's window - every cell sits at first_passing or one below."""
    rng = np.random.default_rng(104)
    n = 200
    everyone = distinct(rng, 6)
    windows = []      # (marker, k, start)
    taken = everyone
    for k in MULTIPLICITIES[:-1]:
        for start in (0, 37, 150):
            m = distinct(rng, 1, avoid=taken)
            taken = np.union1d(taken, m)
            windows.append((m[0], k, start))
    held = [[m for m, k, start in windows if (r - start) % n < k] for r in range(n)]
    refs = []
    for r in range(n):
        want = max(20, 6 + len(held[r])) + int(rng.integers(0, 5))
        own = distinct(rng, want - 6 - len(held[r]), avoid=taken)
        taken = np.union1d(taken, own)
        refs.append(as_set(everyone, held[r], own))
    queries = []
    for i, (m, k, start) in enumerate(windows):
        nobody = distinct(rng, 4, avoid=taken)
        taken = np.union1d(taken, nobody)
        queries.append(as_set(np.roll(everyone, i)[:4], [m], nobody))
    queries.append(as_set(everyone[:5], distinct(rng, 3, avoid=taken)))      # multiplicity 200 alone: 5 shared with everyone
    queries.append(as_set(everyone[:4], distinct(rng, 4, avoid=taken)))      # ... and 4
    queries.append(as_set(everyone, [w[0] for w in windows]))                # every pool marker: the counts differ from reference to reference
    queries.append(as_set(everyone[:2], [w[0] for w in windows[::2]], distinct(rng, 9, avoid=taken)))
    return refs, queries, HALF, False, "multiplicity"


# ------------------------------------------------------------------ sliced
@functools.lru_cache(maxsize=None)
def sliced():
    """References of 70 000, 25 and 0 markers. Queries: A, 65 537 markers (five slices, the last of one marker), shares with the large reference exactly its
    markers at the slice seams and its last one - 8, and the threshold lies between 7 and 8 of 65 537; B, 65 537 markers, shares the seams but not its last marker
    - 7; C and D, 65 536 markers (never sliced), share 8 (the seams and the first marker) and 7; a query of 10 markers, one of them in the large reference; an empty one."""
    rng = np.random.default_rng(105)
    big = np.sort(distinct(rng, 4 * 65537 + 70000 + 100))
    rng.shuffle(big)
    a, b, c, d = (np.sort(big[i * 65537:i * 65537 + n]) for i, n in enumerate((65537, 65537, 65536, 65536)))
    rest = big[4 * 65537:]
    seams = [SLICE - 1, SLICE, 2 * SLICE - 1, 2 * SLICE, 3 * SLICE - 1, 3 * SLICE, 4 * SLICE - 1]
    ten = np.sort(rest[:10])
    small_ref = np.sort(rest[10:35])
    large = as_set(a[seams], a[-1:], b[seams], c[seams], c[:1], d[seams], ten[:1], rest[35:35 + 70000 - 31])
    screen_val = (7.5 / 65537.0) ** (1.0 / 21.0)
    return [large, small_ref, np.zeros(0, np.uint64)], [a, ten, b, np.zeros(0, np.uint64), c, d], screen_val, False, "sliced"


SLICED_LARGE_QUERIES = (0, 2)      # the queries of `sliced` above 4 * SLICE markers


# ------------------------------------------------------------------ wide
@functools.lru_cache(maxsize=None)
def wide():
    """36 864 references of 20 - 24 markers in families of 64 - 130: a family has 26 markers of its own, a member holds each with probability 0.85 and fills up with
    private ones. 1 900 queries of 20 - 24 markers: about half from one family's markers, the others one each from other families - at 0.80 (the default: threshold
    0.0092) one shared marker passes, none fails, so a query passes its family, the ~85 holders of each single marker, and nothing else. A few queries are
    short (rescued: the whole row passes) or empty. Returns the case and, as sixth element, one further reference for the step past INV_LDS_REFS."""
    rng = np.random.default_rng(106)
    n = INV_LDS_REFS
    fam_sizes = []
    while sum(fam_sizes) < n:
        left = n - sum(fam_sizes)
        s = int(rng.integers(64, 131))
        if left - s < 64 and left != s:
            s = left if 64 <= left <= 130 else left - 64
        fam_sizes.append(s)
    assert sum(fam_sizes) == n and all(64 <= s <= 130 for s in fam_sizes)
    n_fam = len(fam_sizes)
    family = np.repeat(np.arange(n_fam), fam_sizes)
    sizes = rng.integers(20, 25, n + 1)
    pool = distinct(rng, 26 * n_fam + 26 * (n + 1) + 30 * 1900)
    core, own, spare = pool[:26 * n_fam].reshape(n_fam, 26), pool[26 * n_fam:26 * (n_fam + n + 1)].reshape(n + 1, 26), pool[26 * (n_fam + n + 1):]
    keep = rng.random((n + 1, 26)) < 0.85
    refs = []
    for r in range(n + 1):
        f = family[r] if r < n else 0      # (the further reference is one more member of family 0)
        mine = core[f][keep[r]][:sizes[r]]
        refs.append(as_set(mine, own[r][:sizes[r] - len(mine)]))
    queries = []
    for q in range(1900):
        if q in (0, 700, 1899):
            queries.append(np.zeros(0, np.uint64))
            continue
        size = int(rng.integers(1, 20)) if q % 97 == 5 else int(rng.integers(20, 25))
        home = int(rng.integers(0, n_fam))
        others = rng.choice(n_fam - 1, size - size // 2, replace=False)
        others = others + (others >= home)
        singles = core[others, rng.integers(0, 26, len(others))]
        n_spare = min(int(rng.integers(0, 3)), len(singles))
        queries.append(as_set(rng.permutation(core[home])[:size // 2], singles[:len(singles) - n_spare], spare[30 * q:30 * q + n_spare]))
    return refs[:n], queries, 0.80, True, "wide", refs[n]


def case(name):
    """a case by its test id"""
    if name.startswith("grid"):
        _, sv, rescue = name.split("-")
        return grid({"080": 0.80, "half": HALF, "one": 1.0}[sv], rescue == "rescue")
    if name.startswith("values"):
        return values(name.split("-")[1])
    return {"multiplicity": multiplicity, "sliced": sliced}[name]()


SMALL_CASES = [f"grid-{sv}-{r}" for sv in ("080", "half", "one") for r in ("rescue", "plain")] + ["values-main", "values-tiny", "values-empty", "values-empty_rescue", "multiplicity"]
