"""CPU: the bucket rule of the blocked seed index (psk_bsi_plan, csrc/seed_index.hip; no GPU is touched). bits0 = about 8 entries per bucket of the largest
block (at most 24 bits, at most 2k); a tagged index has max(bits0, 2k - 8) bits, so that the k-mer bits below the bucket fit the entries' tag byte; the index
is tagged when $PSK_BSI_TAG forces it, or - unless forbidden - when its bucket tables are no larger than the key array the walks stop reading."""
import ctypes as C

import pytest

from pyskani_amd import _capi

DEFAULT, FORBID, FORCE = -1, 0, 1


def plan(k, max_block, n_blocks, n_entries, mode=DEFAULT):
    lib = _capi.load()
    bits, tagged = C.c_int(-1), C.c_int(-1)
    lib.psk_bsi_plan(k, max_block, n_blocks, n_entries, mode, C.byref(bits), C.byref(tagged))
    return bits.value, tagged.value


def bits0(k, max_block):
    b = 4
    while b < 24 and (8 << b) < max_block:
        b += 1
    return min(b, 2 * k)


def blocks(n_refs):
    return (n_refs + 255) // 256


# seeds per genome = bases / c at c = 125
CONTRACT = dict(k=15, max_block=256 * 40_000, n_blocks=blocks(10_000), n_entries=10_000 * 40_000)
AVA_1K = dict(k=15, max_block=256 * 40_000, n_blocks=blocks(1_000), n_entries=1_000 * 40_000)
META_100K = dict(k=15, max_block=256 * 133_000, n_blocks=blocks(100_000), n_entries=100_000 * 133_000)      # c = 30: bits0 = 23
SMALL = dict(k=15, max_block=256 * 2_500, n_blocks=blocks(320), n_entries=320 * 2_500)                      # a few hundred small genomes (the tests)


def test_the_projects_shapes():
    assert bits0(15, CONTRACT["max_block"]) == 21
    assert plan(**CONTRACT) == (22, 1)
    nb = CONTRACT["n_blocks"] * ((1 << 22) + 1) * 4
    assert 670e6 < nb < 672e6 and 4 * CONTRACT["n_entries"] == 1.6e9      # the bucket tables against the key array
    assert plan(**AVA_1K) == (22, 1)
    assert bits0(15, META_100K["max_block"]) == 23
    assert plan(**META_100K) == (23, 1)                                    # already fine enough: the buckets do not change
    assert plan(**SMALL) == (bits0(15, SMALL["max_block"]), 0) and bits0(15, SMALL["max_block"]) < 22


@pytest.mark.parametrize("shape", [CONTRACT, AVA_1K, META_100K, SMALL])
def test_forbid_and_force(shape):
    b0 = bits0(shape["k"], shape["max_block"])
    assert plan(mode=FORBID, **shape) == (b0, 0)                           # today's index
    assert plan(mode=FORCE, **shape) == (max(b0, 2 * shape["k"] - 8), 1)


def test_k16_is_tagged_only_when_forced_or_the_blocks_are_large():
    # 32-bit k-mers: 24-bit bucket tables, 64 MB per block - more than the keys of a block of 256 x 40 000 seeds (41 MB)
    assert plan(16, 256 * 40_000, 40, 10_000 * 40_000) == (21, 0)
    assert plan(16, 256 * 40_000, 40, 10_000 * 40_000, FORCE) == (24, 1)
    assert plan(16, 256 * 40_000, 40, 10_000 * 40_000, FORBID) == (21, 0)
    # blocks of 256 x 80 000 seeds: 82 MB of keys per block
    assert plan(16, 256 * 80_000, 40, 40 * 256 * 80_000) == (24, 1)
    # exactly at the rule's edge: n_blocks * (2^24 + 1) entries, and one fewer
    edge = 40 * ((1 << 24) + 1)
    assert plan(16, 256 * 80_000, 40, edge) == (24, 1)
    assert plan(16, 256 * 80_000, 40, edge - 1) == (bits0(16, 256 * 80_000), 0)


def test_k14():
    assert plan(14, 256 * 40_000, 40, 10_000 * 40_000) == (21, 1)          # bits0 = 21 > 2k - 8 = 20: the buckets do not change
    assert plan(14, 256 * 2_500, 2, 320 * 2_500, FORCE) == (20, 1)
    assert plan(14, 256 * 2_500, 2, 320 * 2_500) == (bits0(14, 256 * 2_500), 0)
    assert plan(14, 256 * 2_500, 2, 2 * ((1 << 20) + 1)) == (20, 1)


def test_tagged_implies_the_low_bits_fit_the_tag_byte():
    for k in range(8, 17):
        for max_block in (1, 1000, 1 << 17, 1 << 22, 1 << 27, (1 << 31) - 257):
            for n_blocks in (1, 3, 400):
                for mode in (DEFAULT, FORBID, FORCE):
                    bits, tagged = plan(k, max_block, n_blocks, max_block * n_blocks, mode)
                    assert 0 < bits <= 2 * k and bits <= 24
                    if tagged:
                        assert 2 * k - bits <= 8, (k, max_block, n_blocks, mode)
                    else:
                        assert bits == bits0(k, max_block)
                    assert tagged == 1 if mode == FORCE else True
                    assert tagged == 0 if mode == FORBID else True
