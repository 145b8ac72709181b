"""CPU: the locality order's C-ABI surface, and a pure-numpy statement of its grouping rule (what tests/test_gpu_locality.py holds the GPU's order to).

The rule (csrc/locality.hip): a reference's first S = 128 markers (they are stored sorted and unique: a bottom-s min-hash) are gathered with the reference's index;
for every marker, the references that hold it among their bottom markers, in ascending index - each of them but the first makes one edge (first holder, itself);
two references are linked when at least T = 3 markers made an edge of them; groups = connected components; the order = stable sort of the references by
(smallest index of their group, own index)."""
import collections
import os
import re

import numpy as np

from conftest import ROOT

S, T = 128, 3


def locality_order(marker_sets, s=S, t=T):
    """marker_sets: one sorted array of distinct markers per reference -> (slot_of, n_groups)"""
    n = len(marker_sets)
    holders = collections.defaultdict(list)
    for r, m in enumerate(marker_sets):
        for x in np.asarray(m)[:s].tolist():
            holders[x].append(r)
    edges = collections.Counter()
    for rs in holders.values():
        for r in rs[1:]:
            edges[(rs[0], r)] += 1
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for (a, b), c in edges.items():
        if c >= t:
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    label = [find(r) for r in range(n)]
    ref_of = sorted(range(n), key=lambda r: (label[r], r))
    slot_of = np.empty(n, np.uint32)
    slot_of[ref_of] = np.arange(n, dtype=np.uint32)
    return slot_of, len(set(label))


def _families(rng, n_fam, n_mem, n_markers=400, keep=0.7):
    """marker sets of n_fam families: every member keeps `keep` of its family's markers and adds markers of its own"""
    fam_of, sets = [], []
    anc = [np.unique(rng.integers(0, 1 << 42, n_markers, dtype=np.uint64)) for _ in range(n_fam)]
    for f in range(n_fam):
        for _ in range(n_mem):
            own = rng.integers(0, 1 << 42, int(n_markers * (1 - keep)), dtype=np.uint64)
            sets.append(np.unique(np.concatenate([anc[f][rng.random(len(anc[f])) < keep], own])))
            fam_of.append(f)
    return fam_of, sets


def test_rule_puts_shuffled_families_in_contiguous_runs_and_keeps_a_local_layout():
    rng = np.random.default_rng(5)
    fam_of, sets = _families(rng, 7, 30)
    slot_of, groups = locality_order(sets)
    assert groups == 7 and (slot_of == np.arange(len(sets))).all()      # family by family: the identity
    perm = rng.permutation(len(sets))
    slot_of, groups = locality_order([sets[i] for i in perm])
    fam = np.array(fam_of)[perm]
    assert groups == 7 and sorted(slot_of.tolist()) == list(range(len(sets)))
    for f in range(7):
        mine = np.flatnonzero(fam == f)
        sl = slot_of[mine]
        assert sl.max() - sl.min() + 1 == len(mine)        # one contiguous run of slots
        assert (np.diff(sl) > 0).all()                      # inside a group: insertion order
    firsts = [np.flatnonzero(fam == f)[0] for f in range(7)]
    assert [int(slot_of[i]) for i in sorted(firsts)] == sorted(int(slot_of[i]) for i in firsts)      # groups in the order of their first members


def test_rule_does_not_link_on_one_or_two_shared_markers_and_leaves_singletons_in_place():
    rng = np.random.default_rng(6)
    a = np.unique(rng.integers(0, 1 << 42, 300, dtype=np.uint64))
    b = np.unique(rng.integers(0, 1 << 42, 300, dtype=np.uint64))
    b2 = np.unique(np.concatenate([b, a[:2]]))      # two of a's smallest markers: chance, not kinship
    slot_of, groups = locality_order([a, b2, a.copy(), np.zeros(0, np.uint64)])
    assert groups == 3 and slot_of.tolist() == [0, 2, 1, 3]
    b3 = np.unique(np.concatenate([b, a[:3]]))
    assert locality_order([a, b3])[1] == 1


def test_header_binding_and_null_database():
    import ctypes as C
    from pyskani_amd import _capi
    header = open(os.path.join(ROOT, "include", "pyskani_amd.h")).read()
    assert re.search(r"psk_status psk_db_locality\(psk_db\* db, uint32_t\* slot_of, uint32_t\* n_groups, uint32_t\* is_identity\);", header)
    assert int(re.search(r"#define PSK_ABI_VERSION (\d+)", header).group(1)) == 7 == _capi.ABI_VERSION
    lib = _capi.load()
    assert lib.psk_abi_version() == 7
    g, ident = C.c_uint32(7), C.c_uint32(7)
    assert lib.psk_db_locality(None, None, C.byref(g), C.byref(ident)) == _capi.PSK_EINVAL      # (before any lane or device is touched)
    assert (g.value, ident.value) == (7, 7)
