"""No GPU: the cases of tests/dedup_sort_cases.py are what their names say, and their by-definition keys are the project's oracle's.

tests/test_gpu_dedup_sorts.py compares the device with numpy on these cases; it proves something only while the cases keep the properties they were built for (a run past
every tile, a sum past 2^53, keys that need every byte, families of colliding codes, one / two / three radix passes, the one cluster that needs the top bit ...). They are
asserted here, from the case's inputs alone, so an edit that weakens a case fails on any machine.

The keys the reference sorts are computed in dedup_sort_cases.py from the format's definition; here they are held, on every block of every case, to the plain-C oracle's
training vectors (orc_selector_training_vectors, orc_endpoint_training_vectors -- themselves pinned to the real reference in test_oracle_vs_reference.py), packed into
keys the way test_gpu_etc1s_kernels.py packs them."""
import numpy as np
import pytest

import dedup_sort_cases as D
from helpers import oracle, ptr, f32p, u64p


def _run_lengths(keys):
    return np.unique(keys, return_counts=True)[1]


# ----------------------------------------------------------------------------- the by-definition keys against the oracle

@pytest.mark.parametrize("name", D.SELECTOR_CASES)
def test_selector_keys_are_the_oracles(name):
    case = D.unique_case("selector", name)
    vec = np.zeros((case.n, 16), np.float32); w = np.zeros(case.n, np.uint64)
    oracle().orc_selector_training_vectors(ptr(case.blocks), case.n, 1, ptr(vec, f32p), ptr(w, u64p))
    assert ((vec >= 0) & (vec <= 3) & (vec == np.rint(vec))).all()
    keys = (vec.astype(np.uint32) << (30 - 2 * np.arange(16, dtype=np.uint32))).sum(axis=1).astype(np.uint32)
    bad = np.nonzero(keys != case.keys)[0]
    assert bad.size == 0, f"{name}: block {bad[0]}: by definition {case.keys[bad[0]]:#010x}, oracle {keys[bad[0]]:#010x}"


@pytest.mark.parametrize("name", D.ENDPOINT_CASES)
def test_endpoint_keys_are_the_oracles(name):
    case = D.unique_case("endpoint", name)
    vec = np.zeros((case.n, 6), np.float32)
    oracle().orc_endpoint_training_vectors(ptr(case.blocks), case.n, ptr(vec, f32p))
    bytes_ = np.rint(vec.astype(np.float64) * 255.0).astype(np.uint64)
    assert (bytes_.astype(np.float32) * np.float32(1.0 / 255.0) == vec).all()   # the float the reference stores is byte * (1/255)
    keys = (bytes_ << (8 * (5 - np.arange(6, dtype=np.uint64)))).sum(axis=1).astype(np.uint64)
    bad = np.nonzero(keys != case.keys)[0]
    assert bad.size == 0, f"{name}: block {bad[0]}: by definition {case.keys[bad[0]]:#014x}, oracle {keys[bad[0]]:#014x}"


@pytest.mark.parametrize("kind,name", [("selector", n) for n in D.SELECTOR_CASES] + [("endpoint", n) for n in D.ENDPOINT_CASES])
def test_blocks_are_valid_etc1s(kind, name):
    """differential and flip bits set, zero deltas, both table fields equal -- and the bytes the key must ignore are not constant"""
    b = D.unique_case(kind, name).blocks
    assert (b[:, 0:3] & 7 == 0).all() and (b[:, 3] & 3 == 3).all()
    if (kind, name) == ("endpoint", "second_table"):       # the one case that is no ETC1S: the second table field differs everywhere, and takes every value
        assert ((b[:, 3] >> 5) != ((b[:, 3] >> 2) & 7)).all() and np.unique((b[:, 3] >> 2) & 7).size == 8
        assert (D.endpoint_keys(b) != D.endpoint_keys_of_codes((D.endpoint_codes(b) & ~7) | ((b[:, 3] >> 2) & 7))).mean() > 0.9    # reading it gives other keys
    else:
        assert ((b[:, 3] >> 5) == ((b[:, 3] >> 2) & 7)).all()
    ignored = b[:, 0:4] if kind == "selector" else b[:, 4:8]
    assert all(np.unique(ignored[:, c]).size >= 8 for c in range(4))


def test_the_reference_on_a_list_worked_by_hand():
    keys = np.array([7, 3, 7, 7, 0xFFFFFFFF, 3], np.uint32)
    w = np.array([1, 2, 1 << 40, 4, 5, (1 << 63) + 1], np.uint64)
    uniq, offsets, order, sums = D.unique_reference(keys, w)
    assert uniq.tolist() == [3, 7, 0xFFFFFFFF] and offsets.tolist() == [0, 2, 5, 6] and order.tolist() == [1, 5, 0, 2, 3, 4]
    assert [int(s) for s in sums] == [(1 << 63) + 3, (1 << 40) + 5, 5]
    D.check_groups(6, 3, keys, uniq, offsets, order, w, sums)
    sizes, offs, order, pos = D.rank_reference(np.array([2, 0, 2, 4, 0], np.uint32), 6)
    assert sizes.tolist() == [2, 0, 2, 0, 1, 0, 0] and offs.tolist() == [0, 2, 2, 4, 4, 5, 5] and order.tolist() == [1, 4, 0, 2, 3] and pos.tolist() == [0, 0, 1, 0, 1]


# ----------------------------------------------------------------------------- selector cases

def test_sort_paths():
    """both sides of both switches, for every entry point, and every large case on the radix path"""
    assert [D.sort_path(n) for n in D.SWITCH_N] == ["single", "merge", "merge", "radix"]
    for kind, names in (("selector", D.SELECTOR_CASES), ("endpoint", D.ENDPOINT_CASES)):
        for name in names:
            case = D.unique_case(kind, name)
            assert case.path == "radix" or name.startswith("switch_n"), name
        assert {D.unique_case(kind, n).n for n in names if n.startswith("switch_n")} == set(D.SWITCH_N)
    assert {D.rank_case(n).n for n in D.RANK_CASES if n.startswith("switch_n")} == set(D.SWITCH_N)
    assert all(D.rank_case(n).path == "radix" for n in D.RANK_CASES if not n.startswith("switch_n"))
    assert max(D.rank_case(n).n for n in D.RANK_CASES) == 150001 >= max(D.unique_case(k, n).n for k, names in (("selector", D.SELECTOR_CASES), ("endpoint", D.ENDPOINT_CASES)) for n in names)


def test_selector_distinct():
    case = D.unique_case("selector", "distinct")
    assert case.n == 40000 and np.unique(case.keys).size == 40000
    assert (np.diff(case.keys.astype(np.int64)) < 0).sum() > 15000          # shuffled, not sorted
    assert case.weights.min() >= 1 and case.weights.max() <= 4096
    assert all(np.unique((case.keys >> (8 * byte)) & 255).size == 256 for byte in range(4))


def test_selector_one_run():
    case = D.unique_case("selector", "one_run")
    assert case.n == 32769 and np.unique(case.keys).size == 1
    assert np.unique(case.blocks[:, :4], axis=0).shape[0] > 10000           # differing header bytes
    total = sum(int(w) for w in case.weights)
    assert 2 ** 53 < total < 2 ** 63
    assert int(case.reference[3][0]) == total
    assert (case.weights == 2 ** 40 + np.arange(1, case.n + 1, dtype=np.uint64)).all()
    assert total > 2 ** 55 and total % 2 == 1 and int(float(total)) != total   # no double holds it, so a double accumulator is wrong in any order of addition
    assert int(case.weights.astype(np.float64).sum()) != total              # (numpy's pairwise sum in double, for one)
    assert total % 2 ** 32 != total                                          # a 32-bit accumulator


def test_selector_run_scales():
    case = D.unique_case("selector", "run_scales")
    uniq, counts = np.unique(case.keys, return_counts=True)
    assert uniq.size == len(D.RUN_SCALE_LONG) + D.RUN_SCALE_SHORT
    long_at = np.nonzero(counts > 3)[0]
    assert sorted(counts[case.facts["long_slots"]].tolist()) == list(D.RUN_SCALE_LONG)      # every length 1, 2, 4 ... 65,536 once
    short = np.delete(counts, case.facts["long_slots"])
    assert short.size == D.RUN_SCALE_SHORT and set(short.tolist()) == {1, 2, 3}
    assert case.n == int(counts.sum()) and case.path == "radix"
    assert (np.diff(long_at) >= 50).all()                                    # short runs between any two long ones, in key order
    big = counts[long_at]
    assert (np.diff(big) > 0).any() and (np.diff(big) < 0).any()             # lengths not monotone in key order
    # block order says nothing about the run: the blocks of the longest run are spread over the whole list
    at = np.nonzero(case.keys == uniq[np.argmax(counts)])[0]
    assert at[0] < 20 and at[-1] > case.n - 20 and np.diff(at).max() < 40
    # run starts relative to a tile of 256 .. 16,384 items: many different remainders
    starts = case.reference[1][:-1].astype(np.int64)
    for tile in (256, 1024, 4096, 16384):
        assert np.unique(starts % tile).size >= min(tile, starts.size) // 4
    assert int(case.reference[3].max()) > 2 ** 32


def test_selector_key_bytes():
    case = D.unique_case("selector", "key_bytes")
    keys, pairs = D.key_bytes_pairs()
    assert case.n == 33000 and case.path == "radix"
    present = set(np.unique(case.keys).tolist())
    assert present == set(keys.tolist())
    assert all(k in present for k in D.SPECIAL_KEYS)
    flips = {a ^ b for a, b in pairs}
    assert all(a in present and b in present and bin(a ^ b).count("1") == 1 for a, b in pairs)
    assert {1 << 31, 1} <= flips and all(any((1 << (8 * byte + j)) in flips for j in range(8)) for byte in range(4))
    for k in keys:          # several times, far apart
        at = np.nonzero(case.keys == k)[0]
        assert at.size >= 70 and at[-1] - at[0] > case.n * 9 // 10


@pytest.mark.parametrize("n", D.SWITCH_N)
def test_selector_switch(n):
    case = D.unique_case("selector", f"switch_n{n}")
    u = np.unique(case.keys).size
    assert case.n == n and n // 4 < u <= n // 3
    assert case.keys[0] == case.keys[-1] and (case.blocks[0] != case.blocks[-1]).any()
    assert _run_lengths(case.keys).max() >= 4


# ----------------------------------------------------------------------------- endpoint cases

def test_endpoint_families():
    keys, families = D.endpoint_families()
    assert np.unique(keys).size == 236235                                    # test_host_logic.py::test_endpoint_codebook_can_never_reach_the_threaded_gate
    assert sum(f.size - 1 for f in families) == (1 << 18) - 236235
    assert all(f.size >= 2 and np.unique(keys[f]).size == 1 for f in families)


@pytest.mark.parametrize("n", D.SWITCH_N)
def test_endpoint_switch(n):
    few, every = D.unique_case("endpoint", f"switch_n{n}_few"), D.unique_case("endpoint", f"switch_n{n}_all")
    assert few.n == n == every.n
    assert np.unique(D.endpoint_codes(few.blocks)).size == 50 and _run_lengths(few.keys).min() >= n // 50 // 3
    assert np.unique(D.endpoint_codes(every.blocks)).size > n * 0.9 and (_run_lengths(every.keys) == 1).mean() > 0.8


def test_endpoint_collisions():
    case = D.unique_case("endpoint", "collisions")
    all_keys, families = D.endpoint_families()
    assert case.n == 32769 and case.path == "radix"
    codes = D.endpoint_codes(case.blocks)
    used_codes = np.unique(codes)
    fam_keys, members = np.unique(all_keys[used_codes], return_counts=True)
    assert fam_keys.size == case.facts["families"] == 1027 >= 100
    assert (members >= 2).all()                                              # only multi-code families, two codes and more of each present
    # every family is complete: a code of the family that is missing from the list could hide a split
    assert used_codes.size == sum(f.size for f in families) == (1 << 18) - 236235 + 1027
    # interleaved: blocks of one family are seldom neighbours (the largest family is a tenth of the list), and the different codes of a family lie far apart
    assert (case.keys[1:] == case.keys[:-1]).mean() < 0.03
    for k in fam_keys[::20]:
        at = np.nonzero(case.keys == k)[0]
        assert np.unique(codes[at]).size >= 2 and at[-1] - at[0] > 10000
    assert np.unique(case.keys).size == fam_keys.size


def test_endpoint_random_selectors():
    case = D.unique_case("endpoint", "random_selectors")
    assert case.n == 100000
    assert np.unique(case.blocks[:, 4:], axis=0).shape[0] > 99000
    u = np.unique(case.keys).size
    assert u < np.unique(D.endpoint_codes(case.blocks)).size <= case.n       # some blocks share a key under different codes
    assert all(np.unique((case.keys >> np.uint64(8 * byte)) & np.uint64(255)).size >= 64 for byte in range(6))


# ----------------------------------------------------------------------------- rank cases

@pytest.mark.parametrize("n", D.SWITCH_N)
def test_rank_switch(n):
    small, full = D.rank_case(f"switch_n{n}_k37"), D.rank_case(f"switch_n{n}_k{n}")
    assert small.n == n == full.n and small.k == 37 and full.k == n
    assert np.unique(small.cluster).size == 37
    sizes = np.bincount(full.cluster, minlength=n)
    assert (sizes == 0).sum() > n // 4 and (sizes > 1).sum() > n // 8 and sizes[0] and sizes[n - 1]


def test_rank_passes():
    """one, two and three passes of 8 bits (D.rank_passes names the header and the line the width was read from)"""
    assert D.ONESWEEP_RADIX_BITS == 8
    assert [D.sort_bits(k) for k in (1, 2, 3, 4, 5, 256, 257, 65536, 65537)] == [1, 1, 2, 2, 3, 8, 9, 16, 17]
    assert [D.rank_passes(k) for k in D.PASSES_K] == [1, 2, 3]
    for k in D.PASSES_K:
        case = D.rank_case(f"passes_k{k}")
        assert case.n == 150001 and case.k == k and case.path == "radix"
        top = 1 << (D.sort_bits(k) - 1)
        assert (case.cluster >= top).sum() > 100 and (case.cluster == k - 1).any()      # the last pass has work to do


@pytest.mark.parametrize("k", D.BITS_EDGE_K)
def test_rank_bits_edges(k):
    case = D.rank_case(f"bits_k{k}")
    assert case.n == 40000 and case.k == k
    last = np.nonzero(case.cluster == k - 1)[0]
    assert last.size >= 3
    if k > 2 and (k - 1) & (k - 2) == 0:            # k = 2^b + 1: cluster 2^b alone needs the top bit, and a sort without that bit gives another order
        top = D.sort_bits(k) - 1
        assert D.sort_bits(k) == D.sort_bits(k - 1) + 1 and k - 1 == 1 << top
        assert (case.cluster >> top).sum() == last.size
        short = np.argsort(case.cluster & np.uint32((1 << top) - 1), kind="stable")
        assert (short != case.reference[2]).sum() > 100
    if k > 1:
        assert np.unique(case.cluster).size > min(k, 40000) // 3


def test_rank_skew():
    case = D.rank_case("skew")
    sizes = np.bincount(case.cluster, minlength=case.k)
    assert case.n == 100000 and case.k == 5000 and case.facts["big"] == 2500
    assert sizes[2500] == case.n - case.k + 1 and (np.delete(sizes, 2500) == 1).all()
    at = np.nonzero(case.cluster != 2500)[0]
    assert at[0] < 200 and at[-1] > case.n - 200                             # the single blocks are spread through the list


def test_rank_sparse():
    case = D.rank_case("sparse")
    sizes = np.bincount(case.cluster, minlength=case.k)
    assert case.n == 40000 and case.k == 100000
    assert (sizes == 0).sum() >= 60000 and not sizes[:20000].any() and not sizes[80000:].any()
    assert sizes[20000:80000].max() >= 3
