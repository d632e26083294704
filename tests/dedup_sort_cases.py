"""Inputs and the numpy reference of the de-duplication and block-ranking sort tests, made on the CPU from fixed seeds: tests/test_gpu_dedup_sorts.py runs them on the
device, tests/test_dedup_sort_cases_host.py checks -- with numpy and the plain-C oracle alone -- that every case is what its name says, so that a later edit cannot turn
one into a weaker one.

The three entry points (bu_hip_k_unique_selector_vectors, bu_hip_k_unique_endpoint_vectors, bu_hip_k_map_rank_blocks) all sort through sort_pairs.h, where rocPRIM takes
one of three algorithms by the number of items: a single-block sort up to SINGLE_MAX, a merge sort up to MERGE_MAX, the one-sweep radix sort above (sort_path). The cases
sit on both sides of both switches and well inside the radix path.

Keys are computed from the blocks by the FORMAT'S definition, never by the code under test:
  selector key   sum(sel[i] << (30 - 2 i)) over the 16 selectors of etc1s_transcode_helpers.selectors_of_etc_blocks (texel i = y * 4 + x); that helper is pinned to the
                 reference by the transcoder goldens and shares nothing with k_selector_keys. The key ignores the header bytes, so they are random.
  endpoint key   clip(base - b) of r, g, b, then clip(base + b), as one 48-bit number: base = the 5-bit colour expanded to 8 bits, b = the outer modifier of the block's
                 intensity table (helpers.ETC1_INTEN_TABLES[:, 3]). The key ignores the selector bytes, so they are random.
Every block is a valid ETC1S block: differential and flip bits set, zero deltas, both table fields equal -- but for the endpoint case "second_table", which says why.

The expected outputs are numpy's: np.unique, a stable argsort, np.add.reduceat on uint64 (unique_reference); a stable argsort and np.bincount (rank_reference). All
integer work: every comparison is exact.

Nothing is built at import; every builder is cached and its result is never written to."""
import functools

import numpy as np

from etc1s_transcode_helpers import selectors_of_etc_blocks
from helpers import ETC1_INTEN_TABLES

SINGLE_MAX = 1024     # rocPRIM's single-block sort: kernel_config<256, 4> when the configuration names none (device_radix_sort.hpp)
MERGE_MAX = 32768     # sort_pairs.h's merge_sort_limit
SWITCH_N = (1024, 1025, 32768, 32769)
ONESWEEP_RADIX_BITS = 8   # rocPRIM's default_radix_sort_onesweep_config for 32-bit keys with 32-bit values on gfx950 (see rank_passes)


def sort_path(n):
    return "single" if n <= SINGLE_MAX else ("merge" if n <= MERGE_MAX else "radix")


# ----------------------------------------------------------------------------- keys by definition, and blocks with wanted keys

def etc1s_headers(color5, table):
    """(n, 3) 5-bit colours, (n,) tables -> the first four bytes of (n, 8) ETC1S blocks (differential, zero deltas, both tables the same, flipped); the rest zero"""
    color5, table = np.asarray(color5, np.int64), np.asarray(table, np.int64)
    out = np.zeros((table.size, 8), np.uint8)
    out[:, 0:3] = color5 << 3
    out[:, 3] = (table << 5) | (table << 2) | 3
    return out


def selector_keys(blocks):
    sel = selectors_of_etc_blocks(blocks).astype(np.uint32)
    return (sel << (30 - 2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint64).astype(np.uint32)


def blocks_of_selector_keys(keys, rng):
    """valid ETC1S blocks whose selector key is keys[b]: random colour and table bytes, the low 32 bits laid out as the format stores them (selector -> ETC1 pixel index
    {3, 2, 0, 1}, its LSB at bit x * 4 + y, its MSB 16 above). What comes back is checked against the definition, selector_keys."""
    keys = np.asarray(keys, np.uint32).astype(np.int64)
    n = keys.size
    out = etc1s_headers(rng.integers(0, 32, (n, 3)), rng.integers(0, 8, n))
    lo = np.zeros(n, np.int64)
    for i in range(16):
        x, y = i & 3, i >> 2
        raw = np.array([3, 2, 0, 1])[(keys >> (30 - 2 * i)) & 3]
        lo |= ((raw & 1) << (x * 4 + y)) | ((raw >> 1) << (16 + x * 4 + y))
    for k in range(4):
        out[:, 4 + k] = (lo >> (8 * (3 - k))) & 255
    assert (selector_keys(out) == keys.astype(np.uint32)).all()
    return out


def endpoint_keys_of_codes(code):
    """code = r5 << 13 | g5 << 8 | b5 << 3 | table -> the 48-bit key"""
    code = np.asarray(code, np.int64)
    c5 = np.stack([(code >> 13) & 31, (code >> 8) & 31, (code >> 3) & 31], axis=1)
    base = (c5 << 3) | (c5 >> 2)
    b = ETC1_INTEN_TABLES[code & 7, 3].astype(np.int64)[:, None]
    six = np.concatenate([np.clip(base - b, 0, 255), np.clip(base + b, 0, 255)], axis=1).astype(np.uint64)
    return (six << (8 * (5 - np.arange(6, dtype=np.uint64)))).sum(axis=1).astype(np.uint64)


def endpoint_codes(blocks):
    b = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 8).astype(np.int64)
    return ((b[:, 0] >> 3) << 13) | ((b[:, 1] >> 3) << 8) | ((b[:, 2] >> 3) << 3) | (b[:, 3] >> 5)


def endpoint_keys(blocks):
    return endpoint_keys_of_codes(endpoint_codes(blocks))


def blocks_of_endpoint_codes(code, rng):
    """valid ETC1S blocks of the given (colour5, table) codes with random selector bytes"""
    code = np.asarray(code, np.int64)
    out = etc1s_headers(np.stack([(code >> 13) & 31, (code >> 8) & 31, (code >> 3) & 31], axis=1), code & 7)
    out[:, 4:] = rng.integers(0, 256, (code.size, 4))
    assert (endpoint_codes(out) == code).all()
    return out


# ----------------------------------------------------------------------------- references

def unique_reference(keys, weights=None):
    """-> distinct keys ascending, offsets[u + 1] (offsets[u] = n), order = stable argsort (ascending block index inside a key), u64 weight sum per run (or None)"""
    keys = np.asarray(keys)
    order = np.argsort(keys, kind="stable").astype(np.uint32)
    uniq, counts = np.unique(keys, return_counts=True)
    offsets = np.zeros(uniq.size + 1, np.uint32)
    offsets[1:] = np.cumsum(counts)
    sums = None
    if weights is not None:
        w = np.asarray(weights)
        assert w.dtype == np.uint64
        sums = np.add.reduceat(w[order], offsets[:-1].astype(np.int64)) if keys.size else np.zeros(0, np.uint64)
        assert sums.dtype == np.uint64
    return uniq, offsets, order, sums


def check_groups(n, u, keys_np, got_keys, got_offsets, got_idx, weights=None, got_weights=None):
    """distinct keys ascending; blocks of every distinct vector ascending and complete; summed weights"""
    uniq, inverse = np.unique(keys_np, return_inverse=True)
    assert u == uniq.size and (got_keys[:u] == uniq).all()
    assert got_offsets[0] == 0 and got_offsets[u] == n and (np.diff(got_offsets[:u + 1].astype(np.int64)) > 0).all()
    order = np.argsort(keys_np, kind="stable")        # stable: ascending block index inside a key
    assert (got_idx == order).all()
    if weights is not None:
        assert (got_weights[:u] == np.array([weights[order[got_offsets[i]:got_offsets[i + 1]]].sum() for i in range(u)], np.uint64)).all()


def rank_reference(cluster, k):
    n = cluster.size
    order = np.argsort(cluster, kind="stable").astype(np.uint32)             # block ids grouped by cluster, ascending inside a cluster
    sizes = np.zeros(k + 1, np.uint32); sizes[:k] = np.bincount(cluster, minlength=k)
    offsets = np.zeros(k + 1, np.uint32); offsets[1:] = np.cumsum(sizes[:k])
    pos = np.zeros(n, np.uint32); pos[order] = np.arange(n, dtype=np.uint32) - offsets[cluster[order]]
    return sizes, offsets, order, pos


# ----------------------------------------------------------------------------- cases of the two unique entry points

class UniqueCase:
    """kind "selector" (32-bit keys, u64 weights given to the entry point) or "endpoint" (48-bit keys, no weights); keys = by definition from the blocks"""

    def __init__(self, kind, name, blocks, weights=None, **facts):
        self.kind, self.name = kind, name
        self.blocks = np.ascontiguousarray(blocks, np.uint8)
        self.n = self.blocks.shape[0]
        self.keys = selector_keys(self.blocks) if kind == "selector" else endpoint_keys(self.blocks)
        self.weights = None if weights is None else np.ascontiguousarray(weights, np.uint64)
        assert (self.weights is not None) == (kind == "selector") and (self.weights is None or self.weights.size == self.n)
        self.path = sort_path(self.n)
        self.facts = facts          # what the builder planted, for test_dedup_sort_cases_host.py
        for a in (self.blocks, self.keys, self.weights):
            if a is not None:
                a.setflags(write=False)

    @functools.cached_property
    def reference(self):
        return unique_reference(self.keys, self.weights)


RUN_SCALE_LONG = tuple(1 << e for e in range(17))      # 1, 2, 4, ... 65,536
RUN_SCALE_SHORT = 1000
SPECIAL_KEYS = (0x00000000, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, 0x00000001)


def _distinct_u32(rng, count, exclude=()):
    pool = np.setdiff1d(np.unique(rng.integers(0, 1 << 32, 2 * count + 64, dtype=np.uint64)), np.asarray(list(exclude), np.uint64))
    return rng.permutation(pool)[:count].astype(np.uint32)


def _selector_distinct():
    """40,000 distinct random selector words in a shuffled order, weights 1 .. 4,096: every run has length 1"""
    rng = np.random.default_rng([61, 1])
    keys = _distinct_u32(rng, 40000)
    return UniqueCase("selector", "distinct", blocks_of_selector_keys(keys, rng), rng.integers(1, 4097, keys.size).astype(np.uint64))


def _selector_one_run():
    """32,769 blocks of one selector pattern under differing header bytes; weights 2^40 + i, i = 1 .. n, so the one sum is just above 2^55 and odd: exact in u64, far
    past 32 bits, and no double at all (those are multiples of 8 up there) -- whatever order a double accumulator adds in, it ends wrong"""
    rng = np.random.default_rng([61, 2])
    n = 32769
    blocks = blocks_of_selector_keys(np.full(n, 0x9C3A61E5, np.uint32), rng)
    return UniqueCase("selector", "one_run", blocks, (np.uint64(1) << np.uint64(40)) + np.arange(1, n + 1, dtype=np.uint64))


def _selector_run_scales():
    """Runs of 1, 2, 4, ... 65,536 blocks, each length once, and 1,000 runs of 1 to 3 blocks, under random keys. The long runs are spread evenly through the key order
    (about 59 short runs between two of them) with their lengths in a seeded order, and the block order is a seeded permutation: a run starts and ends anywhere relative
    to whatever tile the run-length and keyed-reduction primitives work in, and a block's index says nothing about its run. Weights up to 2^33."""
    rng = np.random.default_rng([61, 3])
    n_runs = len(RUN_SCALE_LONG) + RUN_SCALE_SHORT
    keys = np.sort(_distinct_u32(rng, n_runs))
    lengths = rng.integers(1, 4, n_runs)
    slots = (np.arange(len(RUN_SCALE_LONG)) * (n_runs // len(RUN_SCALE_LONG)) + 29)      # where in the key order the long runs sit
    lengths[slots] = rng.permutation(np.array(RUN_SCALE_LONG))
    per_block = rng.permutation(np.repeat(keys, lengths))
    weights = rng.integers(1, 1 << 33, per_block.size, dtype=np.uint64)
    return UniqueCase("selector", "run_scales", blocks_of_selector_keys(per_block, rng), weights, long_slots=slots)


def key_bytes_pairs():
    """-> (keys, pairs): the special keys, and 60 random words each with the words that differ from it in bit 31 only, in bit 0 only, and in one (seeded) bit of each of
    its four bytes; pairs = (key, key ^ one bit) for all of those"""
    rng = np.random.default_rng([61, 4])
    base = _distinct_u32(rng, 60, exclude=SPECIAL_KEYS)
    pairs = []
    for x in base.tolist():
        flips = [31, 0] + [8 * byte + int(rng.integers(0, 8)) for byte in range(4)]
        pairs += [(x, x ^ (1 << f)) for f in flips]
    keys = np.unique(np.array(list(SPECIAL_KEYS) + [v for p in pairs for v in p], np.uint32))
    return keys, pairs


def _selector_key_bytes():
    """n = 33,000 over 408 keys that need all four key bytes (SPECIAL_KEYS and the one-bit pairs of key_bytes_pairs); the list is round after round of all the
    keys, every round in an order of its own, so every key comes about 80 times, spread over the whole list"""
    keys, _ = key_bytes_pairs()
    rng = np.random.default_rng([61, 5])
    n = 33000
    rounds = -(-n // keys.size)
    per_block = np.concatenate([rng.permutation(keys) for _ in range(rounds)])[:n]
    return UniqueCase("selector", "key_bytes", blocks_of_selector_keys(per_block, rng), rng.integers(1, 4097, n).astype(np.uint64))


def _selector_switch(n):
    """n blocks over about n / 3 distinct keys; the first and the last block are duplicates of each other"""
    rng = np.random.default_rng([61, 6, n])
    pool = _distinct_u32(rng, n // 3)
    per_block = pool[rng.integers(0, pool.size, n)]
    per_block[n - 1] = per_block[0]
    return UniqueCase("selector", f"switch_n{n}", blocks_of_selector_keys(per_block, rng), rng.integers(1, 4097, n).astype(np.uint64))


@functools.lru_cache(maxsize=None)
def endpoint_families():
    """-> (keys of all 2^18 codes, the list of families): a family = the codes (two or more) whose clamped keys coincide, found from the definition"""
    keys = endpoint_keys_of_codes(np.arange(1 << 18))
    order = np.argsort(keys, kind="stable")
    _, first, counts = np.unique(keys[order], return_index=True, return_counts=True)
    families = [order[f:f + c] for f, c in zip(first[counts > 1], counts[counts > 1])]
    keys.setflags(write=False)
    return keys, families


def _endpoint_switch(n, spread):
    """n blocks of codes drawn from 50 values (long runs) or from all 2^18 (short ones), random selector bytes"""
    rng = np.random.default_rng([62, 1, n, int(spread == "few")])
    pool = rng.permutation(1 << 18)[:50] if spread == "few" else np.arange(1 << 18)
    return UniqueCase("endpoint", f"switch_n{n}_{spread}", blocks_of_endpoint_codes(pool[rng.integers(0, pool.size, n)], rng))


def _endpoint_collisions():
    """n = 32,769 blocks only of codes whose clamped key coincides with another code's. There are 1,027 such families of 14 to 2,744 codes, 26,936 codes in all: every
    one of them, in a seeded order (so the codes of a family are interleaved with everyone else's), and the front of that list again to fill n. A rank table that
    splits a family, or merges two, shows as a wrong group count."""
    rng = np.random.default_rng([62, 2])
    _, families = endpoint_families()
    codes = rng.permutation(np.concatenate(families))
    n = 32769
    assert codes.size <= n
    return UniqueCase("endpoint", "collisions", blocks_of_endpoint_codes(np.tile(codes, 2)[:n], rng), families=len(families))


def _endpoint_random_selectors():
    """100,000 blocks of random codes under random selector bytes"""
    rng = np.random.default_rng([62, 3])
    return UniqueCase("endpoint", "random_selectors", blocks_of_endpoint_codes(rng.integers(0, 1 << 18, 100000), rng))


def _endpoint_second_table():
    """33,000 blocks of random codes whose SECOND table field (bits 4..2 of byte 3) differs from the first. No ETC1S block looks like that, and with equal fields nothing
    can tell which of the two a kernel reads; the training vector is sub-block 0's (frontend.cpp:846, get_block_low_high_colors(block_colors, 0); the oracle reads
    the same bits), so the key by definition takes the first field and ignores the second."""
    rng = np.random.default_rng([62, 4])
    n = 33000
    blocks = blocks_of_endpoint_codes(rng.integers(0, 1 << 18, n), rng)
    first = blocks[:, 3] >> 5
    second = (first + rng.integers(1, 8, n).astype(np.uint8)) & 7
    blocks[:, 3] = (first << 5) | (second << 2) | 3
    return UniqueCase("endpoint", "second_table", blocks)


_UNIQUE_BUILDERS = {("selector", "distinct"): _selector_distinct, ("selector", "one_run"): _selector_one_run, ("selector", "run_scales"): _selector_run_scales,
                    ("selector", "key_bytes"): _selector_key_bytes, ("endpoint", "collisions"): _endpoint_collisions,
                    ("endpoint", "random_selectors"): _endpoint_random_selectors, ("endpoint", "second_table"): _endpoint_second_table}
for _n in SWITCH_N:
    _UNIQUE_BUILDERS[("selector", f"switch_n{_n}")] = functools.partial(_selector_switch, _n)
    for _spread in ("few", "all"):
        _UNIQUE_BUILDERS[("endpoint", f"switch_n{_n}_{_spread}")] = functools.partial(_endpoint_switch, _n, _spread)

SELECTOR_CASES = [name for kind, name in _UNIQUE_BUILDERS if kind == "selector"]
ENDPOINT_CASES = [name for kind, name in _UNIQUE_BUILDERS if kind == "endpoint"]


@functools.lru_cache(maxsize=None)
def unique_case(kind, name):
    return _UNIQUE_BUILDERS[(kind, name)]()


# ----------------------------------------------------------------------------- cases of bu_hip_k_map_rank_blocks

class RankCase:
    def __init__(self, name, cluster, k, **facts):
        self.name, self.k = name, int(k)
        self.cluster = np.ascontiguousarray(cluster, np.uint32)
        self.n = self.cluster.size
        assert self.n and int(self.cluster.max()) < self.k
        self.path = sort_path(self.n)
        self.facts = facts
        self.cluster.setflags(write=False)

    @functools.cached_property
    def reference(self):
        return rank_reference(self.cluster, self.k)


def sort_bits(k):
    """the key bits launch_rank_blocks sorts over: ceil(log2 k), at least 1"""
    return max(1, int(k - 1).bit_length())


def rank_passes(k):
    """One-sweep passes of the sort over sort_bits(k) bits. The digit is 8 bits wide: rocprim/device/detail/config/device_radix_sort_onesweep.hpp of the installed
    rocPRIM gives gfx950, for integer keys of 3-4 bytes with values of 3-4 bytes ("Based on key_type = int, value_type = int"),
    radix_sort_onesweep_config<kernel_config<1024, 16>, kernel_config<1024, 16>, 8, block_radix_rank_algorithm::match>. So k = 200 (8 bits) is one pass,
    k = 700 (10 bits) two, k = 70,000 (17 bits) three."""
    return -(-sort_bits(k) // ONESWEEP_RADIX_BITS)


def _random_clusters(rng, n, k):
    """uniform over 0 .. k - 1, with the last cluster (the one that may need the top bit alone) and cluster 0 in use"""
    c = rng.integers(0, k, n).astype(np.uint32)
    at = rng.permutation(n)[:2]
    c[at[0]] = k - 1
    if n > 1:
        c[at[1]] = 0
    return c


def _rank_switch(n, k):
    rng = np.random.default_rng([63, 1, n, k])
    return RankCase(f"switch_n{n}_k{k}", _random_clusters(rng, n, k), k)


PASSES_K = (200, 700, 70000)


def _rank_passes(k):
    """n = 150,001 blocks, k chosen for one, two and three one-sweep passes (rank_passes states the digit width that was read)"""
    rng = np.random.default_rng([63, 2, k])
    return RankCase(f"passes_k{k}", _random_clusters(rng, 150001, k), k)


BITS_EDGE_K = (1, 2, 3, 256, 257, 65536, 65537)


def _rank_bits_edge(k):
    """n = 40,000 at the edges of the loop that turns k into a bit count. Cluster k - 1 is in use (three blocks, spread); for k = 2^b + 1 that is cluster 2^b, the only one
    that needs the top bit -- a sort one bit short files its blocks under cluster 0, in front of everything."""
    rng = np.random.default_rng([63, 3, k])
    n = 40000
    c = _random_clusters(rng, n, k)
    c[[n // 7, n // 2, n - 3]] = k - 1
    return RankCase(f"bits_k{k}", c, k)


def _rank_skew():
    """n = 100,000, k = 5,000: cluster 2,500 holds n - k + 1 blocks, every other cluster exactly one; block order is a seeded permutation"""
    rng = np.random.default_rng([63, 4])
    n, k = 100000, 5000
    c = np.concatenate([np.arange(k), np.full(n - k, k // 2)]).astype(np.uint32)
    return RankCase("skew", rng.permutation(c), k, big=k // 2)


def _rank_sparse():
    """n = 40,000, k = 100,000: at least 60,000 clusters are empty, among them all below 20,000 and all from 80,000 on"""
    rng = np.random.default_rng([63, 5])
    return RankCase("sparse", rng.integers(20000, 80000, 40000).astype(np.uint32), 100000, first=20000, last=79999)


_RANK_BUILDERS = {}
for _n in SWITCH_N:
    for _k in (37, _n):
        _RANK_BUILDERS[f"switch_n{_n}_k{_k}"] = functools.partial(_rank_switch, _n, _k)
for _k in PASSES_K:
    _RANK_BUILDERS[f"passes_k{_k}"] = functools.partial(_rank_passes, _k)
for _k in BITS_EDGE_K:
    _RANK_BUILDERS[f"bits_k{_k}"] = functools.partial(_rank_bits_edge, _k)
_RANK_BUILDERS["skew"] = _rank_skew
_RANK_BUILDERS["sparse"] = _rank_sparse

RANK_CASES = list(_RANK_BUILDERS)


@functools.lru_cache(maxsize=None)
def rank_case(name):
    return _RANK_BUILDERS[name]()
