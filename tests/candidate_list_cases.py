"""Seeded inputs for the kernels that walk a candidate list or a member list in fixed-size pieces, with lists well past one piece: refine_endpoint_clusterization
(rounds of RQ = 256 candidates per queue), find_optimal_selector_clusters (lists of FOSC_QUAD_MIN = 384 and more take the quad tables) and
create_optimized_selector_codebook (waves take COSC_CHUNK = 128 consecutive CSR members). CPU only. Every case is a dict of read-only arrays that includes the oracle's
output, built once per process (lru_cache): the GPU tests share one oracle run across their parametrisations.

The numpy restatements (refine_errors, unclamped, fosc_errors, texel_errors, cosc_totals) only COUNT conditions in tests/test_candidate_list_cases_host.py and word the
failure messages of tests/test_gpu_candidate_lists.py; the expected value of every GPU test is the oracle's."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import helpers as H
from helpers import oracle, ptr, u32p, csr_from_lists

RQ = 256              # etc1s_refine_kernels.hip: candidates per round
FOSC_QUAD_MIN = 384   # etc1s_selector_kernels.hip: list length from which the quad tables are built
COSC_CHUNK = 128      # etc1s_selector_kernels.hip: CSR members per wave and step
MASKED = np.iinfo(np.int64).max   # the oracle's error of an entry whose table is above the block's

REFINE_KINDS = ("flat", "hier", "foreign")
REFINE_LISTS = ("long", "t0_255_257", "t0_256_256", "t0_257_255", "u64_c1", "single", "empty", "table7")
T0_COUNTS = {"t0_255_257": (255, 257), "t0_256_256": (256, 256), "t0_257_255": (257, 255)}
# the group of a block (refine cases): what its current cluster was set to
GROUPS = ("none", "later member of a pair inside round 0", "later member of a pair across rounds", "later copy of an exact planted endpoint")
SLOTS = 58            # list positions 0..57: copies of entries of positions 58..255 (the fitted codebook), so both members of such a pair lie in round 0
LONG = 1900           # the long list = clusters 0..LONG-1, so a position in it is a cluster index and the flat case sees the same positions
FOSC_LENS = (383, 384, 385, 447, 700, 64, 1, 0)
FOSC_SPACINGS = (1, 64, 320)


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ----------------------------------------------------------------------------- numpy restatements (counting only)

def unclamped(params):
    """base_unclamped of etc1s_device.h over (K, 4) {r5, g5, b5, table}: none of the entry's four colours is clamped"""
    p = np.asarray(params)
    return H.etc1s_clamp_class(p[:, :3], p[:, 3]) == 0


def _entry_colours(c5, table):
    """(..., 3) colour5, (...) table -> (..., 4, 3) int32: the four colours, clamped"""
    c5 = np.asarray(c5, np.int32)
    base = (c5 << 3) | (c5 >> 2)
    return np.clip(base[..., None, :] + H.ETC1_INTEN_TABLES[np.asarray(table, np.int64)][..., :, None], 0, 255).astype(np.int32)


def _metric_axes(rgb, perceptual):
    """(..., 3) int32 colours -> three int32 arrays whose differences are what orc_color_distance squares"""
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    if not perceptual:
        return r, g, b
    l = r * 14 + g * 45 + b * 5
    return l, r * 64 - l, b * 64 - l


def _distance(perceptual, d0, d1, d2):
    """orc_color_distance from the three differences of _metric_axes (int32: every intermediate stays below 2^31)"""
    if not perceptual:
        return d0 * d0 + d1 * d1 + d2 * d2
    return ((d0 * d0) >> 5) + ((((d1 * d1) >> 5) * 26) >> 7) + ((((d2 * d2) >> 5) * 3) >> 7)


def _refine_errors_raw(tiles, params, perceptual):
    n, k = tiles.shape[0], params.shape[0]
    px = _metric_axes(tiles[..., :3].reshape(n, 16, 3).astype(np.int32), perceptual)
    col = _metric_axes(_entry_colours(params[:, :3], params[:, 3]), perceptual)          # 3 x (k, 4)
    out = np.empty((n, k), np.uint32)
    step = 32

    def work(k0):
        d = [p[:, None, :, None] - c[None, k0:k0 + step, None, :] for p, c in zip(px, col)]   # (n, step, 16, 4)
        out[:, k0:k0 + step] = _distance(perceptual, *d).min(axis=3).sum(axis=2)

    with ThreadPoolExecutor(8) as pool:
        list(pool.map(work, range(0, k, step)))
    return out


def refine_errors(tiles, params, perceptual, block_cluster=None):
    """(n, K) int64 block errors by the definition in orc_refine_endpoint_clusterization: per block and entry the sum over 16 texels of the minimum over the entry's four
    colours of orc_color_distance. With block_cluster, entries whose table is above the table of the block's current cluster are MASKED."""
    err = _refine_errors_raw(np.asarray(tiles), np.asarray(params), int(perceptual)).astype(np.int64)
    if block_cluster is not None:
        table = np.asarray(params)[:, 3].astype(np.int64)
        err[table[None, :] > table[np.asarray(block_cluster)][:, None]] = MASKED
    return err


def refine_winners(err, block_cluster, lists, block_list):
    """The winner rule over masked errors: first minimum in list order; the current cluster wins non-zero ties; the first zero ends the scan; no admissible entry: 0.
    lists: per list the cluster indices in list order; block_list: the list of every block."""
    out = np.zeros(err.shape[0], np.uint32)
    for li, members in enumerate(lists):
        blocks = np.nonzero(block_list == li)[0]
        if not blocks.size or not len(members):
            continue
        members = np.asarray(members, np.int64)
        sub = err[np.ix_(blocks, members)]
        first = sub.argmin(axis=1)
        m = sub[np.arange(blocks.size), first]
        win = members[first]
        cur = np.asarray(block_cluster, np.int64)[blocks]
        cur_in = (members[None, :] == cur[:, None]).any(axis=1)
        cur_ties = cur_in & (err[blocks, cur] == m) & (m != 0)
        win = np.where(cur_ties, cur, win)
        out[blocks] = np.where(m == MASKED, 0, win)
    return out


def selector_word(sel8):
    """(k, 8) selector blocks -> (k,) the 32 selector bits (bytes 4-7, big endian)"""
    b = np.asarray(sel8, np.uint8).astype(np.uint32)
    return (b[:, 4] << 24) | (b[:, 5] << 16) | (b[:, 6] << 8) | b[:, 7]


def word_selectors(words):
    """(k,) selector words -> (k, 16) selectors of texel p = y * 4 + x (etc.h:232-236, as unpack_etc1s of the oracle)"""
    w = np.asarray(words, np.uint32)
    to_sel = np.array([2, 3, 1, 0], np.int64)
    out = np.zeros((w.size, 16), np.int64)
    for y in range(4):
        for x in range(4):
            bit = x * 4 + y
            out[:, y * 4 + x] = to_sel[((w >> bit) & 1) | (((w >> (16 + bit)) & 1) << 1)]
    return out


def texel_errors(tiles, enc, perceptual):
    """(n, 4, 16) int64: orc_color_distance of texel p = y * 4 + x of block i to colour s of the block's own endpoint (header of enc)"""
    n = tiles.shape[0]
    enc = np.asarray(enc)
    col = _metric_axes(_entry_colours(enc[:, :3] >> 3, enc[:, 3] >> 5), perceptual)                    # 3 x (n, 4)
    px = _metric_axes(np.asarray(tiles)[..., :3].reshape(n, 16, 3).astype(np.int32), perceptual)       # 3 x (n, 16)
    return _distance(perceptual, *[c[:, :, None] - p[:, None, :] for p, c in zip(px, col)]).astype(np.int64)


def fosc_errors(tiles, enc, selector_words, perceptual):
    """(n, K_s) int64 by the definition in orc_find_optimal_selector_clusters: the block's 16 texel errors under the selectors of entry k"""
    te = texel_errors(tiles, enc, perceptual)
    sel = word_selectors(selector_words)
    out = np.zeros((te.shape[0], sel.shape[0]), np.int64)
    for p in range(16):
        out += te[:, :, p][:, sel[:, p]]
    return out


def fosc_winners(err, tiles, lists, block_list, chunk):
    """first minimum in list order; a block identical to its predecessor inside a chunk takes the predecessor's choice (frontend.cpp:2557-2564); empty list: 0"""
    n = err.shape[0]
    out = np.zeros(n, np.uint32)
    for li, members in enumerate(lists):
        blocks = np.nonzero(block_list == li)[0]
        if blocks.size and len(members):
            members = np.asarray(members, np.int64)
            out[blocks] = members[err[np.ix_(blocks, members)].argmin(axis=1)]
    flat = np.asarray(tiles).reshape(n, -1)
    same = np.concatenate([[False], (flat[1:] == flat[:-1]).all(axis=1)]) & (np.arange(n) % chunk != 0)
    for b in np.nonzero(same)[0]:
        out[b] = out[b - 1]
    return out


def cosc_totals(tiles, enc, offsets, indices, perceptual):
    """(k, 16, 4) int64: the oracle's total_err[p][s] of every cluster"""
    te = texel_errors(tiles, enc, perceptual)
    k = offsets.size - 1
    out = np.zeros((k, 16, 4), np.int64)
    for c in range(k):
        out[c] = te[indices[offsets[c]:offsets[c + 1]]].sum(axis=0).T
    return out


# ----------------------------------------------------------------------------- refine cases

TEST_TEXELS = (0, 5, 10, 15)   # the four texels both refine kernels sum first and prune on (FIRST_PX)
N_THRESHOLD_TILES = 120


@functools.lru_cache(maxsize=None)
def _refine_endpoints():
    """which planted endpoints carry which planted pair: (e0: positions 3, 40, 300; e1: positions 260, 700; 56 with a copy in a slot of round 0; 60 with a copy in a
    later round; 3 whose exact endpoint stands twice)"""
    order = np.random.default_rng(4100).permutation(198)
    return int(order[0]), int(order[1]), order[2:SLOTS], order[SLOTS:SLOTS + 60], order[SLOTS + 60:SLOTS + 63]


@functools.lru_cache(maxsize=None)
def refine_tiles():
    """helpers.etc1s_planted_test_tiles trimmed to n % 4 == 3 (3,143: the last workgroup of four waves has one wave that exits), its last 120 ladder tiles replaced by
    THRESHOLD tiles: for every other endpoint with a copy in a later round, four tiles made of the endpoint's four colours with noise of 1..3 on the texels 0, 5, 10, 15
    alone. Their error under the endpoint lies wholly in the four texels the kernels look at first, so the partial sum they prune on EQUALS the threshold when the
    endpoint's other copy has set it: `partial <= threshold` is met with equality."""
    t = H.etc1s_planted_test_tiles()
    n = t.shape[0] - (t.shape[0] - 3) % 4
    t = np.ascontiguousarray(t[:n])
    meta = H.etc1s_planted_tiles()[1]
    head = np.searchsorted(meta["endpoint"], np.arange(198))
    rng = np.random.default_rng(4104)
    at = n - N_THRESHOLD_TILES
    for e in _refine_endpoints()[3][::2]:
        base = (meta["color5"][head[e]].astype(np.int64) << 3) | (meta["color5"][head[e]] >> 2)
        for _ in range(4):
            sel = rng.integers(0, 4, 16)
            sel[:4] = rng.permutation(4)
            px = np.clip(base[None, :] + H.ETC1_INTEN_TABLES[meta["table"][head[e]]][sel][:, None], 0, 255)
            noise = rng.integers(1, 4, (4, 3)) * rng.choice([-1, 1], (4, 3))
            px[list(TEST_TEXELS)] = np.clip(px[list(TEST_TEXELS)] + noise, 0, 255)
            t[at, :, :, :3] = px.reshape(4, 4, 3)
            at += 1
    assert at == n
    t.setflags(write=False)
    return t


def threshold_tile_endpoints():
    """the planted endpoint of each of the last N_THRESHOLD_TILES tiles of refine_tiles"""
    return np.repeat(_refine_endpoints()[3][::2], 4)


def texel_errors_under(tiles, params, perceptual):
    """(m, 16) int64: per texel of tile i the minimum over the four colours of entry params[i] of orc_color_distance (row i of one with row i of the other)"""
    m = tiles.shape[0]
    px = _metric_axes(np.asarray(tiles)[..., :3].reshape(m, 16, 3).astype(np.int32), perceptual)
    col = _metric_axes(_entry_colours(params[:, :3], params[:, 3]), perceptual)
    return _distance(perceptual, *[p[:, :, None] - c[:, None, :] for p, c in zip(px, col)]).min(axis=2).astype(np.int64)


def _nudged(src, rng):
    """the seam test's recipe: one colour component +-1 within 0..31, every fifth copy's table + 1 mod 8"""
    m = src.copy()
    i = np.arange(m.shape[0])
    ch = rng.integers(0, 3, m.shape[0])
    m[i, ch] = np.clip(m[i, ch].astype(np.int64) + rng.choice([-1, 1], m.shape[0]), 0, 31)
    m[::5, 3] = (m[::5, 3] + 1) % 8
    return m


def _table0_entries(pool, count_unclamped, count_clamped, rng):
    """table-0 entries from the pool's colours, jittered: components 1..30 (unclamped: 8 <= base - 8, base + 8 <= 255), or one component pushed to 0 or 31 (clamped)"""
    total = count_unclamped + count_clamped
    c = pool[rng.integers(0, pool.shape[0], total), :3].astype(np.int64) + rng.integers(-2, 3, (total, 3))
    c = np.clip(c, 1, 30)
    ch = rng.integers(0, 3, count_clamped)
    rows = np.arange(count_unclamped, total)
    c[rows, ch] = np.where(c[rows, ch] < 16, 0, 31)
    out = np.zeros((total, 4), np.uint8)
    out[:, :3] = c
    out = out[rng.permutation(total)]
    assert int(unclamped(out).sum()) == count_unclamped
    return out


@functools.lru_cache(maxsize=None)
def _refine_base(perceptual):
    """the codebook, the lists, the blocks' current clusters and their groups: shared by the three kinds of one perceptual value"""
    rng = np.random.default_rng(4101)
    tiles = refine_tiles()
    n = tiles.shape[0]
    meta = H.etc1s_planted_tiles()[1]
    n_ep = int(meta["endpoint"].max()) + 1
    fitted, cluster0 = H.planted_endpoint_codebook(perceptual)
    cluster0 = cluster0[:n].astype(np.int64)
    head = np.searchsorted(meta["endpoint"], np.arange(n_ep))
    exact = np.ascontiguousarray(np.concatenate([meta["color5"][head], meta["table"][head][:, None]], axis=1).astype(np.uint8))
    pool = np.concatenate([fitted, exact])
    assert n_ep == 198 and SLOTS + n_ep == RQ

    # ---- the long list: [slots][fitted][filler = nudged copies, of which 900 are copies of unclamped entries]
    n_fill = LONG - RQ
    plain_pool = pool[unclamped(pool)]
    fill = np.concatenate([_nudged(pool[np.arange(n_fill - 900) % pool.shape[0]], rng), _nudged(plain_pool[np.arange(900) % plain_pool.shape[0]], rng)])
    params = np.zeros((LONG, 4), np.uint8)
    params[SLOTS:RQ] = fitted
    params[RQ:] = fill[rng.permutation(n_fill)]
    named = (3, 40, 260, 300, 700)
    free = [int(p) for p in RQ + rng.permutation(n_fill) if int(p) not in named]
    exact_pos = np.array([free.pop() for _ in range(n_ep)])
    params[exact_pos] = exact                      # every planted endpoint itself: a zero-error entry for its noise-free tiles

    e0, e1, in_round, across, twice = _refine_endpoints()
    # half of the duplicated fitted entries are made exact, so that zero ties occur wherever a group is
    for e in np.concatenate([[e0, e1], in_round[::2], across[::2]]):
        params[SLOTS + e] = exact[e]
    group = np.zeros(n, np.uint8)
    pair = np.full((n, 2), -1, np.int64)           # (earlier position, later position) of a group block's pair
    cur = cluster0 + SLOTS
    ep_of = np.full(n, -1, np.int64)
    ep_of[:meta.shape[0]] = meta["endpoint"][:min(n, meta.shape[0])]
    ep_of[n - N_THRESHOLD_TILES:] = threshold_tile_endpoints()

    def file_under(e, first, later, g, which=slice(None)):
        """the blocks `which` of planted endpoint e: current cluster = the later member of the pair (first, later), whose entries are equal"""
        assert first < later and (params[first] == params[later]).all()
        b = np.nonzero(ep_of == e)[0][which]
        cur[b], group[b], pair[b] = later, g, (first, later)

    slots = [s for s in range(SLOTS) if s not in (3, 40)]
    params[3] = params[40] = params[300] = params[SLOTS + e0]
    file_under(e0, 3, 40, 1, slice(0, None, 2))         # positions 3 and 40: inside round 0
    file_under(e0, 3, 300, 2, slice(1, None, 2))        # positions 3 and 300: across rounds
    params[260] = params[700] = params[SLOTS + e1]
    file_under(e1, 260, 700, 2)                         # positions 260 and 700: across rounds
    for s, e in zip(slots, in_round):
        params[s] = params[SLOTS + e]
        file_under(e, s, SLOTS + e, 1)                  # the later member is the fitted entry: the cluster the codebook gives these blocks anyway
    for e in across:
        later = free.pop()
        params[later] = params[SLOTS + e]
        file_under(e, SLOTS + e, later, 2)
    for e in twice:
        later = next(p for p in free if p > exact_pos[e])
        free.remove(later)
        params[later] = exact[e]
        file_under(e, int(exact_pos[e]), later, 3, np.nonzero(meta["noise"][meta["endpoint"] == e] == 0)[0])

    # a pair whose members are in ONE round of the list as it comes (the unsorted kernel's rounds) and in TWO rounds of its queue's (table, position) order (the
    # sorted kernel's rounds): the two entries either side of a round boundary of the queue order, where they are of one table and nothing else was planted
    planted_at = set(named) | set(range(RQ)) | set(int(p) for p in exact_pos) | set(int(p) for p in pair[:, 1])
    queue_pair = None
    in_queue = np.nonzero(unclamped(params))[0] if perceptual else np.arange(LONG)
    order = in_queue[np.argsort(params[in_queue, 3], kind="stable")]
    for edge in range(RQ, order.size, RQ):
        a, b = sorted((int(order[edge - 1]), int(order[edge])))
        if params[a, 3] == params[b, 3] and a // RQ == b // RQ and a not in planted_at and b not in planted_at:
            params[b] = params[a]
            queue_pair = (a, b, edge)
            break
    assert queue_pair is not None

    # ---- the other lists, laid behind the long one; every list ascending
    lists = {"long": np.arange(LONG)}
    parts, at = [params], LONG
    for name, (n_plain, n_clamped) in T0_COUNTS.items():
        parts.append(_table0_entries(pool, n_plain, n_clamped, rng))
        lists[name] = np.arange(at, at + n_plain + n_clamped); at += n_plain + n_clamped
    cand = _nudged(plain_pool[rng.integers(0, plain_pool.shape[0], 400)], rng)
    cand = cand[unclamped(cand)][:64]
    clamped_pool = pool[~unclamped(pool)]
    parts.append(np.concatenate([cand, clamped_pool[rng.integers(0, clamped_pool.shape[0], 1)]])[rng.permutation(65)])
    lists["u64_c1"] = np.arange(at, at + 65); at += 65
    parts.append(exact[100:101])
    lists["single"] = np.arange(at, at + 1); at += 1
    lists["empty"] = np.zeros(0, np.int64)
    seven = pool[pool[:, 3] == 7]
    t7 = seven[np.arange(64) % seven.shape[0]].copy()
    ch = rng.integers(0, 3, 64)
    t7[np.arange(64), ch] = np.clip(t7[np.arange(64), ch].astype(np.int64) + rng.integers(-1, 2, 64), 0, 31)
    parts.append(t7)
    lists["table7"] = np.arange(at, at + 64); at += 64
    params = np.ascontiguousarray(np.concatenate(parts))
    k = params.shape[0]
    assert k == at and k <= 4000

    # ---- blocks: filed under the list of their current cluster; seeded runs of the others re-filed under the short lists with a member of it as current cluster
    block_list = np.zeros(n, np.int64)
    others = rng.permutation(np.nonzero(group == 0)[0])
    taken = 0
    for name, count in (("t0_255_257", 220), ("t0_256_256", 220), ("t0_257_255", 220), ("u64_c1", 120), ("single", 40), ("table7", 150)):
        b = others[taken:taken + count]; taken += count
        block_list[b] = REFINE_LISTS.index(name)
        cur[b] = rng.choice(lists[name], count)
    # a seeded eighth (of the blocks outside the groups) moved to a random other entry of its list
    moved = rng.permutation(others)[:n // 8]
    for b in moved:
        members = lists[REFINE_LISTS[block_list[b]]]
        if members.size > 1:
            cur[b] = members[(np.searchsorted(members, cur[b]) + rng.integers(1, members.size)) % members.size]
    list_of_cluster = np.zeros(k, np.int64)
    for li, name in enumerate(REFINE_LISTS):
        list_of_cluster[lists[name]] = li
    assert (list_of_cluster[cur] == block_list).all()     # every block is filed under the list that holds its current cluster
    return _frozen(dict(tiles=tiles, params=params, block_cluster=np.ascontiguousarray(cur.astype(np.uint32)), block_list=block_list, group=group, pair=pair,
                        lists=tuple(np.ascontiguousarray(lists[name].astype(np.uint32)) for name in REFINE_LISTS), queue_pair=np.array(queue_pair),
                        exact_pos=exact_pos, endpoint=ep_of))


@functools.lru_cache(maxsize=None)
def refine_case(kind, perceptual):
    """-> dict: tiles, params (K, 4), block_cluster, n_parents, cand_offsets, cand_indices, block_parent, expected (the oracle's), and what the host test counts with:
    lists (cluster indices per list, list order), block_list (the list every block is filed under; 0 in the flat case), group, pair, queue_pair, exact_pos, endpoint"""
    base = dict(_refine_base(int(perceptual)))
    tiles, params, cur = base["tiles"], base["params"], base["block_cluster"]
    n, k = tiles.shape[0], params.shape[0]
    if kind == "flat":
        n_parents, lists, block_list = 0, (np.arange(k, dtype=np.uint32),), np.zeros(n, np.int64)
        coffs, cidx = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    else:
        lists, block_list = base["lists"], base["block_list"].copy()
        n_parents = len(lists)
        if kind == "foreign":
            # a seeded quarter filed under a list that does not hold their current cluster (never the empty one); forty of them with a table below 7 under the table-7 list
            rng = np.random.default_rng(4102)
            q = rng.permutation(n)[:n // 4]
            non_empty = np.array([li for li, l in enumerate(lists) if l.size])
            block_list[q] = non_empty[(np.searchsorted(non_empty, block_list[q]) + rng.integers(1, non_empty.size, q.size)) % non_empty.size]
            low = q[params[cur[q], 3] < 7][:40]
            block_list[low] = REFINE_LISTS.index("table7")
            assert (block_list[q] != base["block_list"][q]).all()
        coffs, cidx = csr_from_lists(list(lists))
    block_parent = np.ascontiguousarray(block_list.astype(np.uint8))
    exp = np.zeros(n, np.uint32)
    oracle().orc_refine_endpoint_clusterization(ptr(tiles), n, ptr(cur, u32p), ptr(params), k, n_parents, ptr(coffs, u32p), ptr(cidx, u32p), ptr(block_parent),
                                                int(perceptual), ptr(exp, u32p))
    base.update(kind=kind, perceptual=int(perceptual), n_parents=n_parents, cand_offsets=coffs, cand_indices=cidx, block_parent=block_parent, expected=exp,
                lists=tuple(lists), block_list=block_list)
    return _frozen(base)


def queue_ranks(params, members, cur_table, perceptual):
    """For one list and one current table: (queue of every member: 0 unclamped, 1 clamped, -1 not admissible; rank of every member in its queue's order). The order is
    the sorted kernel's: by table, and inside a table by list position (the kernel's order inside a table is not defined; the round a rank falls in hardly depends on it)."""
    p = params[np.asarray(members, np.int64)]
    ok = p[:, 3] <= cur_table
    queue = np.where(ok, np.where(unclamped(p) & bool(perceptual), 0, 1), -1)
    rank = np.full(len(members), -1, np.int64)
    for qi in (0, 1):
        m = np.nonzero(queue == qi)[0]
        rank[m[np.argsort(p[m, 3], kind="stable")]] = np.arange(m.size)
    return queue, rank


# ----------------------------------------------------------------------------- selector cases

WHITE, BLACK = slice(2500, 2516), slice(2520, 2536)


@functools.lru_cache(maxsize=None)
def selector_tiles():
    """refine_tiles with the two runs of identical tiles of the existing selector test (one straddling block 2048), sixteen flat white and sixteen flat black tiles"""
    t = refine_tiles().copy()
    t[100:110] = t[100]
    t[2040:2060] = t[2040]
    t[WHITE, :, :, :3] = 255
    t[BLACK, :, :, :3] = 0
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def selector_enc(perceptual):
    enc = H.orc_encode_blocks(selector_tiles(), 1, perceptual)
    enc[105, :3] ^= 0x18      # identical tiles with DIFFERENT endpoints: the copied choice must still be the run head's
    enc.setflags(write=False)
    return enc


def _selector_clusters(enc, k, rng):
    """k - 1 seeded uneven runs of the blocks in selector-word order, and one empty cluster"""
    n = enc.shape[0]
    order = np.argsort(selector_word(enc), kind="stable")
    cuts = np.sort(rng.choice(np.arange(1, n), size=k - 2, replace=False))
    lists = [rng.permutation(r).astype(np.uint32) for r in np.split(order, cuts)]
    lists.insert(5, np.zeros(0, np.uint32))
    return lists


def _words_to_blocks(words):
    out = np.zeros((words.size, 8), np.uint8)
    for i in range(4):
        out[:, 4 + i] = (words >> (24 - 8 * i)) & 255
    return out


def selector_codebook_words(tiles, enc, perceptual, rng):
    """-> the selector words of (300 clusters fitted by the oracle's orc_create_optimized_selector_codebook to seeded runs of the blocks, 400 copies of those with one to
    three texels' selectors changed, 400 random words)"""
    offs, idx = csr_from_lists(_selector_clusters(enc, 300, rng))
    opt = np.zeros((300, 8), np.uint8)
    oracle().orc_create_optimized_selector_codebook(ptr(tiles), ptr(enc), 300, ptr(offs, u32p), ptr(idx, u32p), int(perceptual), ptr(opt))
    w_opt = selector_word(opt)
    w_near = w_opt[rng.integers(0, 300, 400)].copy()
    for i in range(w_near.size):
        for t in rng.choice(16, rng.integers(1, 4), replace=False):
            raw = int(rng.integers(0, 4))
            w_near[i] = (int(w_near[i]) & ~((1 << t) | (1 << (16 + t)))) | ((raw & 1) << t) | ((raw >> 1) << (16 + t))
    return w_opt, w_near, rng.integers(0, 2 ** 32, 400, dtype=np.uint64).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _fosc_base(perceptual):
    rng = np.random.default_rng(4202)
    tiles, enc = selector_tiles(), selector_enc(perceptual)
    n = tiles.shape[0]
    # 1,100 entries in a seeded order; the last 100 random words are spare entries for the planted duplicates
    w_opt, w_near, w_rand = selector_codebook_words(tiles, enc, perceptual, rng)
    where = rng.permutation(1100)
    words = np.zeros(1100, np.uint32)
    words[where] = np.concatenate([w_opt, w_near, w_rand])
    spare = [int(s) for s in where[1000:]]
    usable = np.sort(where[:1000])

    lists = [rng.permutation(usable)[:m].astype(np.int64) for m in FOSC_LENS]
    block_list = rng.choice(len(FOSC_LENS), n, p=[0.11, 0.11, 0.11, 0.22, 0.31, 0.06, 0.03, 0.05])
    # the planted duplicates of the 700 and the 447 list: where the blocks filed there find their minimum today, a copy of that entry 1, 64 or 320 positions on
    # (neighbouring lanes; the same lane one and five iterations later), and the list's most chosen entry moved to position 0 with a copy in the last
    err = fosc_errors(tiles, enc, words, perceptual)
    pairs = []
    for li in (4, 3):
        l = lists[li]
        blocks = np.nonzero(block_list == li)[0]
        votes = np.bincount(err[np.ix_(blocks, l)].argmin(axis=1), minlength=l.size)
        top = int(votes.argmax())
        l[[0, top]] = l[[top, 0]]
        votes[[0, top]] = votes[[top, 0]]
        used = {0, l.size - 1}
        l[-1] = spare.pop(); words[l[-1]] = words[l[0]]
        pairs.append((li, 0, l.size - 1, int(votes[0])))
        reach = {d: 0 for d in FOSC_SPACINGS}
        for k in np.argsort(-votes, kind="stable"):
            k = int(k)
            if not votes[k] or len(spare) < 8:
                break
            for d in sorted(FOSC_SPACINGS, key=lambda d: reach[d]):
                if k not in used and k + d < l.size and k + d not in used:
                    used.update((k, k + d))
                    l[k + d] = spare.pop(); words[l[k + d]] = words[l[k]]
                    pairs.append((li, k, d, int(votes[k])))
                    reach[d] += int(votes[k])
                    break
    sel = _words_to_blocks(words)
    return _frozen(dict(tiles=tiles, enc=enc, selector_blocks=sel, selector_words=words, lists=tuple(np.ascontiguousarray(l.astype(np.uint32)) for l in lists),
                        block_list=block_list, pairs=np.array(pairs, np.int64)))


@functools.lru_cache(maxsize=None)
def fosc_case(kind, perceptual):
    """-> dict: tiles, enc (before the call), selector_blocks (K_s, 8), selector_words, n_parents, cand_offsets, cand_indices, block_parent, chunk, expected_idx,
    expected_enc (the oracle's), lists, block_list, pairs (list, position, spacing -- or last position for position 0 --, blocks that chose it before the copy went in)"""
    base = dict(_fosc_base(int(perceptual)))
    tiles, enc, sel = base["tiles"], base["enc"], base["selector_blocks"]
    n, k = tiles.shape[0], sel.shape[0]
    if kind == "flat":
        n_parents, lists, block_list = 0, (np.arange(k, dtype=np.uint32),), np.zeros(n, np.int64)
        coffs, cidx = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    else:
        lists, block_list = base["lists"], base["block_list"]
        n_parents = len(lists)
        coffs, cidx = csr_from_lists(list(lists))
    block_parent = np.ascontiguousarray(block_list.astype(np.uint8))
    exp_enc, exp_idx = enc.copy(), np.zeros(n, np.uint32)
    oracle().orc_find_optimal_selector_clusters(ptr(tiles), ptr(exp_enc), n, ptr(sel), k, n_parents, ptr(coffs, u32p), ptr(cidx, u32p), ptr(block_parent),
                                                int(perceptual), 2048, ptr(exp_idx, u32p))
    base.update(kind=kind, perceptual=int(perceptual), n_parents=n_parents, cand_offsets=coffs, cand_indices=cidx, block_parent=block_parent, chunk=2048,
                expected_idx=exp_idx, expected_enc=exp_enc, lists=tuple(lists), block_list=block_list)
    return _frozen(base)


@functools.lru_cache(maxsize=None)
def cosc_case(perceptual):
    """One CSR over selector_enc whose cluster boundaries sit where k_cosc_accumulate's 128-member chunks begin, end and are stepped over.
    -> dict: tiles, enc, offsets, indices, stale (k, 8: random bytes everywhere), expected (the oracle's), names (cluster index of every named cluster)"""
    rng = np.random.default_rng(4303)
    tiles, enc = selector_tiles(), selector_enc(int(perceptual))
    n = tiles.shape[0]
    special = np.zeros(n, bool)
    special[WHITE] = special[BLACK] = True
    rest = list(rng.permutation(np.nonzero(~special)[0]))
    lists, names = [], {}

    def add(name, members):
        if name:
            names[name] = len(lists)
        lists.append(np.asarray(members, np.uint32))

    def take(count):
        out = rest[:count]
        del rest[:count]
        return out

    add("first_empty", [])
    add("giant", take(1500))                      # members 0..1499: eleven chunks and 92 members of the twelfth
    add("ends_on_edge_a", take(36))               # ends at 1536 = 12 * 128
    add("starts_on_edge_a", take(100))            # starts at 1536
    for i in range(5):
        add(f"empty_run_{i}", [])                 # five empty clusters at member 1636, in the middle of chunk 12
    add("ends_on_edge_b", take(28))               # 1636..1663: ends at 1664 = 13 * 128
    add("one_chunk", take(128))                   # exactly chunk 13
    for i in range(20):
        add(f"single_{i}", take(1))
    add("white", np.arange(WHITE.start, WHITE.stop))
    add("black", np.arange(BLACK.start, BLACK.stop))
    cuts = np.sort(rng.choice(np.arange(1, len(rest)), size=39, replace=False))
    for run in np.split(np.array(rest), cuts):
        add(None, run)
    add("last_empty", [])
    offs, idx = csr_from_lists(lists)
    k = len(lists)
    stale = rng.integers(0, 256, (k, 8), dtype=np.uint8)
    exp = stale.copy()
    oracle().orc_create_optimized_selector_codebook(ptr(tiles), ptr(enc), k, ptr(offs, u32p), ptr(idx, u32p), int(perceptual), ptr(exp))
    return _frozen(dict(tiles=tiles, enc=enc, perceptual=int(perceptual), offsets=offs, indices=idx, stale=stale, expected=exp, names=names))
