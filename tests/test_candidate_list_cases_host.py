"""That the generated inputs of tests/test_gpu_candidate_lists.py (candidate_list_cases.py) reach what they were made to reach: candidate lists of several rounds in
each queue of the refine kernels, winners found in a late round, ties between equal entries inside a round and across rounds that the current cluster or the earlier position
must win, lists without an admissible entry, selector lists on both sides of the quad-table threshold with equal entries in neighbouring lanes and in later iterations, and
a member CSR whose cluster boundaries sit on, before and under the 128-member chunks. CPU only, and the oracle only: the conditions are on the INPUTS, so a failure here is
mended in the builders, never in the thresholds. The figures in brackets are what the builders give today (perceptual 1 / 0 where two are given).
"""
import numpy as np
import pytest

import candidate_list_cases as CL

PERCEPTUAL = [1, 0]


@pytest.fixture(scope="module", params=PERCEPTUAL)
def refine(request):
    """per perceptual value: the three cases and the masked (n, K) errors they share (same tiles, codebook and current clusters)"""
    p = request.param
    cases = {kind: CL.refine_case(kind, p) for kind in CL.REFINE_KINDS}
    flat = cases["flat"]
    return p, cases, CL.refine_errors(flat["tiles"], flat["params"], p, flat["block_cluster"])


def test_refine_restatement_reproduces_the_oracle(refine):
    p, cases, err = refine
    for kind, c in cases.items():
        got = CL.refine_winners(err, c["block_cluster"], c["lists"], c["block_list"])
        assert (got == c["expected"]).all(), (kind, p, np.nonzero(got != c["expected"])[0][:8])
    plain = CL.unclamped(cases["flat"]["params"])
    assert (plain == (CL.H.etc1s_clamp_class(cases["flat"]["params"][:, :3], cases["flat"]["params"][:, 3]) == 0)).all()


def test_refine_layout(refine):
    p, cases, _ = refine
    flat, hier, foreign = cases["flat"], cases["hier"], cases["foreign"]
    n, k = flat["tiles"].shape[0], flat["params"].shape[0]
    assert n % 4 == 3 and k <= 4000                                    # [3143, 3566]
    assert flat["n_parents"] == 0 and hier["n_parents"] == 8 and (hier["cand_offsets"] == foreign["cand_offsets"]).all()
    params, plain = hier["params"], CL.unclamped(hier["params"])
    lists = dict(zip(CL.REFINE_LISTS, hier["lists"]))
    filed = np.bincount(hier["block_list"], minlength=8)
    for name, l in lists.items():
        assert (np.diff(l.astype(np.int64)) > 0).all(), name            # ascending, every cluster once
        assert (filed[CL.REFINE_LISTS.index(name)] > 0) == (name != "empty"), name
    assert sum(l.size for l in lists.values()) == k                     # the lists partition the codebook
    long = lists["long"]
    assert int(plain[long].sum()) >= 600 and int((~plain[long]).sum()) >= 600   # [848 unclamped and 1,052 clamped / 849 and 1,051]
    for name, (n_plain, n_clamped) in CL.T0_COUNTS.items():
        l = lists[name]
        assert (params[l, 3] == 0).all() and int(plain[l].sum()) == n_plain and int((~plain[l]).sum()) == n_clamped
        assert filed[CL.REFINE_LISTS.index(name)] >= 200                # [220 each]
    assert int(plain[lists["u64_c1"]].sum()) == 64 and lists["u64_c1"].size == 65
    assert lists["single"].size == 1 and lists["empty"].size == 0 and (params[lists["table7"], 3] == 7).all() and lists["table7"].size == 64
    print("blocks per list", dict(zip(CL.REFINE_LISTS, filed.tolist())))
    # every block of `hier` is filed under the list of its current cluster, a quarter of `foreign` is not
    list_of = np.zeros(k, np.int64)
    for li, l in enumerate(hier["lists"]):
        list_of[l] = li
    cur = hier["block_cluster"]
    assert (list_of[cur] == hier["block_list"]).all()
    strangers = list_of[cur] != foreign["block_list"]
    assert strangers.sum() == n // 4 and filed[CL.REFINE_LISTS.index("empty")] == 0 and (foreign["block_list"] != CL.REFINE_LISTS.index("empty")).all()
    assert (foreign["block_list"][strangers] == 0).sum() >= 30           # the long list is among the lists used [46]
    # the planted pairs: equal entries at the named positions
    for a, b in ((3, 40), (3, 300), (260, 700)):
        assert (params[a] == params[b]).all()
    a, b, edge = (int(v) for v in hier["queue_pair"])
    assert (params[a] == params[b]).all() and a // CL.RQ == b // CL.RQ   # one round of the list as it comes ...
    queue, rank = CL.queue_ranks(params, long, 7, p)
    assert queue[a] == queue[b] and {int(rank[a]), int(rank[b])} == {edge - 1, edge} and edge % CL.RQ == 0   # ... two rounds of its queue's order
    exact = hier["exact_pos"]
    assert exact.size == 198 and np.unique(exact).size == 198 and (exact >= CL.RQ).all() and (exact < CL.LONG).all()
    assert (hier["group"] == 3).sum() >= 18 and (hier["pair"][hier["group"] == 3, 0] < hier["pair"][hier["group"] == 3, 1]).all()
    # the current clusters: as the codebook gives them, moved, set by a group -- all three present
    assert (hier["group"] > 0).sum() >= 50 * 3 and (hier["group"] == 0).sum() >= n // 2


def test_refine_lists_run_to_several_rounds(refine):
    p, cases, err = refine
    deep = {q: 0 for q in ("each queue > 512", "clamped > 1024")}
    late = {256: 0, 512: 0, "list position >= 256": 0}
    for kind in ("flat", "hier"):
        c = cases[kind]
        params, cur, exp = c["params"], c["block_cluster"], c["expected"]
        for li, members in enumerate(c["lists"]):
            if not members.size:
                continue
            pos_of = np.full(params.shape[0], -1, np.int64)
            pos_of[members] = np.arange(members.size)
            for t in range(8):
                blocks = np.nonzero((c["block_list"] == li) & (params[cur, 3] == t))[0]
                if not blocks.size:
                    continue
                queue, rank = CL.queue_ranks(params, members, t, p)
                counts = [(queue == 0).sum(), (queue == 1).sum()]
                deep["each queue > 512"] += blocks.size * (min(counts) > 512)
                deep["clamped > 1024"] += blocks.size * (counts[1] > 1024)
                w = pos_of[exp[blocks]]
                assert (w >= 0).all() and (queue[w] >= 0).all()            # every winner is an admissible member of the block's list
                for edge in (256, 512):
                    late[edge] += int((rank[w] >= edge).sum())
                late["list position >= 256"] += int((w >= 256).sum())
    print(p, deep, late)
    if p:
        assert deep["each queue > 512"] >= 200      # [4240: every block of the flat case, 1,097 blocks of the long list]
    else:
        assert deep["clamped > 1024"] >= 200        # [4239: every entry is in the clamped queue]
    assert late[256] >= 100 and late[512] >= 30     # [4216 and 3329 / 4887 and 4158: in the flat case 768 table-0 entries come first in each queue]
    assert late["list position >= 256"] >= 100      # the rounds of the unsorted kernel [3390 / 3400]


def test_refine_ties_are_decisive(refine):
    p, cases, err = refine
    counts = {}
    for kind in ("flat", "hier"):
        c = cases[kind]
        cur, exp, group, pair = c["block_cluster"].astype(np.int64), c["expected"].astype(np.int64), c["group"], c["pair"]
        b = np.nonzero(group > 0)[0]
        first, later = pair[b, 0], pair[b, 1]
        assert (cur[b] == later).all() and (c["block_list"][b] == 0).all()          # positions in the long list (or the flat list) are cluster indices
        e_first, e_later = err[b, first], err[b, later]
        lo = (err[b][:, :CL.LONG] if kind == "hier" else err[b]).min(axis=1)                # the minimum over the block's list
        shared = (e_first == lo) & (e_later == lo)                                   # both members of the pair hold the list's minimum
        one_round = first // CL.RQ == later // CL.RQ
        for zero in (False, True):
            for same in (True, False):
                sel = shared & ((lo == 0) == zero) & (one_round == same)
                # the winner the rule names: at error 0 the earliest position with it, else the current cluster (the later member); never the other member
                if zero:
                    ok = (exp[b][sel] != later[sel]) & (err[b[sel], exp[b][sel]] == 0) & (exp[b][sel] <= first[sel])
                    decided = int((ok & (exp[b][sel] == first[sel])).sum())
                else:
                    ok = exp[b][sel] == later[sel]
                    decided = int(ok.sum())
                assert ok.all(), (kind, zero, same)
                counts[kind, "zero" if zero else "non-zero", "one round" if same else "across rounds"] = decided
    print(p, counts)
    for key, v in counts.items():
        assert v >= 50, (key, v)    # [flat and hier alike: non-zero 299 in one round and 399 across, zero 279 in one round and 273 across / 291, 399, 279, 273]


def test_refine_threshold_is_met_with_equality(refine):
    """the threshold tiles: the error under the pair's entry is non-zero and lies wholly in the four texels the kernels sum first, the pair holds the list's minimum and the
    later member (the current cluster) wins; counted where the members sit in different rounds of the clamped queue's order, so that the round of the earlier one has set the
    threshold to exactly the partial sum of the later one"""
    p, cases, err = refine
    for kind in ("flat", "hier"):
        c = cases[kind]
        n, params = c["tiles"].shape[0], c["params"]
        b = np.arange(n - CL.N_THRESHOLD_TILES, n)
        first, later = c["pair"][b, 0], c["pair"][b, 1]
        assert (c["group"][b] == 2).all() and (c["endpoint"][b] == CL.threshold_tile_endpoints()).all()
        te = CL.texel_errors_under(c["tiles"][b], params[later], p)
        whole, part = te.sum(axis=1), te[:, list(CL.TEST_TEXELS)].sum(axis=1)
        assert (whole == err[b, later]).all() and (whole == part).all() and (whole > 0).all()
        lo = (err[b][:, :CL.LONG] if kind == "hier" else err[b]).min(axis=1)
        decisive = (err[b, first] == lo) & (whole == lo) & (c["expected"][b] == later)
        apart = np.zeros(b.size, bool)
        for t in range(8):
            queue, rank = CL.queue_ranks(params, c["lists"][0], t, p)
            of_t = params[later, 3] == t
            apart |= of_t & (queue[later] == 1) & (rank[first] // CL.RQ != rank[later] // CL.RQ)
        print(p, kind, "threshold tiles with a decisive tie", int(decisive.sum()), "of them across rounds of the clamped queue", int((decisive & apart).sum()))
        assert decisive.sum() >= 100 and (decisive & apart).sum() >= 10     # [120 and 52 in both cases / 120 and 24 flat, 104 hier]


def test_refine_no_admissible_entry_and_movement(refine):
    p, cases, err = refine
    c = cases["foreign"]
    t7 = CL.REFINE_LISTS.index("table7")
    none = (c["block_list"] == t7) & (c["params"][c["block_cluster"], 3] < 7)
    assert none.sum() >= 30 and (c["expected"][none] == 0).all()     # [149 / 149]
    for kind, c in cases.items():
        moved = int((c["expected"] != c["block_cluster"]).sum())
        print(p, kind, "blocks that change cluster", moved)
        assert moved >= c["expected"].size // 10                      # [flat 2302, hier 2246, foreign 2485 / 2308, 2249, 2490 of 3143]


# ----------------------------------------------------------------------------- selector assignment

@pytest.fixture(scope="module", params=PERCEPTUAL)
def fosc(request):
    p = request.param
    cases = {kind: CL.fosc_case(kind, p) for kind in ("flat", "hier")}
    c = cases["flat"]
    return p, cases, CL.fosc_errors(c["tiles"], c["enc"], c["selector_words"], p)


def test_fosc_restatement_reproduces_the_oracle(fosc):
    p, cases, err = fosc
    for kind, c in cases.items():
        got = CL.fosc_winners(err, c["tiles"], c["lists"], c["block_list"], c["chunk"])
        assert (got == c["expected_idx"]).all(), (kind, p, np.nonzero(got != c["expected_idx"])[0][:8])
        want = c["enc"].copy()
        want[:, 4:] = c["selector_blocks"][got, 4:]
        assert (want == c["expected_enc"]).all()


def test_fosc_layout_and_ties(fosc):
    p, cases, err = fosc
    flat, hier = cases["flat"], cases["hier"]
    tiles, n = flat["tiles"], flat["tiles"].shape[0]
    assert flat["selector_blocks"].shape == (1100, 8) and flat["n_parents"] == 0 and hier["n_parents"] == 8
    assert (tiles[2040:2060] == tiles[2040]).all() and (tiles[100:110] == tiles[100]).all() and (flat["enc"][105, :3] != flat["enc"][104, :3]).any()
    assert tuple(l.size for l in hier["lists"]) == CL.FOSC_LENS
    filed = np.bincount(hier["block_list"], minlength=8)
    assert (filed >= 50).all(), filed.tolist()                                      # [349, 346, 335, 719, 963, 184, 91, 156]
    for l in hier["lists"]:
        assert np.unique(l).size == l.size and (l.size < 2 or (np.diff(l.astype(np.int64)) < 0).any())   # every entry once, in no cluster order
    empty = hier["block_list"] == CL.FOSC_LENS.index(0)
    runs = np.concatenate([[False], (tiles.reshape(n, -1)[1:] == tiles.reshape(n, -1)[:-1]).all(axis=1)])
    assert (hier["expected_idx"][empty & ~runs] == 0).all()                         # blocks filed under the empty list come out as entry 0
    words = hier["selector_words"]
    shared = {d: 0 for d in CL.FOSC_SPACINGS + ("first and last",)}
    for li, k, d, _ in hier["pairs"]:
        l = hier["lists"][li].astype(np.int64)
        other = d if k == 0 and d == l.size - 1 else k + d
        assert words[l[k]] == words[l[other]] and l[k] != l[other]
        blocks = np.nonzero((hier["block_list"] == li) & ~runs)[0]
        sub = err[np.ix_(blocks, l)]
        at_min = (sub[:, k] == sub.min(axis=1)) & (sub[:, other] == sub.min(axis=1))
        assert (hier["expected_idx"][blocks[at_min]] == l[sub[at_min].argmin(axis=1)]).all()
        shared["first and last" if other != k + d or d not in CL.FOSC_SPACINGS else d] += int(at_min.sum())
    print(p, "blocks whose minimum two equal entries share, by spacing", shared)
    for d in CL.FOSC_SPACINGS:
        assert shared[d] >= 100, (d, shared)                                        # [1: 133, 64: 129, 320: 127, first and last: 39 / 133, 139, 134, 44]
    late, distinct = 0, set()
    for kind, c in cases.items():
        for li, l in enumerate(c["lists"]):
            blocks = np.nonzero((c["block_list"] == li) & ~runs)[0]
            if l.size and blocks.size:
                pos_of = np.full(1100, -1, np.int64)
                pos_of[l] = np.arange(l.size)
                w = pos_of[c["expected_idx"][blocks]]
                assert (w >= 0).all()
                late += int((w >= CL.FOSC_QUAD_MIN).sum())
        distinct |= set(c["expected_idx"].tolist())
    print(p, "winners at positions >= 384:", late, "distinct winners:", len(distinct))
    assert late >= 100 and len(distinct) > 200                                      # [2267 and 980 / 2198 and 973]


# ----------------------------------------------------------------------------- selector codebook

@pytest.mark.parametrize("perceptual", PERCEPTUAL)
def test_cosc_layout(perceptual):
    c = CL.cosc_case(perceptual)
    offs, names = c["offsets"].astype(np.int64), c["names"]
    size = np.diff(offs)
    k = size.size
    chunk = CL.COSC_CHUNK
    assert names["first_empty"] == 0 and size[0] == 0 and names["last_empty"] == k - 1 and size[-1] == 0
    assert size[names["giant"]] >= 1500 and offs[-1] % chunk != 0 and offs[-1] == c["tiles"].shape[0]      # [1500; 3143 members = 24 chunks and 71]
    assert np.sort(c["indices"]).tolist() == list(range(c["tiles"].shape[0]))                               # every block in one cluster
    for name in ("starts_on_edge_a", "one_chunk"):
        assert offs[names[name]] % chunk == 0 and size[names[name]] > 0
    for name in ("ends_on_edge_a", "ends_on_edge_b", "one_chunk"):
        assert offs[names[name] + 1] % chunk == 0 and size[names[name]] > 0
    run = [names[f"empty_run_{i}"] for i in range(5)]
    assert run == list(range(run[0], run[0] + 5)) and (size[run] == 0).all()
    assert offs[run[0]] % chunk != 0 and size[run[0] - 1] > 0 and size[run[-1] + 1] > 0                    # stepped over in the middle of a chunk's walk
    singles = [names[f"single_{i}"] for i in range(20)]
    assert singles == list(range(singles[0], singles[0] + 20)) and (size[singles] == 1).all()
    tiles = c["tiles"]
    for name, value in (("white", 255), ("black", 0)):
        members = c["indices"][offs[names[name]]:offs[names[name] + 1]]
        assert members.size == 16 and (tiles[members][..., :3] == value).all()
    # stale bytes everywhere; only the selector bytes of non-empty clusters change
    exp, stale = c["expected"], c["stale"]
    assert (exp[:, :4] == stale[:, :4]).all() and (exp[size == 0] == stale[size == 0]).all() and (exp[size > 0, 4:] != stale[size > 0, 4:]).any(axis=1).sum() > k // 2
    tot = CL.cosc_totals(tiles, c["enc"], c["offsets"], c["indices"], perceptual)
    best = tot.min(axis=2, keepdims=True)
    tied = ((tot == best).sum(axis=2) > 1).any(axis=1) & (size > 0)
    print(perceptual, "clusters with two selectors tied for a texel", np.nonzero(tied)[0].tolist())
    assert tied[names["white"]] and tied[names["black"]]               # [the white and the black cluster]
    # ... and the restated totals give the oracle's selectors: the lowest of the tied ones
    sel = CL.word_selectors(CL.selector_word(exp))
    assert (sel[size > 0] == tot.argmin(axis=2)[size > 0]).all()
