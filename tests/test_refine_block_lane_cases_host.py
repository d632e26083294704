"""That the generated inputs of tests/test_gpu_refine_block_lanes.py (refine_block_lane_cases.py) reach what they were made to reach in the refine path that gives
every block a lane: buckets of 0, 1, 63, 64, 65 and 129 blocks among 16 parents x 8 tables, a block count that is no multiple of 64, one wave whose lanes queue from
no entry at all to several times the queue's capacity, clamped entries that pass the four-texel look in some lanes of that wave only, zero-error winners, both kinds
of tie, lists without an admissible entry, blocks filed under a list that does not hold their current cluster, a flat codebook and a call on a sub-range. CPU only,
and the oracle only: the conditions are on the INPUTS, so a failure here is mended in the builder, never in the thresholds. Figures in brackets: what the builder
gives today (perceptual 1 / 0 where two are given).
"""
import numpy as np
import pytest

import candidate_list_cases as CL
import refine_block_lane_cases as RB

PERCEPTUAL = [1, 0]


@pytest.fixture(scope="module", params=PERCEPTUAL)
def lanes(request):
    p = request.param
    cases = {kind: RB.lane_case(kind, p) for kind in RB.KINDS}
    c = cases["hier"]
    return p, cases, CL.refine_errors(c["tiles"], c["params"], p, c["block_cluster"])


def test_restatement_reproduces_the_oracle(lanes):
    p, cases, err = lanes
    for kind, c in cases.items():
        got = CL.refine_winners(err, c["block_cluster"], c["lists"], c["block_list"])
        assert (got == c["expected"]).all(), (kind, p, np.nonzero(got != c["expected"])[0][:8])


def test_layout_and_bucket_sizes(lanes):
    p, cases, _ = lanes
    hier, foreign, flat = cases["hier"], cases["foreign"], cases["flat"]
    n, k = hier["tiles"].shape[0], hier["params"].shape[0]
    assert 2000 <= n <= 4096 and n % 64 != 0 and k <= 1900                       # [3143 blocks = 49 waves' worth and 7; 1320 clusters]
    assert hier["n_parents"] == foreign["n_parents"] == RB.N_PARENTS == 16 and flat["n_parents"] == 0
    assert hier["lists"][RB.P_EMPTY].size == 0 and hier["lists"][RB.P_UNUSED].size > 0
    for l in hier["lists"]:
        assert np.unique(l).size == l.size and (l.size < 2 or (np.diff(l.astype(np.int64)) < 0).any())   # every cluster once, in no cluster order
    sizes = np.bincount(RB.bucket_keys(hier), minlength=128).reshape(16, 8)
    for (parent, table), want in RB.BUCKET_SIZES.items():
        assert sizes[parent, table] == want
    assert {0, 1, 63, 64, 65, 129} <= set(sizes.reshape(-1).tolist())
    assert (sizes == 0).sum() >= 16 and (sizes[RB.P_EMPTY] == 0).all() and (sizes[RB.P_UNUSED] == 0).all() and (sizes > 0).sum() >= 90   # [24 empty, 104 in use]
    assert (sizes > 64).sum() >= 3                                                # buckets of more than one wave [3 / 4]
    print(p, "bucket sizes", sizes.tolist())
    # the flat case: eight buckets, by table alone
    assert set(RB.bucket_keys(flat).tolist()) == set(range(8))
    s0, s1 = RB.SLAB
    assert 0 < s0 < s1 < n and s0 % 64 and s1 % 64 and (s1 - s0) % 64            # the sub-range call: pointers offset by 1000 blocks, 1,111 blocks
    # every block of `hier` is filed under a list that holds its current cluster
    for li, l in enumerate(hier["lists"]):
        b = hier["block_list"] == li
        assert np.isin(hier["block_cluster"][b], l).all()


def test_survivor_extremes_share_a_wave():
    """Bucket (parent 0, table 7) has 64 blocks: one wave, whatever order the scatter leaves. A lane queues an unclamped entry when the entry's chroma bound is at most
    the lane's threshold at that moment; the threshold starts at the error of the current cluster and never falls below the minimum m over the block's list, so
        #{entries with bound <= m}  <=  entries queued  <=  #{entries with bound <= error of the current cluster}.
    Lanes whose current cluster is an exact match that needs clamping start at threshold 0 with no unclamped entry at bound 0: nothing is queued. Lanes on a far-off member
    queue several times the capacity."""
    c = RB.lane_case("hier", 1)
    params, cur = c["params"], c["block_cluster"].astype(np.int64)
    b = np.nonzero(RB.bucket_keys(c) == 0 * 8 + 7)[0]
    assert b.size == 64
    members = c["lists"][0].astype(np.int64)
    plain = CL.unclamped(params[members])                                          # table 7 admits every entry
    err = CL.refine_errors(c["tiles"][b], params, 1)
    floor, first = err[:, members].min(axis=1), err[np.arange(64), cur[b]]
    bound = RB.chroma_bounds(c["tiles"][b], params[members])
    assert (bound[:, plain] <= err[:, members[plain]]).all()                       # the restated bound is one
    at_least = ((bound <= floor[:, None]) & plain[None, :]).sum(axis=1)
    at_most = ((bound <= first[:, None]) & plain[None, :]).sum(axis=1)
    print("unclamped entries", int(plain.sum()), "queued at least", np.sort(at_least).tolist(), "at most", np.sort(at_most).tolist())
    assert (at_most == 0).sum() >= 6 and ((first == 0) & (at_most == 0)).sum() >= 6     # [13 lanes queue nothing, 12 of them exact matches]
    assert at_least.max() > 2 * RB.QCAP and (at_least > 2 * RB.QCAP).sum() >= 20        # [77; 41 lanes past twice the capacity]
    assert np.unique(at_least).size >= 10                                                # and counts in between [21 distinct]
    # clamped entries that pass the four-texel look in some lanes only: surely in (first look <= m), surely out (first look > the first threshold)
    look = RB.first_look(c["tiles"][b], params[members[~plain]], 1)
    split = (look <= floor[:, None]).any(axis=0) & (look > first[:, None]).any(axis=0)
    print("clamped entries", int((~plain).sum()), "in for some lanes and out for others", int(split.sum()))
    assert split.sum() >= 20                                                        # [69 of 74]


def test_ties_zero_winners_and_groups(lanes):
    p, cases, err = lanes
    c = cases["hier"]
    cur, exp, group, pair = c["block_cluster"].astype(np.int64), c["expected"].astype(np.int64), c["group"], c["pair"]
    lo = np.array([err[b, c["lists"][c["block_list"][b]].astype(np.int64)].min() for b in range(cur.size)])
    counts = {}
    for g in (RB.TIE_NONZERO, RB.TIE_ZERO):
        b = np.nonzero(group == g)[0]
        first, later = pair[b, 0], pair[b, 1]
        assert (cur[b] == later).all() and (c["params"][first] == c["params"][later]).all() and (first != later).all()
        shared = (err[b, first] == lo[b]) & (err[b, later] == lo[b])
        if g == RB.TIE_NONZERO:
            sel = shared & (lo[b] != 0)
            assert (exp[b][sel] == later[sel]).all()                               # the current cluster wins, though it stands later in the list
        else:
            sel = shared & (lo[b] == 0)
            assert (exp[b][sel] != later[sel]).all() and (err[b[sel], exp[b][sel]] == 0).all()   # the first zero in list order wins, never the current cluster
        counts[g] = int(sel.sum())
    zero = int((lo == 0).sum())
    print(p, "decisive ties", counts, "zero-error winners", zero)
    assert counts[RB.TIE_NONZERO] >= 100 and counts[RB.TIE_ZERO] >= 100 and zero >= 300   # [249, 330 and 991 / 240, 330 and 992]
    for kind, k in cases.items():
        assert (k["expected"] != k["block_cluster"]).sum() >= k["expected"].size // 10


def test_foreign_blocks_and_lists_without_an_admissible_entry(lanes):
    p, cases, _ = lanes
    hier, c = cases["hier"], cases["foreign"]
    strangers = np.array([cu not in set(c["lists"][li].tolist()) for cu, li in zip(c["block_cluster"], c["block_list"])])
    assert strangers.sum() >= c["expected"].size // 8 and (c["block_list"] != RB.P_EMPTY).all()     # [523 of 3143]
    assert (c["block_list"][strangers] == RB.P_UNUSED).sum() >= 10                                    # the list nobody is filed under in `hier` is swept here
    none = (c["block_list"] == RB.P_TABLE7) & (c["params"][c["block_cluster"], 3] < 7)
    assert none.sum() >= 30 and (c["expected"][none] == 0).all()                                      # [40]
    # strangers and residents share buckets: a wave redoes some lanes and keeps the others
    keys = RB.bucket_keys(c)
    mixed = sum(1 for k in np.unique(keys) if strangers[keys == k].any() and not strangers[keys == k].all())
    assert mixed >= 30
    assert (hier["block_list"] != c["block_list"]).sum() == strangers.sum()
