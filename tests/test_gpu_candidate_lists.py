"""-m gpu parity tests of the three ETC1S frontend kernels that take a list in fixed-size pieces, on lists well past the first piece: bu_hip_k_refine_endpoint_clusterization
(k_refine_sorted and the unsorted k_refine_endpoint_clusterization: rounds of 256 candidates per queue), bu_hip_k_find_optimal_selector_clusters (pair tables below 384
candidates, quad tables from there) and bu_hip_k_create_optimized_selector_codebook (128-member chunks of the CSR). Bit-exact against oracle/etc1s_oracle.c.

The inputs come from candidate_list_cases.py, one oracle run per case and process; what they reach (queues of five rounds, winners in late rounds, ties the current
cluster or the earlier position must win inside a round and across rounds, lists without an admissible entry, equal selector words in neighbouring lanes and in later
iterations, cluster boundaries on and under the chunk edges) is held on the CPU by test_candidate_list_cases_host.py."""
import ctypes as C

import numpy as np
import pytest

import candidate_list_cases as CL

pytestmark = pytest.mark.gpu

VP = C.c_void_p


def _describe_refine(case, got, bad):
    """the first differing blocks of a refine case: their list, where the expected winner sits (queue and rank in the queue's order, list position), their group"""
    params, cur = case["params"], case["block_cluster"]
    lines = []
    for b in bad[:5]:
        li = int(case["block_list"][b])
        members = case["lists"][li]
        name = CL.REFINE_LISTS[li] if case["n_parents"] else "flat"
        queue, rank = CL.queue_ranks(params, members, int(params[cur[b], 3]), case["perceptual"])
        where = []
        for who, ci in (("expected", int(case["expected"][b])), ("got", int(got[b]))):
            at = np.nonzero(members == ci)[0]
            if at.size:
                q = int(queue[at[0]])
                where.append(f"{who} {ci} {params[ci].tolist()} at list position {int(at[0])}, " +
                             (f"{('unclamped', 'clamped')[q]} queue rank {int(rank[at[0]])}" if q >= 0 else "not admissible"))
            else:
                where.append(f"{who} {ci} (not in the list)")
        g = int(case["group"][b])
        lines.append(f"block {int(b)} (list {name} of {members.size}, current {int(cur[b])} table {int(params[cur[b], 3])}, group: {CL.GROUPS[g]}"
                     + (f", pair {case['pair'][b].tolist()}" if g else "") + "): " + "; ".join(where))
    return "\n".join(lines)


@pytest.mark.parametrize("presorted", [True, False])
@pytest.mark.parametrize("perceptual", [1, 0])
@pytest.mark.parametrize("kind", CL.REFINE_KINDS)
def test_refine_long_lists(hip_ctx, kind, perceptual, presorted, request):
    # presorted: k_refine_sort_lists + k_refine_sorted (the default); otherwise the kernel that filters and classifies the lists as it reads them
    if not presorted:
        hip_ctx.set_tuning(refine_unsorted=1)
        request.addfinalizer(hip_ctx.set_tuning)   # back to the process defaults
    c = CL.refine_case(kind, perceptual)
    n, k = c["tiles"].shape[0], c["params"].shape[0]
    bufs = [hip_ctx.upload(c[name]) for name in ("tiles", "block_cluster", "params", "cand_offsets", "cand_indices", "block_parent")]
    d_out = hip_ctx.alloc(n * 4)
    try:
        hip_ctx.check(hip_ctx.lib.k_refine_endpoint_clusterization(hip_ctx.h, bufs[0], n, bufs[1], bufs[2], k, c["n_parents"], bufs[3], bufs[4], bufs[5], perceptual, d_out),
                      "k_refine")
        got = hip_ctx.download(d_out, (n,), np.uint32)
    finally:
        for p in bufs + [d_out]:
            hip_ctx.free(p)
    bad = np.nonzero(got != c["expected"])[0]
    assert bad.size == 0, f"{bad.size} of {n} blocks differ:\n" + _describe_refine(c, got, bad)
    assert (got != c["block_cluster"]).any(), "degenerate test: nothing moved"


@pytest.mark.parametrize("perceptual", [1, 0])
@pytest.mark.parametrize("kind", ["flat", "hier"])
def test_find_optimal_selector_clusters_long_lists(hip_ctx, kind, perceptual):
    """through bu_hip_k_find_optimal_selector_clusters, which lays the candidates' selector words out in list order first (the cand_words branch of the kernel)"""
    c = CL.fosc_case(kind, perceptual)
    n, k = c["tiles"].shape[0], c["selector_blocks"].shape[0]
    bufs = [hip_ctx.upload(c[name]) for name in ("tiles", "enc", "selector_blocks", "cand_offsets", "cand_indices", "block_parent")]
    d_out = hip_ctx.alloc(n * 4)
    try:
        hip_ctx.check(hip_ctx.lib.k_find_optimal_selector_clusters(hip_ctx.h, bufs[0], bufs[1], n, bufs[2], k, c["n_parents"], bufs[3], bufs[4], bufs[5], perceptual,
                                                                   c["chunk"], d_out), "k_fosc")
        got_idx = hip_ctx.download(d_out, (n,), np.uint32)
        got_enc = hip_ctx.download(bufs[1], (n, 8), np.uint8)
    finally:
        for p in bufs + [d_out]:
            hip_ctx.free(p)
    bad = np.nonzero(got_idx != c["expected_idx"])[0]
    lengths = [int(c["lists"][c["block_list"][b]].size) for b in bad[:8]]
    assert bad.size == 0, f"{bad.size} of {n} differ, first blocks {bad[:8]} (lists of {lengths}): got {got_idx[bad[:8]]} expected {c['expected_idx'][bad[:8]]}"
    assert (got_enc == c["expected_enc"]).all(), np.nonzero((got_enc != c["expected_enc"]).any(axis=1))[0][:8]


@pytest.mark.parametrize("perceptual", [1, 0])
def test_create_optimized_selector_codebook_chunk_edges(hip_ctx, perceptual):
    c = CL.cosc_case(perceptual)
    k = c["stale"].shape[0]
    bufs = [hip_ctx.upload(c[name]) for name in ("tiles", "enc", "offsets", "indices", "stale")]
    try:
        hip_ctx.check(hip_ctx.lib.k_create_optimized_selector_codebook(hip_ctx.h, bufs[0], bufs[1], k, bufs[2], bufs[3], perceptual, bufs[4]), "k_cosc")
        got = hip_ctx.download(bufs[4], (k, 8), np.uint8)
    finally:
        for p in bufs:
            hip_ctx.free(p)
    bad = np.nonzero((got != c["expected"]).any(axis=1))[0]     # all 8 bytes: stale bytes stay, in the colour bytes and in empty clusters
    named = {v: name for name, v in c["names"].items()}
    assert bad.size == 0, (f"{bad.size} of {k} clusters differ, first {[(int(b), named.get(int(b), 'seeded run'), int(c['offsets'][b]), int(c['offsets'][b + 1])) for b in bad[:6]]}: "
                           f"got {got[bad[:3]].tolist()} expected {c['expected'][bad[:3]].tolist()}")
