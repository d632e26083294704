"""The per-node host reference of the TSVQ (tests/native/tsvq_node_host.cpp: root and split of ONE node through the bodies of csrc/host/tsvq.h) tied to the
tree builder: the reference's loop (enc.h:1616-1660: root, pop the variance queue, split) replayed in Python over nothing but the shim's root() and split() and
a Python copy of the queue's tie rules must give the leaves and the parent cut of bu_host_tsvq -- which tests/test_host_logic.py pins to the real reference --
and of the reference itself where oracle/_ref is present. tests/test_gpu_tsvq_nodes.py compares the device's records with this shim."""
import ctypes as C

import numpy as np
import pytest

from helpers import TsvqNodes, csr_blob_split, have_ref, ref, ptr, u32p, u64p, f32p
from test_gpu_tsvq import _data, _endpoint_like

VP = C.c_void_p


class VarianceHeap:
    """bu::variance_heap (enc.h:1455-1544): sift-up moves past parents with priority <= new; sift-down prefers the right child only when strictly larger and
    stops when the moving entry is strictly larger than the chosen child. Priorities are float32 values held as Python floats (comparisons are exact)."""

    def __init__(self, index, priority):
        self.h = [None, (index, priority)]

    def __len__(self):
        return len(self.h) - 1

    def top(self):
        return self.h[1][0]

    def pop(self):
        h = self.h
        moving = h.pop()
        n = len(h) - 1
        if not n:
            return
        at = 1
        while 2 * at <= n:
            child = 2 * at
            if child < n and h[child][1] < h[child + 1][1]:
                child += 1
            if moving[1] > h[child][1]:
                break
            h[at] = h[child]
            at = child
        h[at] = moving

    def push(self, index, priority):
        h = self.h
        h.append(None)
        k = len(h) - 1
        while k >> 1 and not h[k >> 1][1] > priority:
            h[k] = h[k >> 1]
            k >>= 1
        h[k] = (index, priority)


def replay_tree(rows, weights, max_leaves):
    """tsvq<N>::generate + split (csrc/host/tsvq.h) over the shim -> the node table: dicts of members / left / right / codebook_index"""
    S = TsvqNodes(rows, weights)
    members = np.arange(rows.shape[0], dtype=np.uint32)
    r = S.root(members)
    nodes = [dict(var=float(r["var"]), weight=int(r["weight"]), origin=r["origin"].copy(), members=members, left=-1, right=-1, codebook_index=-1)]
    heap = VarianceHeap(0, nodes[0]["var"])
    leaves, next_index = 1, 0
    while len(heap) and leaves < max_leaves:
        ni = heap.top()
        heap.pop()
        nd = nodes[ni]
        if nd["members"].size <= 1:
            continue
        s, lm, rm = S.split(nd["members"], nd["weight"], nd["origin"])
        if not s["ok"]:
            continue
        nd["left"], nd["right"], nd["codebook_index"] = len(nodes), len(nodes) + 1, next_index
        next_index += 1
        for side, m in (("l", lm), ("r", rm)):
            var = float(s[side + "_var"])
            if var <= 0.0 and m.size > 1 and not (rows[m] == rows[m[0]]).all():
                var = float(np.float32(1e-4))   # enc.h:1766-1792
            nodes.append(dict(var=var, weight=int(s[side + "_weight"]), origin=s[side + "_centroid"].copy(), members=m, left=-1, right=-1, codebook_index=-1))
            if var > 0.0 and m.size > 1:
                heap.push(len(nodes) - 1, var)
        leaves += 1
    S.close()
    return nodes


def top_clusters(nodes, max_clusters):
    """tsvq<N>::top_clusters (enc.h:1598-1628)"""
    out, stack, ni = [], [], 0
    while True:
        cur = nodes[ni]
        if cur["left"] < 0 or 2 + cur["codebook_index"] > max_clusters:
            out.append(cur["members"])
            if not stack:
                return out
            ni = stack.pop()
            continue
        stack.append(cur["right"])
        ni = cur["left"]


def _lists(blob):
    offs, idx = csr_blob_split(blob)
    return [idx[offs[i]:offs[i + 1]].tolist() for i in range(offs.size - 1)]


def _inputs(kind):
    rng = np.random.default_rng({"sel": 11, "ep5": 12, "line": 13}[kind])
    if kind == "sel":
        v = _data("sel", 16, 3000, rng); k, p, wmax = 200, 16, 4096
    elif kind == "ep5":
        v = _endpoint_like("ep5", 2000, rng); k, p, wmax = 150, 8, 50
    else:
        v = _data("line", 6, 400, rng); k, p, wmax = 40, 4, 5   # 64 collinear points: degenerate projections, the half split, variances that round to <= 0
    w = rng.integers(1, wmax + 1, v.shape[0]).astype(np.uint64)
    return v, w, k, p


@pytest.mark.parametrize("kind", ["sel", "ep5", "line"])
def test_replayed_nodes_give_the_host_tree(kind):
    from basis_universal_amd import etc1s
    F = etc1s.load_frontend_library()
    v, w, k, p = _inputs(kind)
    n, dim = v.shape
    nodes = replay_tree(v, w, k)
    leaves = [nd["members"].tolist() for nd in nodes if nd["left"] < 0]
    parents = [m.tolist() for m in top_clusters(nodes, p)]
    assert len(leaves) > 1 and sorted(i for l in leaves for i in l) == list(range(n))
    cap = 4 * n + 4 * k + 100
    a = np.zeros(cap, np.uint32); b = np.zeros(cap, np.uint32)
    assert F.bu_host_tsvq(dim, v.ctypes.data_as(VP), w.ctypes.data_as(VP), n, k, p, a.ctypes.data_as(VP), cap, b.ctypes.data_as(VP), cap) == 1
    assert _lists(a) == leaves, "leaves differ from bu_host_tsvq"
    assert _lists(b) == parents, "parent cut differs from bu_host_tsvq"
    if have_ref():
        a3 = np.zeros(cap, np.uint32); b3 = np.zeros(cap, np.uint32)
        assert ref().ref_tsvq(dim, ptr(v, f32p), ptr(w, u64p), n, k, p, 0, ptr(a3, u32p), cap, ptr(b3, u32p), cap) == 1
        assert _lists(a3) == leaves and _lists(b3) == parents, "differs from the reference"


def test_root_of_a_sublist_is_the_root_of_that_training_set():
    """root(members) in list order = the root of a quantiser whose training set is rows[members] (what the partitioned build starts its sub-trees from), and
    an unsplittable node (two identical rows) reports ok = 0 with nothing else set."""
    rng = np.random.default_rng(5)
    v = _data("sel", 16, 500, rng); w = rng.integers(1, 1 << 30, v.shape[0]).astype(np.uint64)
    m = rng.permutation(v.shape[0])[:137].astype(np.uint32)
    a = TsvqNodes(v, w).root(m)
    b = TsvqNodes(v[m], w[m]).root(np.arange(m.size))
    assert a.tobytes() == b.tobytes()
    assert int(a["weight"]) == int(w[m].astype(object).sum()) and (a["origin"][16:] == 0).all() and a["pad"] == 0
    two = np.ones((2, 6), np.float32)
    s, lm, rm = TsvqNodes(two, np.array([3, 4], np.uint64)).split([0, 1], 7, two[0])
    assert s["ok"] == 0 and lm.size == 0 and rm.size == 0 and not np.frombuffer(s.tobytes(), np.uint8).any()
