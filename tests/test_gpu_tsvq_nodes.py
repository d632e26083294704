"""-m gpu: the TSVQ entry points of include/basisu_hip.h ONE NODE at a time. tests/test_gpu_tsvq.py compares whole trees; here every record field and every member
list of a round is compared, bit for bit, with the per-node host reference (tests/native/tsvq_node_host.cpp, tied to the tree builder and the reference by
tests/test_tsvq_node_host.py) or, for the integer bookkeeping, with numpy. The C ABI is driven directly through hip_ctx.lib. No tolerances anywhere: floats compare as
their uint32 bits.

Fields outside the comparison, and why: bu_tsvq_split::pad is written by no kernel; after ok == 0 the rest of a record is whatever the kernel had (only ok is
compared). Centroid / origin components dim..15 ARE defined -- the one-workgroup kernels store 0.0f there, the many-workgroup kernels copy their zero-initialised
control block -- so they are asserted to be +0.0f."""
import ctypes as C

import numpy as np
import pytest

from helpers import TsvqNodes, TSVQ_ROOT, TSVQ_NODE, TSVQ_SPLIT, TSVQ_SPAN
from test_gpu_tsvq import _data, _endpoint_like

pytestmark = pytest.mark.gpu
VP = C.c_void_p
NBUF = 4   # BU_TSVQ_BUFFERS


def vp(a):
    return a.ctypes.data_as(VP)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def pack_keys(v):
    """selector rows (values 0..3) -> one dword per row, component 0 in the top two bits"""
    keys = np.zeros(v.shape[0], np.uint32)
    for k in range(16):
        keys = (keys << np.uint32(2)) | v[:, k].astype(np.uint32)
    return keys


def sel_rows(n, seed, draw=None):
    """exactly n distinct selector rows in ascending order"""
    v = _data("sel", 16, draw or (n + n // 8 + 8), np.random.default_rng(seed))
    assert v.shape[0] >= n
    return np.ascontiguousarray(v[:n])


def line_rows(dim, n):
    """n distinct collinear points (the `line` data of test_gpu_tsvq.py with as many distinct points as asked for)"""
    t = np.arange(n, dtype=np.float32)
    return np.ascontiguousarray(np.tile(t[:, None], (1, dim)) * np.float32(0.25))


# ----------------------------------------------------------------------------- the device side

class Quantiser:
    """one bu_tsvq on the session's context; mode: packed | float | packed_device | endpoint_device (rows = (keys, group offsets) there)"""

    def __init__(self, ctx, mode, rows, weights=None):
        self.ctx, self.L, self.mode = ctx, ctx.lib, mode
        self.root = np.zeros(1, TSVQ_ROOT)
        self._dev = []
        if mode == "packed":
            self.n = rows.shape[0]
            self.q = self.L.tsvq_create_packed16(ctx.h, vp(pack_keys(rows)), vp(weights), self.n, vp(self.root))
        elif mode == "packed_device":
            self.n = rows.shape[0]
            self._dev = [ctx.upload(pack_keys(rows)), ctx.upload(weights)]
            self.q = self.L.tsvq_create_packed16_device(ctx.h, self._dev[0], self._dev[1], self.n, vp(self.root))
        elif mode == "endpoint_device":
            keys, goffs = rows
            self.n = keys.shape[0]
            self._dev = [ctx.upload(keys), ctx.upload(goffs)]
            self.q = self.L.tsvq_create_endpoint_device(ctx.h, self._dev[0], self._dev[1], self.n, vp(self.root))
        else:
            self.n = rows.shape[0]
            self.q = self.L.tsvq_create(ctx.h, rows.shape[1], vp(np.ascontiguousarray(rows, np.float32)), vp(weights), self.n, vp(self.root))
        assert self.q, self.L.last_error(ctx.h)
        self.root = self.root[0]

    def split(self, nodes):
        out = np.zeros(nodes.size, TSVQ_SPLIT)
        assert self.L.tsvq_split(self.ctx.h, self.q, vp(nodes), nodes.size, vp(out)) == 1, self.L.last_error(self.ctx.h)
        return out

    def split_deep(self, nodes, levels):
        out = np.zeros(nodes.size, TSVQ_SPLIT)
        deep = np.zeros(max(nodes.size * ((2 << levels) - 2), 1), TSVQ_SPLIT)
        deep["ok"] = 0xDEAD   # every slot must be written
        assert self.L.tsvq_split_deep(self.ctx.h, self.q, vp(nodes), nodes.size, vp(out), levels, vp(deep)) == 1, self.L.last_error(self.ctx.h)
        return out, deep

    def roots(self, nodes):
        out = np.zeros(nodes.size, TSVQ_ROOT)
        out["pad"] = 7
        assert self.L.tsvq_roots(self.ctx.h, self.q, vp(nodes), nodes.size, vp(out)) == 1, self.L.last_error(self.ctx.h)
        return out

    def members(self, buf, start, count):
        out = np.full(count, 0xFFFFFFFF, np.uint32)
        assert self.L.tsvq_read_members(self.ctx.h, self.q, buf, start, count, vp(out)) == 1
        return out

    def close(self):
        if self.q:
            self.L.tsvq_destroy(self.ctx.h, self.q)
            self.q = None
        for p in self._dev:
            self.ctx.free(p)
        self._dev = []


@pytest.fixture
def make(hip_ctx, request):
    """make(mode, rows, weights, **tuning) -> Quantiser created under that tuning; everything is destroyed and the tuning reset afterwards"""
    made = []
    request.addfinalizer(hip_ctx.set_tuning)   # (runs last: finalizers run in reverse order)
    request.addfinalizer(lambda: [q.close() for q in made])

    def _make(mode, rows, weights=None, **tuning):
        hip_ctx.set_tuning(**tuning)   # copied into the quantiser when it is created
        made.append(Quantiser(hip_ctx, mode, rows, weights))
        return made[-1]
    return _make


# ----------------------------------------------------------------------------- the host side

class HNode:
    """a node of the host trace: where its list lives, the list, what its parent's record said about it"""

    def __init__(self, buf, start, members, weight, origin, var=None):
        self.buf, self.start, self.members, self.weight, self.origin, self.var = buf, start, members, int(weight), np.array(origin, np.float32), var
        self.count = members.size
        self.rec = self.left = self.right = None

    def record(self, pad=0):
        r = np.zeros(1, TSVQ_NODE)[0]
        r["buf"], r["start"], r["count"], r["pad"], r["weight"], r["origin"] = self.buf, self.start, self.count, pad, self.weight, self.origin
        return r

    def host_split(self, S):
        """the shim's split of this node (once) -> its children as HNodes (None where there is no split)"""
        if self.rec is None:
            self.rec, lm, rm = S.split(self.members, self.weight, self.origin)
            if self.rec["ok"]:
                b = (self.buf + 1) % NBUF
                self.left = HNode(b, self.start, lm, self.rec["l_weight"], self.rec["l_centroid"], self.rec["l_var"])
                self.right = HNode(b, self.start + lm.size, rm, self.rec["r_weight"], self.rec["r_centroid"], self.rec["r_var"])
        return self.left, self.right

    def queued_var(self):
        """the variance the tree driver queues this child with (enc.h:1766-1792: 1e-4 for a non-positive variance of a node with differing members)"""
        v = np.float32(self.var)
        return np.float32(1e-4) if v <= 0 and self.count > 1 else v


def records(nodes, pads=None):
    out = np.zeros(len(nodes), TSVQ_NODE)
    for i, nd in enumerate(nodes):
        out[i] = nd.record(pads[i] if pads else 0)
    return out


def host_rounds(S, n, rounds):
    """[batch of round 1 (the root), batch of round 2 (its children), ...]: every node of two members and more of the generation before, all split by the shim"""
    r = S.root(np.arange(n, dtype=np.uint32))
    level, out = [HNode(0, 0, np.arange(n, dtype=np.uint32), r["weight"], r["origin"], r["var"])], []
    for _ in range(rounds):
        level = [nd for nd in level if nd.count >= 2]
        if not level:
            break
        out.append(level)
        level = [c for nd in level for c in nd.host_split(S) if c is not None]
    return r, out


def assert_root(got, exp, dim, what):
    assert got["weight"] == exp["weight"], what
    assert (bits(got["origin"][:dim]) == bits(exp["origin"][:dim])).all() and bits(got["var"]) == bits(exp["var"]), f"{what}: {got} != {exp}"
    assert (bits(got["origin"][dim:]) == 0).all(), what   # the kernels store 0.0f there
    assert got["pad"] == 0, f"{what}: a record still flagged for the next kernel variant"


def assert_split(got, nd, dim, what):
    """the device's record `got` of host node nd (already split by the shim)"""
    exp = nd.rec
    assert got["ok"] == exp["ok"], f"{what}: ok {got['ok']} != {exp['ok']}"
    if not exp["ok"]:
        return
    for f in ("l_count", "r_count", "l_weight", "r_weight"):
        assert got[f] == exp[f], f"{what}: {f} {got[f]} != {exp[f]}"
    for f in ("l_var", "r_var"):
        assert bits(got[f]) == bits(exp[f]), f"{what}: {f} {got[f]!r} != {exp[f]!r}"
    for f in ("l_centroid", "r_centroid"):
        assert (bits(got[f][:dim]) == bits(exp[f][:dim])).all(), f"{what}: {f} {got[f][:dim]} != {exp[f][:dim]}"
        assert (bits(got[f][dim:]) == 0).all(), f"{what}: {f}[{dim}:] not +0.0f"


def assert_lists(q, nd, what):
    """the children's lists of host node nd where the header puts them, the node's own list untouched"""
    own = q.members(nd.buf, nd.start, nd.count)
    assert (own == nd.members).all(), f"{what}: the node's own span changed"
    if not nd.rec["ok"]:
        return
    b, lc, rc = (nd.buf + 1) % NBUF, int(nd.rec["l_count"]), int(nd.rec["r_count"])
    gl, gr = q.members(b, nd.start, lc), q.members(b, nd.start + lc, rc)
    assert (gl == nd.left.members).all() and (gr == nd.right.members).all(), f"{what}: child lists differ from the host's"
    # without any reference: each child keeps the parent's list order, and the two partition the parent's list
    pos = np.full(q.n, -1, np.int64); pos[own] = np.arange(own.size)
    assert (np.diff(pos[gl]) > 0).all() and (np.diff(pos[gr]) > 0).all() and (pos[gl] >= 0).all() and (pos[gr] >= 0).all(), what
    assert lc + rc == nd.count and np.array_equal(np.sort(np.concatenate([gl, gr])), np.sort(own)), what


def check_rounds(q, S, dim, rounds=3, what=""):
    """root + `rounds` rounds (batches of 1, 2, 4 ... nodes) on the device against the shim -> (host root, host batches, the device's records as bytes)"""
    hroot, batches = host_rounds(S, q.n, rounds)
    assert_root(q.root, hroot, dim, f"{what} root")
    seen = [q.root.tobytes()[:76]]
    for r, batch in enumerate(batches):
        got = q.split(records(batch))
        for i, nd in enumerate(batch):
            assert_split(got[i], nd, dim, f"{what} round {r + 1} node {i} (buf {nd.buf} start {nd.start} count {nd.count})")
        for i, nd in enumerate(batch):
            assert_lists(q, nd, f"{what} round {r + 1} node {i}")
            seen.append(b"".join(got[i][f].tobytes() for f in got.dtype.names if f != "pad") if nd.rec["ok"] else b"0")
    return hroot, batches, seen


def weights_for(kind, n, rng):
    if kind == "ones":
        return np.ones(n, np.uint64)
    if kind == "w4096":
        return rng.integers(1, 4097, n).astype(np.uint64)
    if kind == "w3e9":   # weights past 2^24: (float)weight rounds, sums leave the exact range
        w = rng.integers(1, 4097, n).astype(np.uint64); w[rng.integers(0, n, 5)] = 3_000_000_000
        return w
    if kind == "heavy_one":   # one member of >= 2^22 in an otherwise light node
        w = rng.integers(1, 4, n).astype(np.uint64); w[n // 3] = (1 << 22) + 12345
        return w
    if kind == "pow2":   # test_gpu_tsvq.py's sel_pow2 pattern scaled to n: whole 256-member blocks of 2^16, then of 2^20, then ones
        w = np.ones(n, np.uint64); a = 256 * max(1, n // 1200); w[:a * 4] = 65536; w[a * 4: a * 4 + max(256, a // 2)] = 1 << 20
        return w
    return rng.integers(1, int(kind) + 1, n).astype(np.uint64)   # "2^k" as a number


# ----------------------------------------------------------------------------- a. the one-workgroup split kernel

NARROW = [("packed", "sel", 1, "w4096"), ("packed", "sel", 2, "w4096"), ("packed", "sel", 3, "w4096"), ("packed", "sel", 257, "w4096"), ("packed", "sel", 700, "w4096"),
          ("float", "sel", 1, "w4096"), ("float", "sel", 2, "w4096"), ("float", "sel", 3, "w4096"), ("float", "sel", 257, "w4096"), ("float", "sel", 700, "w4096"),
          ("packed", "sel", 32768 + 40, "w4096"),   # the exact pass's `big = count > 512 * 64` branch
          ("packed", "sel", 700, "ones"), ("packed", "sel", 700, "w3e9"), ("float", "sel", 700, "w3e9"),
          ("packed", "sel", 700, 2 ** 44), ("packed", "sel", 700, 2 ** 50),   # back through the ok == 2 redo into the chained variant
          ("packed", "sel", 700, "heavy_one"), ("float", "sel", 700, "heavy_one"),
          ("float", "ep5", 700, "w4096"), ("float", "ep5_dark", 700, 1 << 20), ("float", "line6", 64, 5), ("float", "line16", 64, 5)]


def narrow_input(kind, n, wkind):
    rng = np.random.default_rng(1000 + n)
    if kind == "sel":
        v = sel_rows(n, 1000 + n)
    elif kind.startswith("line"):   # the 64 collinear points of test_gpu_tsvq.py's `line` data (degenerate projections -> the half split)
        v = line_rows(int(kind[4:]), n)
    else:
        v = _endpoint_like(kind, n, rng)
    return v, weights_for(wkind, v.shape[0], rng)


@pytest.mark.parametrize("mode,kind,n,wkind", NARROW, ids=lambda x: str(x))
def test_one_workgroup_split_rounds_match_the_host_node_for_node(make, mode, kind, n, wkind):
    """k_tsvq_split / k_tsvq_split_dense: root, then 3 rounds of 1, 2 and 4 nodes (start offsets, buffers 0 -> 1 -> 2 -> 3)"""
    v, w = narrow_input(kind, n, wkind)
    S = TsvqNodes(v, w)
    dim = v.shape[1]
    seen = {}
    for dense in ((1, 0) if mode == "packed" else (257,)):   # 1: the 128-register build for every batch, 0: never
        q = make(mode, v, w, tsvq_wide_min=0, tsvq_wide6_min=0, tsvq_dense_min=dense)
        _, batches, seen[dense] = check_rounds(q, S, dim, what=f"dense_min={dense}")
    if v.shape[0] >= 3:
        assert len(batches) >= 2
    if len(seen) == 2:
        assert seen[1] == seen[0], "the two builds of the split kernel differ"


@pytest.mark.parametrize("knobs", [dict(tsvq_zero_copy=0), dict(tsvq_chained_only=1)], ids=str)
@pytest.mark.parametrize("mode", ["packed", "float"])
def test_staged_records_and_chained_only_rounds(make, mode, knobs):
    v, w = narrow_input("sel", 700, "w3e9")
    check_rounds(make(mode, v, w, tsvq_wide_min=0, tsvq_wide6_min=0, **knobs), TsvqNodes(v, w), 16, what=str(knobs))


# (No node of identical rows here: the peel pass of tsvq_split_body sends "the first member" right by POSITION -- the API's rows are distinct -- so two identical rows
# come back ok = 1 where prep_split / refine_split return false. Outside the contract, bounded, and not something these tests can hold the kernel to.)


def tie_input(kind):
    """a member EXACTLY half way between the two centroids of the first two-means pass: refine_split sends it right (dl >= dr, enc.h:1988)"""
    if kind == "float6":   # left {-3, -1} x 0.25 with weights 2, 2 -> -0.5; right {0, 2, 4} x 0.25 with weights 1 -> 0.5; the member at 0 ties
        t = np.array([-3, -1, 0, 2, 4], np.float32) * np.float32(0.25)
        return np.ascontiguousarray(np.tile(t[:, None], (1, 6))), np.array([2, 2, 1, 1, 1], np.uint64), 2
    v = np.zeros((4, 16), np.float32); v[:, 0] = [0, 1, 2, 3]   # left {0}, right {1, 2, 3} -> 2; the member at 1 ties
    return v, np.array([10, 1, 1, 1], np.uint64), 1


@pytest.mark.parametrize("mode,kind", [("packed", "sel16"), ("float", "sel16"), ("float", "float6")])
def test_a_member_at_equal_distances_goes_right(make, mode, kind):
    v, w, tie = tie_input(kind)
    _, batches, _ = check_rounds(make(mode, v, w, tsvq_wide_min=0, tsvq_wide6_min=0), TsvqNodes(v, w), v.shape[1], rounds=1)
    nd = batches[0][0]
    assert nd.rec["ok"] == 1 and nd.right.members[0] == tie and nd.left.members[-1] == tie - 1


# ----------------------------------------------------------------------------- b. the many-workgroup paths

WIDE = [("ones", 2050, "ones", dict(tsvq_wide_cov_min=0, tsvq_windows=2)),   # 3 x weight < 2^24: the side_chains_exact shortcut
        ("ones_hybrid", 2050, "ones", dict()),                               # default tsvq_wide_cov_min: the covariance pass chained
        ("w2^20", 2050, 1 << 20, dict(tsvq_wide_cov_min=0)), ("w2^20_hybrid", 2050, 1 << 20, dict()),   # chain totals pass 2^24: real walks
        ("w2^20_nowin", 2050, 1 << 20, dict(tsvq_wide_cov_min=0, tsvq_windows=2)),
        ("pow2", 12000, "pow2", dict(tsvq_wide_cov_min=0)),
        ("w2^50", 2050, 2 ** 50, dict(tsvq_wide_cov_min=0)),                # handed back with ok == 2 and redone
        ("windows", 20000, 4096, dict(tsvq_wide_cov_min=0, tsvq_windows=1))]  # 79 blocks: a 64-block window is taken


@pytest.mark.parametrize("name,n,wkind,knobs", WIDE, ids=[c[0] for c in WIDE])
def test_wide_packed_split_rounds_match_the_host_node_for_node(make, name, n, wkind, knobs):
    """tsvq_wide_kernels.hip next to the one-workgroup kernel in one batch (side stream, narrow-first result order)"""
    wide_min = 512
    v = sel_rows(n, 2000 + n); w = weights_for(wkind, n, np.random.default_rng(2000 + n))
    S = TsvqNodes(v, w)
    q = make("packed", v, w, tsvq_wide_min=wide_min, **knobs)
    _, batches, _ = check_rounds(q, S, 16, rounds=5 if name == "pow2" else 3, what=name)   # (pow2: the first batch with a narrow node is the fifth)
    counts = [[nd.count for nd in b] for b in batches]
    assert counts[0][0] >= wide_min and all(c >= wide_min for c in counts[1]), counts   # the root and its children are wide nodes
    if name == "windows":
        assert (counts[0][0] + 255) // 256 > 64
    else:
        if n < 3000:
            assert 3 <= (counts[1][0] + 255) // 256 and (counts[0][0] + 255) // 256 <= 12
        assert any(min(b) < wide_min <= max(b) for b in counts), f"no batch mixes wide and narrow nodes: {counts}"
    if wkind == "ones":
        assert 3 * n < 1 << 24
    if wkind == 1 << 20:
        assert int(w.astype(object).sum()) > 1 << 24


WIDE6 = [("ep5_dark", 1 << 34), ("line", 5), ("ep5", 4096)]


@pytest.mark.parametrize("kind,wmax", WIDE6, ids=[c[0] for c in WIDE6])
def test_wide6_split_rounds_match_the_host_node_for_node(make, kind, wmax):
    """tsvq_wide6_kernels.hip; the dark data for the double accumulators' block test, the line for degenerate projections (handed back with ok == 2)"""
    wide_min = 512
    rng = np.random.default_rng(77)
    v = line_rows(6, 2050) if kind == "line" else _endpoint_like(kind, 12000 if kind == "ep5_dark" else 2050, rng)
    n = v.shape[0]
    assert 1500 <= n <= 3000, n
    w = rng.integers(1, wmax + 1, n).astype(np.uint64)
    if kind == "ep5_dark":
        w[rng.random(n) < 0.7] = 1
    S = TsvqNodes(v, w)
    q = make("float", v, w, tsvq_wide6_min=wide_min)
    _, batches, _ = check_rounds(q, S, 6, what=kind)
    counts = [[nd.count for nd in b] for b in batches]
    assert counts[0][0] >= wide_min and max(counts[1]) >= wide_min, counts
    assert any(min(b) < wide_min <= max(b) for b in counts), f"no batch mixes wide and narrow nodes: {counts}"


# ----------------------------------------------------------------------------- c. bu_hip_tsvq_roots

def live_spans(batches):
    """every list that is intact after the rounds: the batches' nodes and the last batch's children (one-member ones included)"""
    spans = [nd for b in batches for nd in b]
    return spans + [c for nd in batches[-1] for c in (nd.left, nd.right) if c is not None]


@pytest.mark.parametrize("mode,kind,wkind,wide_min", [("packed", "sel", "w4096", 0), ("packed", "sel", "w4096", 512), ("packed", "sel", 2 ** 50, 512), ("packed", "sel", 2 ** 50, 0),
                                                     ("float", "sel", "w3e9", 0), ("float", "ep5", "w4096", 0)], ids=str)
def test_span_roots_match_the_host(make, mode, kind, wkind, wide_min):
    rng = np.random.default_rng(31)
    v = sel_rows(2050 if wide_min else 700, 31) if kind == "sel" else _endpoint_like(kind, 700, rng)
    n, dim = v.shape
    w = weights_for(wkind, n, rng)
    S = TsvqNodes(v, w)
    q = make(mode, v, w, tsvq_wide_min=wide_min, tsvq_wide6_min=0)
    _, batches, _ = check_rounds(q, S, dim, rounds=2)
    spans = live_spans(batches)
    assert len(spans) >= 6
    if wide_min:
        assert any(s.count >= wide_min for s in spans) and any(s.count < wide_min for s in spans)
    got = q.roots(records(spans))
    for i, s in enumerate(spans):
        assert_root(got[i], S.root(s.members), dim, f"span {i} (buf {s.buf} start {s.start} count {s.count})")
        assert int(got[i]["weight"]) == int(w[s.members].astype(object).sum())


def test_span_roots_refuse_spans_outside_the_training_set(make, hip_ctx):
    v, w = narrow_input("sel", 257, "w4096")
    q = make("packed", v, w)
    good = records([HNode(0, 0, np.arange(257, dtype=np.uint32), 0, np.zeros(16))])
    for field, value in (("buf", NBUF), ("count", 0), ("start", 1)):
        bad = np.concatenate([good, good]); bad[1][field] = value
        out = np.zeros(2, TSVQ_ROOT)
        assert hip_ctx.lib.tsvq_roots(hip_ctx.h, q.q, vp(bad), 2, vp(out)) == 0
        assert "span outside the training set" in hip_ctx.lib.last_error(hip_ctx.h)
        assert not np.frombuffer(out.tobytes(), np.uint8).any(), "a refused call wrote a record"
    assert_root(q.roots(good)[0], TsvqNodes(v, w).root(np.arange(257)), 16, "after the refusals")


def test_packed16_device_equals_packed16(make):
    v, w = narrow_input("sel", 700, "w3e9")
    a, b = make("packed", v, w), make("packed_device", v, w)
    assert a.root.tobytes() == b.root.tobytes()
    S = TsvqNodes(v, w)
    check_rounds(b, S, 16, rounds=1, what="device arrays")
    check_rounds(a, S, 16, rounds=1, what="host arrays")


# ----------------------------------------------------------------------------- d. bu_hip_tsvq_split_deep

def expected_deep(S, batch, pads, levels, attempted_root):
    """{slot index: HNode (split by the shim) or None for ok == 3} by the rule of include/basisu_hip.h; attempted_root[i] False = node i took the many-workgroup path"""
    n, out = len(batch), {}
    cur = [(nd if attempted_root[i] else None) for i, nd in enumerate(batch)]   # generation g - 1, index i * 2^(g-1) + p
    for g in range(1, levels + 1):
        w, nxt = 1 << g, []
        for k in range(n * w):
            parent, floor = cur[k >> 1], np.array([pads[k >> g]], np.uint32).view(np.float32)[0]
            child = None
            if parent is not None and parent.rec["ok"] == 1:
                c = (parent.left, parent.right)[k & 1]
                qv = c.queued_var()
                if c.count > 1 and qv > 0 and qv >= floor:
                    c.host_split(S)
                    child = c
            out[n * (w - 2) + k] = child
            nxt.append(child)
        cur = nxt
    return out


def check_deep(q, S, dim, batch, pads, levels, wide_min=0):
    for nd in batch:
        nd.host_split(S)
    got, deep = q.split_deep(records(batch, pads), levels)
    narrow = [not (wide_min and nd.count >= wide_min) for nd in batch]
    for i, nd in enumerate(batch):
        assert_split(got[i], nd, dim, f"deep batch node {i}")
    exp = expected_deep(S, batch, pads, levels, narrow)
    assert len(exp) == len(batch) * ((2 << levels) - 2)
    for slot, nd in exp.items():
        if nd is None:
            assert deep[slot]["ok"] == 3, f"slot {slot}: ok {deep[slot]['ok']}, expected 3 (not attempted)"
        else:
            assert_split(deep[slot], nd, dim, f"deep slot {slot}")
    # the lists of every generation that was split: the batch's own and children (buf, buf + 1), the descendants' (buf + 2, buf + 3)
    for i, nd in enumerate(batch):
        assert_lists(q, nd, f"deep batch node {i}")
    for slot, nd in exp.items():
        if nd is not None:
            assert_lists(q, nd, f"deep slot {slot}")
    return exp, deep


@pytest.mark.parametrize("mode", ["packed", "float"])
@pytest.mark.parametrize("levels", [1, 2])
def test_deep_round_slots_and_floor(make, mode, levels):
    """three nodes at different starts; node 1 carries a floor between its children's variances: exactly one child is attempted, nothing below the other"""
    v, w = narrow_input("sel", 700, "w4096")
    S = TsvqNodes(v, w)
    q = make(mode, v, w, tsvq_wide_min=0, tsvq_wide6_min=0)
    _, batches, _ = check_rounds(q, S, 16, rounds=2)
    batch = [c for nd in batches[1] for c in (nd.left, nd.right)][:3]   # grandchildren of the root, in buffer 2
    assert len(batch) == 3 and len({nd.start for nd in batch}) == 3 and all(nd.count > 8 for nd in batch)
    l, r = batch[1].host_split(S)
    lo, hi = sorted([l.queued_var(), r.queued_var()])
    floor = np.float32((np.float64(lo) + np.float64(hi)) / 2)
    assert 0 < lo < floor < hi and l.count > 1 and r.count > 1
    pads = [0, int(np.array([floor], np.float32).view(np.uint32)[0]), 0]
    exp, deep = check_deep(q, S, 16, batch, pads, levels)
    w1 = 2
    below = 2 + (0 if l.queued_var() < floor else 1)   # generation 1 slot of node 1's child below the floor: n * 0 + 1 * 2 + side
    assert exp[below] is None and exp[below ^ 1] is not None and deep[below]["ok"] == 3 and deep[below ^ 1]["ok"] == 1
    assert sum(exp[k] is not None for k in range(3 * w1)) == 5   # everything else of generation 1 is attempted
    if levels == 2:
        kids = [3 * 2 + 2 * below, 3 * 2 + 2 * below + 1]
        assert all(exp[k] is None and deep[k]["ok"] == 3 for k in kids), "descendants of an unattempted node"
        assert sum(exp[k] is not None for k in range(6, 18)) >= 8


def far_line_input():
    """48 collinear points far from the origin: the double sum minus the float quotient cancels to a NEGATIVE variance for children of a dozen members"""
    v = np.ascontiguousarray(np.tile(((np.arange(48) + 20000).astype(np.float32) * np.float32(0.25))[:, None], (1, 6)))
    return v, np.random.default_rng(0).integers(1, 4097, 48).astype(np.uint64)


def test_deep_round_attempts_children_of_non_positive_variance(make):
    """the reference queues a child of differing members whose variance came out <= 0 with 1e-4 (enc.h:1766-1792): the deep round must attempt it too"""
    v, w = far_line_input()
    S = TsvqNodes(v, w)
    q = make("float", v, w, tsvq_wide6_min=0)
    _, batches, _ = check_rounds(q, S, 6, rounds=1)
    batch = [c for c in (batches[0][0].left, batches[0][0].right)]
    exp, deep = check_deep(q, S, 6, batch, [0, 0], 2)
    odd = [k for k in range(4) if exp[k] is not None and np.float32(exp[k].var) <= 0 and exp[k].count > 1]
    assert odd and all(deep[k]["ok"] in (0, 1) for k in odd), "no attempted child with a non-positive variance in this input"


def test_deep_round_leaves_wide_nodes_to_ordinary_rounds(make):
    v = sel_rows(2050, 4050); w = weights_for("w4096", 2050, np.random.default_rng(4050))
    S = TsvqNodes(v, w)
    q = make("packed", v, w, tsvq_wide_min=512)
    _, batches, _ = check_rounds(q, S, 16, rounds=2)
    batch = [c for nd in batches[1] for c in (nd.left, nd.right)]
    assert any(nd.count >= 512 for nd in batch) and any(2 <= nd.count < 512 for nd in batch), [nd.count for nd in batch]
    exp, deep = check_deep(q, S, 16, batch, [0] * len(batch), 1, wide_min=512)
    for i, nd in enumerate(batch):
        if nd.count >= 512:
            assert deep[2 * i]["ok"] == 3 and deep[2 * i + 1]["ok"] == 3


def test_deep_round_argument_checks(make, hip_ctx):
    v, w = narrow_input("sel", 257, "w4096")
    q = make("packed", v, w)
    node = records([HNode(0, 0, np.arange(257, dtype=np.uint32), q.root["weight"], q.root["origin"])])
    out = np.zeros(1, TSVQ_SPLIT); deep = np.zeros(14, TSVQ_SPLIT)
    L = hip_ctx.lib
    assert L.tsvq_split_deep(hip_ctx.h, q.q, vp(node), 1, vp(out), 3, vp(deep)) == 0 and "levels" in L.last_error(hip_ctx.h)
    assert L.tsvq_split_deep(hip_ctx.h, q.q, vp(node), 1, vp(out), 1, None) == 0 and "no array for the deeper generations" in L.last_error(hip_ctx.h)
    assert out["ok"][0] == 0 and not np.frombuffer(deep.tobytes(), np.uint8).any()


# ----------------------------------------------------------------------------- 3. records that are no span are refused before anything is launched

@pytest.mark.parametrize("deep", [False, True])
def test_split_refuses_spans_outside_the_training_set(make, hip_ctx, deep):
    v, w = narrow_input("sel", 257, "w4096")
    S = TsvqNodes(v, w)
    q = make("packed", v, w)
    hroot, batches = host_rounds(S, 257, 1)
    good = records(batches[0])
    L = hip_ctx.lib
    for field, value in (("buf", NBUF), ("count", 0), ("start", 1)):
        bad = np.concatenate([good, good]); bad[1][field] = value
        out = np.zeros(2, TSVQ_SPLIT); dp = np.zeros(4, TSVQ_SPLIT)
        r = L.tsvq_split_deep(hip_ctx.h, q.q, vp(bad), 2, vp(out), 1, vp(dp)) if deep else L.tsvq_split(hip_ctx.h, q.q, vp(bad), 2, vp(out))
        assert r == 0 and "span outside the training set" in L.last_error(hip_ctx.h), (field, r, L.last_error(hip_ctx.h))
        assert not np.frombuffer(out.tobytes(), np.uint8).any() and not np.frombuffer(dp.tobytes(), np.uint8).any(), "a refused call wrote a record"
    got = q.split(good)   # the quantiser is as it was
    assert_split(got[0], batches[0][0], 16, "after the refusals")
    assert_lists(q, batches[0][0], "after the refusals")


# ----------------------------------------------------------------------------- e. spans

def test_scatter_and_finish_spans(make, hip_ctx):
    n = 3000
    v = sel_rows(n, 8100); rng = np.random.default_rng(81)
    w = weights_for("w4096", n, rng)
    q = make("packed", v, w, tsvq_wide_min=0)
    _, batches, _ = check_rounds(q, TsvqNodes(v, w), 16)
    leaves = [c for nd in batches[2] for c in (nd.left, nd.right)]
    assert len(leaves) == 8
    leaves[-1] = HNode(leaves[-1].buf, leaves[-1].start, leaves[-1].members[:1], 0, np.zeros(16))   # a span of one member; the leaf's other members lie in no span
    spans = np.zeros(8, TSVQ_SPAN)
    for i, s in enumerate(leaves):
        spans[i] = (s.buf, s.start, s.count, 100 + 7 * i)
    covered = np.concatenate([s.members for s in leaves])
    assert covered.size < n and np.unique(covered).size == covered.size
    FILL = 0xABCD1234
    L, h = hip_ctx.lib, hip_ctx.h
    dev = []

    def filled(count):
        dev.append(hip_ctx.upload(np.full(count, FILL, np.uint32)))
        return dev[-1]
    try:
        d_out = filled(n)
        assert L.tsvq_scatter_spans(h, q.q, vp(spans), 8, d_out) == 1, L.last_error(h)
        exp = np.full(n, FILL, np.uint32)
        for i, s in enumerate(leaves):
            exp[s.members] = 100 + 7 * i
        assert (hip_ctx.download(d_out, n, np.uint32) == exp).all()
        sizes = rng.integers(1, 6, n).astype(np.uint32)
        goffs = np.zeros(n + 1, np.uint32); goffs[1:] = np.cumsum(sizes)
        d_goffs = hip_ctx.upload(goffs); dev.append(d_goffs)
        leaf_exp = np.full(n, FILL, np.uint32); first_exp = np.full(n, FILL, np.uint32); size_exp = np.zeros(8, np.uint32)
        for i, s in enumerate(leaves):
            leaf_exp[s.members] = i
            first_exp[s.members] = np.concatenate([[0], np.cumsum(sizes[s.members])[:-1]])   # the groups of the members in front, in list order
            size_exp[i] = sizes[s.members].sum()
        for with_parent, with_groups in ((True, True), (False, True), (True, False)):
            d_leaf, d_parent, d_first, d_sizes = filled(n), filled(n), filled(n), filled(8)
            assert L.tsvq_finish_spans(h, q.q, vp(spans), 8, d_leaf, d_parent if with_parent else None, d_goffs if with_groups else None,
                                       d_first if with_groups else None, d_sizes if with_groups else None) == 1, L.last_error(h)
            assert (hip_ctx.download(d_leaf, n, np.uint32) == leaf_exp).all()
            assert (hip_ctx.download(d_parent, n, np.uint32) == (exp if with_parent else FILL)).all()
            assert (hip_ctx.download(d_first, n, np.uint32) == (first_exp if with_groups else FILL)).all()
            assert (hip_ctx.download(d_sizes, 8, np.uint32) == (size_exp if with_groups else FILL)).all()
    finally:
        for p in dev:
            hip_ctx.free(p)


# ----------------------------------------------------------------------------- f. bu_hip_tsvq_create_endpoint_device

def test_endpoint_device_rows_and_weights(make, hip_ctx):
    rng = np.random.default_rng(61)
    lo = rng.integers(0, 32, (2300, 3)); hi = np.minimum(31, lo + rng.integers(0, 12, (2300, 3)))
    c5 = np.concatenate([lo, hi], axis=1)
    byte = np.unique((c5 << 3) | (c5 >> 2), axis=0).astype(np.uint64)   # lexicographic = ascending keys
    n = byte.shape[0]
    assert 1800 <= n <= 2300
    keys = np.zeros(n, np.uint64)
    for c in range(6):   # low r,g,b in bits 47..24, high r,g,b in bits 23..0
        keys |= byte[:, c] << np.uint64(40 - 8 * c)
    assert (np.diff(keys.astype(np.int64)) > 0).all()
    sizes = rng.integers(1, 7, n).astype(np.uint32)
    goffs = np.zeros(n + 1, np.uint32); goffs[1:] = np.cumsum(sizes)
    rows = np.ascontiguousarray(byte.astype(np.float32) * np.float32(1.0 / 255.0))   # frontend.cpp:846-851
    w = (2 * sizes).astype(np.uint64)
    S = TsvqNodes(rows, w)
    qd = make("endpoint_device", (keys, goffs), tsvq_wide6_min=0)
    qh = make("float", rows, w, tsvq_wide6_min=0)
    assert qd.root.tobytes() == qh.root.tobytes()
    _, _, seen_d = check_rounds(qd, S, 6, rounds=2, what="rows made on the device")
    _, _, seen_h = check_rounds(qh, S, 6, rounds=2, what="rows from the host")
    assert seen_d == seen_h
    root = np.zeros(1, TSVQ_ROOT)
    d_keys = hip_ctx.upload(keys)
    try:
        for a, b in ((None, d_keys), (d_keys, None)):
            assert not hip_ctx.lib.tsvq_create_endpoint_device(hip_ctx.h, a, b, n, vp(root))
            assert "null pointer" in hip_ctx.lib.last_error(hip_ctx.h)
    finally:
        hip_ctx.free(d_keys)


# ----------------------------------------------------------------------------- g. the multi-GPU exchange on one GPU

def test_exchange_pack_and_unpack_between_two_quantisers(make, hip_ctx):
    """two quantisers stand in for two ranks: each splits half of a round's batch, packs its half, the staging buffers are summed (what all_reduce_u64 does) and
    unpacked into both; both must then hold what a third one holds that split the whole batch"""
    v, w = narrow_input("sel", 700, "w4096")
    S = TsvqNodes(v, w)
    L, h = hip_ctx.lib, hip_ctx.h
    A, B, Cq = (make("packed", v, w, tsvq_wide_min=0) for _ in range(3))
    for q in (A, B, Cq):
        _, batches, _ = check_rounds(q, S, 16, rounds=2)
    batch = [c for nd in batches[1] for c in (nd.left, nd.right)]
    assert len(batch) == 4 and all(nd.count >= 2 for nd in batch)
    for nd in batch:
        nd.host_split(S)
    nodes = records(batch)
    full = Cq.split(nodes); full["pad"] = 0
    staged, mines = [], []
    for q, share in ((A, [0, 2]), (B, [1, 3])):
        mine = np.zeros(4, np.uint8); mine[share] = 1
        recs = np.zeros(4, TSVQ_SPLIT)
        recs[share] = q.split(nodes[share]); recs["pad"] = 0
        d_staging, n_u64 = VP(), C.c_uint64()
        assert L.tsvq_exchange_pack(h, q.q, vp(nodes), vp(mine), vp(recs), 4, C.byref(d_staging), C.byref(n_u64)) == 1, L.last_error(h)
        staged.append((d_staging.value, n_u64.value, hip_ctx.download(d_staging.value, n_u64.value, np.uint64)))
        mines.append(mine)
    (pa, na, sa), (pb, nb, sb) = staged
    total = sum(nd.count for nd in batch)
    rec_at = (total * 4 + 7) // 8   # in u64 words: the child lists end to end, padded to a u64 boundary, then the records
    assert na == nb == rec_at + 4 * TSVQ_SPLIT.itemsize // 8
    # each is zero where the other's nodes lie
    lists_a, lists_b = sa[:rec_at].view(np.uint32), sb[:rec_at].view(np.uint32)
    recs_a, recs_b = sa[rec_at:].view(TSVQ_SPLIT), sb[rec_at:].view(TSVQ_SPLIT)
    at = 0
    for i, nd in enumerate(batch):
        kids = np.concatenate([nd.left.members, nd.right.members])
        mine_l, other_l, mine_r, other_r = (lists_a, lists_b, recs_a, recs_b) if i in (0, 2) else (lists_b, lists_a, recs_b, recs_a)
        assert (mine_l[at:at + nd.count] == kids).all() and not other_l[at:at + nd.count].any(), f"node {i}"
        assert mine_r[i].tobytes() == full[i].tobytes() and not np.frombuffer(other_r[i].tobytes(), np.uint8).any(), f"node {i}"
        at += nd.count
    both = sa + sb
    for q, p, mine in ((A, pa, mines[0]), (B, pb, mines[1])):
        hip_ctx.check(L.memcpy_h2d(h, p, vp(both), both.nbytes), "memcpy_h2d")
        recs = np.zeros(4, TSVQ_SPLIT)
        assert L.tsvq_exchange_unpack(h, q.q, vp(nodes), vp(mine), vp(recs), 4) == 1, L.last_error(h)
        assert recs.tobytes() == full.tobytes()
        for i, nd in enumerate(batch):
            assert_split(recs[i], nd, 16, f"unpacked node {i}")
            assert_lists(q, nd, f"unpacked node {i}")
