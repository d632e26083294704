"""The strip table of bu_hip_k_uastc_rdo_slices as plain host code (basis_universal_amd/csrc/uastc_rdo_strips.h; no GPU, nothing loaded into Python).

rdo_slices_layout_build is compiled with AddressSanitizer and UndefinedBehaviorSanitizer into a stand-alone program that prints the table of every (slice list,
total_jobs) it is given; this file holds the table to the reference's cutting rule written out again here (uastc_rdo, uastc_enc.cpp:4103-4111)."""
import json
import os
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
SLICE_LISTS = ([600, 1, 40, 257, 9, 2, 36, 0, 64], [120, 120, 120], [4400, 300], [257, 40], [0], [0, 0, 5], [1], [1 << 20, 1 << 18, 1 << 16, 4096, 1024, 256, 64, 16, 4, 1, 1, 1, 1],
               [4096] * 64)
JOBS = (0, 1, 3, 4, 64)
ONE_SLICE = (1, 8, 35, 36, 37, 257, 1464, 4096)   # at four jobs 35: one strip (per_job 8), 36: four strips, 37: five, the last of one block
INFO_BYTES, HIST_ENTRY_BYTES, TABLE_BYTES = 32, 16, 2048

MAIN = r"""
#include "uastc_rdo_strips.h"
#include <cstdio>
#include <cstdlib>
#include <string>
// argv: total_jobs, then the slices' block counts. One JSON object on stdout.
int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const uint32_t jobs = (uint32_t)std::strtoul(argv[1], nullptr, 10);
    std::vector<uint32_t> slices;
    for (int k = 2; k < argc; k++) slices.push_back((uint32_t)std::strtoul(argv[k], nullptr, 10));
    bu::rdo_slices_layout L;
    if (!bu::rdo_slices_layout_build(slices.data(), (uint32_t)slices.size(), jobs, L)) { std::printf("{\"ok\": false}\n"); return 0; }
    std::printf("{\"ok\": true, \"total_blocks\": %u, \"longest\": %u, \"recs\": [", L.total_blocks, L.longest);
    for (size_t i = 0; i < L.recs.size(); i++) {
        const bu::rdo_strip_rec& r = L.recs[i];
        std::printf("%s[%u, %u, %u, %u, %llu, %u]", i ? ", " : "", r.first, r.last, r.hist_cap, r.mod_ofs, (unsigned long long)r.hist_ofs, r.slice);
    }
    std::printf("], \"order\": [");
    for (size_t i = 0; i < L.order.size(); i++) std::printf("%s%u", i ? ", " : "", L.order[i]);
    std::printf("], \"slice_strips\": [");
    for (size_t i = 0; i < L.slice_strips.size(); i++) std::printf("%s%u", i ? ", " : "", L.slice_strips[i]);
    std::printf("], \"at\": {\"counters\": %zu, \"strip_counts\": %zu, \"strip_flags\": %zu, \"hist\": %zu, \"state\": %zu, \"zero_bytes\": %zu, \"strips\": %zu, \"order\": %zu, "
                "\"info\": %zu, \"mod_list\": %zu, \"table\": %zu, \"total_bytes\": %zu}}\n",
                L.counters, L.strip_counts, L.strip_flags, L.hist, L.state, L.zero_bytes, L.strips, L.order_at, L.info, L.mod_list, L.table, L.total_bytes);
    return 0;
}
"""


def strip_layout(n, jobs):
    """uastc_rdo's rule for one slice: (per_job or 0, strips, history capacity) -- strip_layout of uastc_rdo_kernels.hip before it moved into the header"""
    per_job = n // jobs if jobs else 0
    if jobs <= 1 or per_job <= 8:
        per_job, strips = 0, 1
    else:
        strips = -(-n // per_job)
    longest, cap = (per_job or n), 64
    while cap < 4 * longest and cap < 1 << 30:
        cap <<= 1
    return per_job, strips, cap


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the strip table program"
    d = tmp_path_factory.mktemp("rdo_slices")
    (d / "main.cpp").write_text(MAIN)
    exe = d / "strip_table"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-Wall", "-Wextra", "-I", str(ROOT / "basis_universal_amd" / "csrc"), "-o", str(exe), str(d / "main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(slices, jobs):
        env = dict(os.environ)
        env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
        r = subprocess.run([str(exe), str(jobs)] + [str(n) for n in slices], capture_output=True, text=True, env=env)
        assert r.returncode == 0 and not r.stderr.strip(), (slices, jobs, r.returncode, r.stderr[-3000:])
        return json.loads(r.stdout)
    return run


@pytest.mark.parametrize("jobs", JOBS)
@pytest.mark.parametrize("slices", SLICE_LISTS, ids=[f"{len(s)}slices_{sum(s)}" for s in SLICE_LISTS])
def test_strip_table(program, slices, jobs):
    L = program(slices, jobs)
    assert L["ok"] and L["total_blocks"] == sum(slices)
    recs, at = L["recs"], L["at"]
    # every slice's strips are those of strip_layout for that slice alone, shifted to where the slice begins; an empty slice has no record
    want, begin = [], 0
    for s, n in enumerate(slices):
        per_job, strips, cap = strip_layout(n, jobs)
        assert L["slice_strips"][s] == strips
        for k in range(strips if n else 0):
            first = begin + k * per_job
            want.append((first, begin + (min(n, (k + 1) * per_job) if per_job else n), cap, first, s))
        begin += n
    assert [(r[0], r[1], r[2], r[3], r[5]) for r in recs] == want
    # the ranges tile [0, total) exactly, in order, and none is empty
    edge = 0
    for first, last, *_ in recs:
        assert first == edge and last > first
        edge = last
    assert edge == sum(slices)
    assert L["longest"] == max([r[1] - r[0] for r in recs], default=0)
    # histories: back to back, none overlapping, all inside their region; the mod_list of a strip is its own block range
    hist_at = 0
    for r in recs:
        assert r[4] == hist_at and r[2] >= 64 and r[2] & (r[2] - 1) == 0
        hist_at += r[2]
    S, n = len(recs), sum(slices)
    regions = [("counters", 16 * len(slices)), ("strip_counts", 4 * S), ("strip_flags", 4 * S), ("hist", hist_at * HIST_ENTRY_BYTES), ("state", n), ("strips", 32 * S), ("order", 4 * S),
               ("info", n * INFO_BYTES), ("mod_list", 4 * n), ("table", n * TABLE_BYTES)]
    end = 0
    for name, size in regions:
        assert at[name] >= end and at[name] % 256 == 0, name
        end = at[name] + size
        if name == "state":
            assert end <= at["zero_bytes"] <= at["strips"]   # what the call clears: counters, strip counts and flags, histories, state -- and not the table it has uploaded
    assert end <= at["total_bytes"]
    # launch order: a permutation of the strips, non-increasing in length, ties in block order
    order = L["order"]
    assert sorted(order) == list(range(S))
    lengths = [recs[i][1] - recs[i][0] for i in order]
    assert all(a >= b for a, b in zip(lengths, lengths[1:]))
    assert all(i < j for (i, a), (j, b) in zip(zip(order, lengths), zip(order[1:], lengths[1:])) if a == b)


def up256(v):
    return (v + 255) & ~255


@pytest.mark.parametrize("jobs", JOBS)
@pytest.mark.parametrize("n", ONE_SLICE)
def test_one_slice_is_the_arithmetic_form(program, n, jobs):
    """The layout of ONE slice is what the arithmetic builds of the kernels (strip k: per_job and one history capacity, no table on the device) work on, and up to
    zero_bytes what the single-slice entry carved before this layout became the only one; the regions of the table it does not upload are all it adds."""
    L = program([n], jobs)
    per_job, strips, cap = strip_layout(n, jobs)
    assert L["ok"] and L["total_blocks"] == n and L["slice_strips"] == [strips] and len(L["recs"]) == strips
    for k, (first, last, hist_cap, mod_ofs, hist_ofs, slice_) in enumerate(L["recs"]):
        assert (first, last) == ((k * per_job, min(n, k * per_job + per_job)) if per_job else (0, n))
        assert (hist_cap, mod_ofs, hist_ofs, slice_) == (cap, first, k * cap, 0)
    assert L["longest"] == (per_job or n)
    # the carve of the single-slice entry as it was: 256 bytes of counters, then strip counts, strip flags, histories and state, every region rounded up to 256
    at, o = L["at"], 0
    for name, size in (("counters", 256), ("strip_counts", 4 * strips), ("strip_flags", 4 * strips), ("hist", strips * cap * HIST_ENTRY_BYTES), ("state", n)):
        assert at[name] == o, name
        o += up256(size)
    assert at["zero_bytes"] == o
    was_total = o + up256(n * INFO_BYTES) + up256(4 * n) + up256(n * TABLE_BYTES)
    assert at["total_bytes"] == was_total + up256(32 * strips) + up256(4 * strips)
    if jobs == 4 and n in (35, 36, 37):
        assert (strips, per_job) == {35: (1, 0), 36: (4, 9), 37: (5, 9)}[n]
        assert L["recs"][-1][:2] == {35: [0, 35], 36: [27, 36], 37: [36, 37]}[n]


def test_a_mip_level_does_not_reserve_level_0s_history(program):
    """a strip's history follows its own slice: 64 entries for the 1-block levels beside level 0's 4 x its blocks"""
    L = program([1 << 20, 1, 1], 1)
    assert [r[2] for r in L["recs"]] == [1 << 22, 64, 64]


def test_block_total_must_fit(program):
    assert not program([0x7FFFFFFF, 1], 4)["ok"]
    assert not program([0xFFFFFFFF, 0xFFFFFFFF], 0)["ok"]
    assert program([0x7FFFFFFF], 4)["ok"]
