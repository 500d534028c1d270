"""The tensor-list edge lists and their reference, checked on the host (no
kernel launches): the net itself, before it judges a kernel.

* every list of tests/list_edges.py puts its edges where it claims to, under
  the substream geometry mirrored from csrc/mt_plan.hpp — the counts
  below are conditions of the GPU suite's coverage and are asserted;
* the Python-integer reference reproduces the reference implementation's own
  fixtures (tests/golden/f1_t3n5.npz, f2_t5n9.npz), cut into tensors;
* the lists go through csrc/seg_plan.hpp as the generation kernels drive it —
  per substream, seg_find on the first group emitted, seg_step up or down —
  in a stand-alone program (tests/host/list_edges_check.cpp) built with
  AddressSanitizer and UndefinedBehaviorSanitizer.
"""
import os
import random
import shutil
import subprocess

import pytest

import list_edges as le
from delta_node.crypto.shamir import field
from golden.fixtures import load_npz, manifest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS = list(le.THRESHOLDS)


def plan(sizes, t):
    n_total = sum(sizes)
    draws, S, backward = le.substream_plan(n_total, t)
    return n_total, le.elems_per_substream(t, draws), S, backward, le.seg_begins(sizes)


# ------------------------------------------------------------ 1. the geometry mirror
def test_substream_plan_regimes():
    # (the bounds of mt_sub_len; E in the 2^10 regime)
    assert [le.elems_per_substream(t) for t in TS] == [1024, 512, 256]
    assert le.substream_plan(16640, 2) == (256, 65, set())  # 65 * 2^8: the last forward-only size
    assert le.substream_plan(16641, 2) == (1024, 17, {2, 4, 6, 8, 10, 12, 14})
    assert le.substream_plan(8861, 3) == (1024, 18, set(range(2, 17, 2)))  # LIST_A at t = 3 (tests/test_gpu_many.py)
    assert le.substream_plan(8861, 2)[0] == 256 and le.substream_plan(1704, 5)[0] == 256  # ... t = 2 and LIST_A59
    assert le.substream_plan((1 << 21) - 1, 2)[0] == 1024 and le.substream_plan(1 << 21, 2)[0] == 4096
    assert le.substream_plan((1 << 24) - 1, 2)[0] == 4096 and le.substream_plan(1 << 24, 2)[0] == 1 << 14
    draws, S, backward = le.substream_plan(1 << 23, 3)  # 2^24 coefficients
    assert (draws, S) == (1 << 14, 1024) and backward == set(range(2, 1023, 2))
    assert le.substream_plan(2048, 2) == (256, 8, set())
    assert le.substream_plan(17 * 1024, 2)[2] == set(range(2, 16, 2))  # the last substream (16) runs forward


@pytest.mark.parametrize("t", TS)
@pytest.mark.parametrize("name", list(le.BUILDERS))
def test_every_list_is_in_the_2e10_regime(name, t):
    sizes = le.build(name, t)
    n_total, E, S, backward, begins = plan(sizes, t)
    assert 16640 < n_total * (t - 1) < 1 << 21
    assert le.substream_plan(n_total, t)[0] == 1024 and S >= 8
    assert E == 1024 // (t - 1)
    assert {2, 4} <= backward and not {0, 1, 3, 5, S - 1} & backward
    assert begins[0] == 0 and begins[-1] == n_total and len(begins) == sum(1 for n in sizes if n) + 1


# ------------------------------------------------------------ 2. each list's claim
@pytest.mark.parametrize("t", TS)
def test_ones(t):
    sizes = le.build("ONES", t)
    n_total, E, S, backward, begins = plan(sizes, t)
    assert sizes[0] == 2 * E - 70 and sizes.count(1) >= E + 140
    assert not any(a == b == c == 0 for a, b, c in zip(sizes, sizes[1:], sizes[2:]))  # a pair, not a triple
    assert sum(a == b == 0 for a, b in zip(sizes, sizes[1:])) == 1
    assert sizes[-5:] == [1, 0, 1, 2, 1] and 5 <= n_total % 64 <= 63
    full, steps = 0, []
    for s in sorted(backward):
        groups = le.substream_groups(n_total, t, s)
        assert len(groups) == E // 64 and groups[-1] + 64 == (s + 1) * E  # wholly inside the substream
        for eb in groups:
            full += len(le.group_segments(begins, eb)) == 64
        # the downward cursor: from the group one higher (emitted just before) to this one
        steps += [le.seg_of(begins, eb + 64) - le.seg_of(begins, eb) for eb in groups[:-1]]
    assert full >= E // 64 - 1, full  # DESIGN 4.3's worst case: 64 iterations of emit_pieces per share
    assert max(steps) >= 64, max(steps)  # seg_step's downward loop over 64 entries
    assert sum(d >= 64 for d in steps) >= E // 64 - 1
    # emptied table entries inside the backward substream: the empties fall in [2E, 3E)
    e, inside = 0, 0
    for n in sizes:
        inside += n == 0 and 2 * E < e < 3 * E
        e += n
    assert inside >= E // 7 - 1
    last = le.group_segments(begins, n_total - n_total % 64)
    assert len(last) >= 4, last  # the last, partial group: several pieces with lanes masked off past n_total
    assert S - 1 not in backward


@pytest.mark.parametrize("t", TS)
def test_bounds(t):
    sizes = le.build("BOUNDS", t)
    n_total, E, S, backward, begins = plan(sizes, t)
    cuts = set(begins)
    for k in (2, 3, 4, 5):
        assert {k * E - 1, k * E, k * E + 1} <= cuts, k
    assert {2, 4} <= backward and not {3, 5} & backward  # a backward k and a forward k, twice each
    # so: a backward substream whose top group ends on a one-element segment and whose bottom group starts
    # with one, and the same for a forward substream
    for s in (2, 3, 4):
        groups = le.substream_groups(n_total, t, s)
        assert len(le.group_segments(begins, groups[0])) >= 2 and len(le.group_segments(begins, groups[-1])) >= 2
        assert le.seg_of(begins, groups[0]) == le.seg_of(begins, s * E - 1) + 1  # the substream starts a segment
    assert n_total % 64 and len(le.group_segments(begins, n_total - n_total % 64)) >= 2  # the ragged end


@pytest.mark.parametrize("t", TS)
def test_sixtyfours(t):
    sizes = le.build("SIXTYFOURS", t)
    n_total, E, S, backward, begins = plan(sizes, t)
    assert n_total % 64 == 0 and sizes[0] == 2 * E and sizes.count(64) >= 3 * E // 64 and 192 in sizes
    seen = []
    for s in (2, 3, 4):
        for eb in le.substream_groups(n_total, t, s):
            segs = le.group_segments(begins, eb)
            assert len(segs) == 1 and begins[segs[0]] == eb and begins[segs[0] + 1] == eb + 64
            assert le.single_tile(begins, segs[0], eb)  # seg_single_tile: its own segment's tile 0
            seen.append(segs[0])
    assert seen == list(range(seen[0], seen[0] + 3 * E // 64))  # the cursor moves one entry per group
    k192 = le.seg_of(begins, 5 * E)
    assert begins[k192] == 5 * E and begins[k192 + 1] == 5 * E + 192
    assert all(le.single_tile(begins, k192, 5 * E + 64 * i) for i in range(3))  # three groups, one tile


@pytest.mark.parametrize("t", TS)
def test_straddle(t):
    sizes = le.build("STRADDLE", t)
    n_total, E, S, backward, begins = plan(sizes, t)
    assert sizes[0] == 3 and sizes[1:6] == [256, 257, 511, 513, 1000]
    in_2_to_5 = [b for b in begins[:-1] if 2 * E <= b < 6 * E]
    assert in_2_to_5 and all(b % 64 for b in in_2_to_5)  # no segment there starts on a group boundary
    crossing = {}
    for s in (2, 3, 4, 5):
        crossing[s] = sum(le.piece_spans_two_tiles(begins, k, eb) for eb in le.substream_groups(n_total, t, s)
                          for k in le.group_segments(begins, eb))
        for eb in le.substream_groups(n_total, t, s):
            assert not le.single_tile(begins, le.seg_of(begins, eb), eb)  # every group goes through emit_pieces
    assert crossing[2] + crossing[4] >= 1, crossing  # w0 + lane - lane_lo > 255 in a backward substream
    assert crossing[3] + crossing[5] >= 1, crossing  # ... and in a forward one


@pytest.mark.parametrize("t", TS)
def test_empty_ends_and_single(t):
    sizes = le.build("EMPTY_ENDS", t)
    assert [n == 0 for n in sizes] == [True, True, False, True, True, False, True]
    assert len(le.seg_begins(sizes)) == 3
    assert len(le.build("SINGLE", t)) == 1


def test_big_list_is_the_2e12_length():
    sizes = le.big_list()
    n_total = sum(sizes)
    assert n_total == (1 << 19) + 77 and n_total * 4 == (1 << 21) + 308
    draws, S, backward = le.substream_plan(n_total, 5)
    assert draws == 1 << 12 and le.elems_per_substream(5, draws) == 1024 and {2, 4} <= backward
    begins, E = le.seg_begins(sizes), 1024
    assert sum(len(le.group_segments(begins, eb)) == 64 for eb in le.substream_groups(n_total, 5, 2)) == 16
    for k in (4, 5):
        assert {k * E - 1, k * E, k * E + 1} <= set(begins)
    assert len(le.group_segments(begins, n_total - n_total % 64)) >= 4


# ------------------------------------------------------------ 3. the reference, pinned
@pytest.mark.parametrize("key,sizes", [("f1", [1, 200, 63, 0, 500, 260]), ("f2", [100, 1, 155])])
def test_reference_reproduces_the_fixtures(key, sizes):
    cfg = manifest()[key]
    z = load_npz(cfg["file"])
    N, t, n = cfg["N"], cfg["t"], cfg["n"]
    assert sum(sizes) == N
    r = le.replayed(cfg["mt_seed"])
    got = le.split_reference([int(s) for s in z["secrets"]], sizes, t, n, r)
    cuts = [sum(sizes[:k]) for k in range(len(sizes) + 1)]
    for x in range(1, n + 1):
        for k, (a, b) in enumerate(zip(cuts, cuts[1:])):
            assert got[x - 1][k] == field.limbs_to_ints(z["share_limbs"][a:b, x - 1, :]), (x, k)
    probe = random.Random(cfg["mt_seed"])
    for _ in range(N * (t - 1)):
        probe.randint(1, le.P - 1)
    assert r.getstate() == probe.getstate()
    want = [le.to_field(int(s)) for s in z["secrets"]]
    for sub, size in zip(z["recon_subsets"], z["recon_sizes"]):
        xs = [int(x) for x in sub[:size]]
        ys = [[v for part in got[x - 1] for v in part] for x in xs]
        assert le.lagrange_reference(ys, xs) == want, xs


def test_replayed_generator_mid_array():
    r = le.replayed(5, 333)
    assert r.getstate()[1][624] == 333  # 333 words of the first array drawn: the index is mid-array
    assert le.replayed(5).getstate()[1][624] == 624  # freshly seeded: the array is regenerated by the first draw


def test_lagrange_reference_is_linear_over_inconsistent_rows():
    rng = random.Random(3)
    xs = [2, 4, 5]
    ya = [[rng.randint(0, le.P - 1) for _ in range(4)] for _ in xs]
    yb = [[rng.randint(0, le.P - 1) for _ in range(4)] for _ in xs]
    both = [[(a + b) % le.P for a, b in zip(ra, rb)] for ra, rb in zip(ya, yb)]
    ra, rb = le.lagrange_reference(ya, xs), le.lagrange_reference(yb, xs)
    assert le.lagrange_reference(both, xs) == [(a + b) % le.P for a, b in zip(ra, rb)]
    # a constant polynomial's shares give the constant
    assert le.lagrange_reference([[7, le.P - 1]] * 3, xs) == [7, le.P - 1]


# ------------------------------------------------------------ 4. the kernels' walk over the store plan
def test_lists_through_the_store_plan_as_the_kernels_walk_it(tmp_path):
    """Every list at every threshold, and the 2^12-length list: per substream
    seg_find on the first emitted group, seg_step up (forward) or down
    (backward), seg_single_tile / seg_piece per group; each element stored
    once at its own place — a stand-alone program under ASan + UBSan (not
    loaded into this process)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    cases = [(name, t, le.build(name, t)) for name in le.BUILDERS for t in TS] + [("BIG", 5, le.big_list())]
    lines = []
    for name, t, sizes in cases:
        n_total, E, S, backward, _ = plan(sizes, t)
        lines.append(" ".join(map(str, [E, S, len(backward)] + sorted(backward) + [len(sizes)] + sizes)))
    lists = tmp_path / "lists.txt"
    lists.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "list_edges_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "delta-node_amd", "csrc"), "-I", os.path.join(ROOT, "tests", "host"),
           os.path.join(ROOT, "tests", "host", "list_edges_check.cpp"), "-o", exe]
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe, str(lists)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    out = run.stdout.split("\n")
    assert out[len(cases)] == "ok", run.stdout
    for i, (name, t, _) in enumerate(cases):
        tag, idx, _, down, _, up = out[i].split()
        assert (tag, int(idx)) == ("list", i)
        if name in ("ONES", "BIG"):
            assert int(down) >= 64 and int(up) >= 64, out[i]  # the cursor crosses a group of one-element tensors
        if name == "SIXTYFOURS":
            assert int(down) >= 1, out[i]
