"""tests/mt_levels.py (the model of the MT19937 draw's jump-level builder)
pinned to the real builder, and the builder's own regime boundaries, scratch
bound and unread table rows.

The real builder is csrc/mt_plan.hpp, the draw's host-only planner, compiled
into tools/mt_levels_check.cpp by the host compiler (no GPU and no HIP
needed); its `dump` mode prints, per
substream count and length, what mt_levels built: back, rt, the part rows,
and per level the jumps n, parts P, waves W, workgroups, the largest
workgroup, the part rows written, the cut list and the table rows read.  The
tool is built with -DDN_TUNING here so that the DN_MT_BACK / DN_MT_RT knobs of
the tuning library can be pinned too (test_gpu_mt_levels.py draws with them),
and once more as the product library is built, which must give the same levels.
test_gpu_mt_levels.py takes its cases from the model; this file is what makes
the model's word the builder's."""
import os
import random
import shutil
import subprocess

import pytest

import mt_levels as ml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDARY_S = [2049, 2050, 4095, 4096, 4097, 4098, 8193, 16385, 65537]


@pytest.fixture(scope="module")
def builders(tmp_path_factory):
    """The tool built as the tuning library is (-DDN_TUNING: the DN_* knobs
    apply) and as the product library is (no knob is read), side by side."""
    cxx = "/opt/rocm/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    out = tmp_path_factory.mktemp("mt_levels")
    exes = {"tuning": str(out / "mt_levels_check_tuning"), "product": str(out / "mt_levels_check")}
    runs = [subprocess.Popen([cxx, "-O1", "-std=c++17", *(["-DDN_TUNING"] if name == "tuning" else []),
                              "-I" + os.path.join(ROOT, "include"),
                              "-I" + os.path.join(ROOT, "delta-node_amd", "csrc"),
                              os.path.join(ROOT, "tools", "mt_levels_check.cpp"), "-o", exe],
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for name, exe in exes.items()]
    for run in runs:
        text = run.communicate()[0]
        assert run.returncode == 0, text[-3000:]
    return exes


@pytest.fixture(scope="module")
def builder(builders):
    return builders["tuning"]


def fields(line):
    return dict(kv.split("=", 1) for kv in line.split()[1:])


def runs_to_set(text):
    out = set()
    for run in text.split(","):
        span, step = run.split("/")
        a, b = span.split("-")
        out.update(range(int(a), int(b) + 1, int(step)))
    return out


def dump(exe, queries, **knobs):
    """The builder's answers: {(ki, S): (S-line fields, [level fields])} for
    ("S", ki, S) queries and {ncoef: fields} for ("N", ncoef) ones."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("DN_")}
    env.update(knobs)
    text = "".join(" ".join(map(str, q)) + "\n" for q in queries)
    r = subprocess.run([exe, "dump"], input=text, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    subs, sizes, cur = {}, {}, None
    for line in r.stdout.splitlines():
        f = fields(line)
        if line.startswith("S "):
            cur = (int(f["ki"]), int(f["S"]))
            subs[cur] = (f, [])
        elif line.startswith("L "):
            subs[cur][1].append(f)
        elif line.startswith("N "):
            sizes[int(f["ncoef"])] = f
    assert len(subs) + len(sizes) == len(set(queries)), "the builder answered another number of queries"
    return subs, sizes


def level_facts(f):
    """What a level line says, in the model's terms."""
    return dict(k=int(f["k"]), n=int(f["n"]), P=int(f["P"]), W=int(f["W"]), wgs=int(f["wgs"]), grp=int(f["grp"]),
                prow=tuple(map(int, f["prow"].split(","))), cuts=tuple(map(int, f["cuts"].split(","))),
                polys=runs_to_set(f["polys"]))


def model_facts(k, l):
    return dict(k=k, n=l.n, P=l.P, W=l.W, wgs=l.wgs, grp=l.grp, prow=l.prow, cuts=l.cuts, polys=set(l.polys))


def assert_same(got, ki, S, back=None, rt_rows=True):
    f, lines = got[(ki, S)]
    mback, mrt, kind, lv, part_rows = ml.plan_for(S, ki, back, rt_rows)
    what = ml.describe(ki, S, kind, lv)
    assert (int(f["back"]), int(f["rt"]), int(f["part_rows"])) == (mback, int(mrt), part_rows), what
    want = [model_facts(k, l) for k, l in enumerate(lv) if l is not None]
    have = [level_facts(x) for x in lines]
    assert len(have) == len(want), what
    for h, w in zip(have, want):
        # wgs and grp pin `per` wherever it matters: the workgroups are each source's jumps in
        # groups of per, so a `per` above every source's count changes no job (mt_levels.shape_of)
        diff = {key: (h[key], w[key]) for key in w if h[key] != w[key] and key != "polys"}
        assert not diff and h["polys"] == w["polys"], (what, diff, sorted(h["polys"] ^ w["polys"])[:8])


def test_builder_constants_are_the_models(builder):
    f = dump(builder, [("S", 0, 2)])[0][(0, 2)][0]
    assert (int(f["direct_rows"]), int(f["jump_rows"]), int(f["rt_rows"]), int(f["max_parts"])) == \
        (ml.DIRECT_ROWS, ml.JUMP_ROWS, ml.RT_ROWS, ml.MAX_PARTS)


def test_model_equals_builder(builder):
    """Every S from 1 to 2200 and the boundary counts, at each substream
    length (the 2^8 length has direct rows only: up to 65 substreams): back,
    rt, part rows, and per level n, P, W, the workgroups, the largest
    workgroup, the part rows, the cut list and the rows read are equal."""
    qs = [("S", ki, S) for ki in range(4) for S in list(range(1, 2201)) + BOUNDARY_S if ml.supported(S, ki)]
    got = dump(builder, qs)[0]
    for _, ki, S in qs:
        assert_same(got, ki, S)


def test_model_equals_the_product_build_of_the_builder(builders):
    """The builder compiled as the product library compiles it, which reads
    no knob: equal to the model at the boundary counts, around every regime
    boundary and at every 7th S to 2200, and deaf to DN_MT_BACK / DN_MT_RT."""
    counts = sorted(set(BOUNDARY_S) | set(range(1, 2201, 7)) | {2, 3, 64, 65, 66, 67, 1024, 1025, 2048, 2051, 2200})
    qs = [("S", ki, S) for ki in range(4) for S in counts if ml.supported(S, ki)]
    got = dump(builders["product"], qs)[0]
    for _, ki, S in qs:
        assert_same(got, ki, S)
    got = dump(builders["product"], qs, DN_MT_BACK="0", DN_MT_RT="0")[0]
    for _, ki, S in qs:
        assert_same(got, ki, S)


def test_model_equals_builder_under_the_tuning_knobs(builder):
    """DN_MT_BACK=0 (every window jumped to) at the three table lengths up to
    their largest draws' counts, and DN_MT_RT=0 (the runtime rows unavailable:
    levels A and B of the 2^14 table) over the runtime level's whole range."""
    qs = [("S", ki, S) for ki, top in ((0, 2048), (1, 4096), (2, 2200)) for S in list(range(2, 300)) + [top - 1, top]]
    got = dump(builder, qs, DN_MT_BACK="0")[0]
    for _, ki, S in qs:
        assert_same(got, ki, S, back=0)
    qs = [("S", 2, S) for S in range(60, 2060)]
    got = dump(builder, qs, DN_MT_RT="0")[0]
    for _, ki, S in qs:
        assert_same(got, ki, S, rt_rows=False)
        assert int(got[(ki, S)][0]["rt"]) == 0


def kind_of(entry):
    """The level kind as the builder's own output shows it."""
    f, lines = entry
    if not lines:
        return "none"
    polys = set().union(*(runs_to_set(x["polys"]) for x in lines))
    if int(f["rt"]):
        assert len(lines) == 1 and min(polys) >= ml.RT_BASE
        return "rt"
    if min(polys) >= ml.DIRECT_BASE:
        assert len(lines) == 1 and max(polys) < ml.RT_BASE
        return "direct"
    assert max(polys) < ml.DIRECT_BASE and int(lines[0]["k"]) == 0 and int(lines[-1]["k"]) == 2
    return "radix"


def test_regime_boundaries_of_the_builder(builder):
    """From the builder's output alone: 2^8-draw substreams up to 65 * 2^8
    coefficients, 2^10 up to 2^21 - 1, 2^12 up to 2^24 - 1, 2^14 from there;
    one tabulated direct level while S - 1 <= 64; at the 2^14 length the
    runtime direct level while S - 1 <= 2048, radix levels after it; a C level
    from S - 1 > 4096."""
    n8 = 65 << 8
    want = {1: (3, 1), n8: (3, 65), n8 + 1: (0, 17), (1 << 21) - 1: (0, 2048), 1 << 21: (1, 512),
            (1 << 24) - 1: (1, 4096), 1 << 24: (2, 1024), (1 << 24) + 1: (2, 1025), ml.MAX_COEFFS: (2, ml.MAX_SUBS)}
    subs, sizes = dump(builder, [("N", n) for n in want] +
                       [("S", ki, S) for ki in range(3) for S in (1, 2, 65, 66, 2049, 2050, 4097, 4098)] +
                       [("S", 3, 1), ("S", 3, 2), ("S", 3, 65)])
    for n, (ki, S) in want.items():
        assert (int(sizes[n]["ki"]), int(sizes[n]["S"])) == (ki, S), n
    for ki in range(4):
        assert kind_of(subs[(ki, 1)]) == "none" and kind_of(subs[(ki, 2)]) == "direct" and kind_of(subs[(ki, 65)]) == "direct"
        assert int(subs[(ki, 2)][0]["back"]) == (0 if ki == 3 else 1)
    for ki in (0, 1):
        for S in (66, 2049, 2050, 4097, 4098):
            assert kind_of(subs[(ki, S)]) == "radix", (ki, S)
    assert kind_of(subs[(2, 66)]) == "rt" and kind_of(subs[(2, 2049)]) == "rt"
    assert kind_of(subs[(2, 2050)]) == "radix" and kind_of(subs[(2, 4098)]) == "radix"
    for ki in range(3):
        assert [int(x["k"]) for x in subs[(ki, 4097)][1]] == [0, 2] and [int(x["k"]) for x in subs[(ki, 4098)][1]] == [0, 1, 2]


def test_part_rows_lie_inside_the_reserved_scratch(builder):
    """For every shape's smallest size, the largest size of each length and
    the sizes around each regime boundary: dn_mt19937_device_scratch_bytes is
    the head, the rows -1 .. S and the part rows mt_levels counted, and every
    level's part rows lie in [S + 1, S + 1 + part rows)."""
    ns = {ml.coeffs_for(S, ki, full) for ki, S in ml.shapes(1, 8200 << 14).values() for full in (False, True)}
    ns |= {65 << 8, (65 << 8) + 1, (1 << 21) - 1, 1 << 21, (1 << 24) - 1, 1 << 24, (2048 << 14) + 1, (2049 << 14) + 1,
           ml.MAX_COEFFS}
    ns = sorted(n for n in ns if n <= ml.MAX_COEFFS)
    subs, sizes = dump(builder, [("N", n) for n in ns] + sorted({("S", ml.sub_len(n), ml.subs(n)) for n in ns}))
    split_levels = 0
    for n in ns:
        f = sizes[n]
        ki, S = int(f["ki"]), int(f["S"])
        head, lines = subs[(ki, S)]
        rows = int(head["part_rows"])
        assert int(f["scratch"]) == int(f["head"]) + (1 + S + 1 + rows) * ml.MT_N * 4 == ml.scratch_bytes(n), n
        for x in lines:
            lo, hi = map(int, x["prow"].split(","))
            if int(x["P"]) > 1:
                split_levels += 1
                assert S + 1 == lo and hi == lo + int(x["n"]) * int(x["P"]) <= S + 1 + rows, (n, x)
                assert hi - lo <= ml.PART_ROWS
            else:
                assert (lo, hi) == (0, 0)
    assert split_levels > 100


def test_rows_no_supported_size_reads(builder):
    """The union of the rows the builder's jobs read over a set of substream
    counts that covers every supported size (mt_levels.covering_subs), against
    the tables: 804 of the 2874 rows are never read by the device draw —

      * the C rows of the 2^10 and 2^12 tables (draws of those lengths have at
        most 2048 / 4096 substreams: no third digit) and A_32 .. A_63 of the
        2^10 table;
      * the direct rows of the 2^12 and 2^14 lengths (draws of those lengths
        have at least 512 / 1024 substreams) and, of the 2^10 length, the even
        D_2 .. D_14 (at least 17 substreams, and an even window is jumped to
        only as the last one);
      * the runtime rows D_s of even s < 1024 (the same, from 1025 substreams).

    (The host reads some of them: host_gf2poly.cpp checks the embedded runtime
    rows against the 2^14 direct rows.)"""
    cover = ml.covering_subs(1, ml.MAX_COEFFS)
    subs = dump(builder, [("S", ki, S) for ki, S in cover])[0]
    used = set()
    for _, lines in subs.values():
        for x in lines:
            used |= runs_to_set(x["polys"])
    total = ml.RT_BASE + ml.RT_ROWS
    assert max(used) < total
    unused = set(range(total)) - used
    t10, t12 = 0, ml.JUMP_ROWS
    want = set(range(t10 + 32, t10 + ml.ROW_B + 1)) | set(range(t12 + ml.ROW_C + 1, t12 + ml.ROW_B + 1))
    want |= {ml.DIRECT_BASE + s - 1 for s in range(2, 16, 2)}
    want |= set(range(ml.DIRECT_BASE + ml.DIRECT_ROWS, ml.DIRECT_BASE + 3 * ml.DIRECT_ROWS))
    want |= {ml.RT_BASE + s - 1 for s in range(2, 1024, 2)}
    assert unused == want, sorted(map(ml.row_name, unused ^ want))[:20]
    assert len(unused) == 804
    assert ml.rows_used(1, ml.MAX_COEFFS) == (used, unused)


def test_shape_census():
    """60 distinct (length, kind, per level (P, W, group)) shapes below 2^21
    coefficients; part counts are what part_cuts returns, at most 29: a
    request for 32 parts gives 23."""
    small = ml.shapes(1, (1 << 21) - 1)
    assert len(small) == 60
    assert {lv[-1][1] for _, _, lv in small if lv} >= set(range(4, 17)) | {19, 22, 23, 25, 28, 29}
    assert len(ml.part_cuts(32, 8)) - 1 == 23 and ml.j0_parts() == 23


@pytest.mark.slow
def test_shape_census_over_every_supported_size():
    """190 shapes up to the largest supported draw (262144 substreams of 2^14
    draws), none with more than 29 parts: the figures DESIGN.md states."""
    every = ml.shapes(1, ml.MAX_COEFFS)
    assert len(every) == 190
    assert max(level[1] for _, _, lv in every for level in lv) == 29


def final_plans(exe, pairs):
    """mt_final_plan's fields, as the builder's `F <idx> <ncoef>` query prints
    them: {(idx, ncoef): {field: int}}."""
    text = "".join(f"F {idx} {n}\n" for idx, n in pairs)
    env = {k: v for k, v in os.environ.items() if not k.startswith("DN_")}
    r = subprocess.run([exe, "dump"], input=text, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {}
    for line in r.stdout.splitlines():
        assert line.startswith("F "), line
        f = {k: int(v) for k, v in fields(line).items()}
        out[(f["idx"], f["ncoef"])] = f
    assert len(out) == len(set(pairs)), "the builder answered another number of queries"
    return out


def test_final_plan_of_the_builder(builders):
    """mt_final_plan (csrc/mt_plan.hpp), which mt_device_run takes CPython's
    state after the draw from.

    The final index against CPython's rule for w = 17 ncoef words drawn at
    index idx, h = 624 - idx of them left in the caller's array:
    idx + w if w <= h else (w - h - 1) % 624 + 1 — at idx 0, 1, 333, 623, 624
    and, for each, the word counts 17, the last w <= h (where one exists), the
    first w > h, and the w with w - h = 624 m - 1, 624 m, 624 m + 1 (17 is a
    unit mod 624, so each residue has word counts) for the first such w, the
    one 624 * 17 words later and one of 2^24-draw size, with the coefficient
    counts next to each.  sig is -1 exactly while w <= h.

    The window the final array is stepped from, for every substream length
    and every S of 1, 2, 3, 65, 66, 1025, 2049 a draw of that length can have
    (2^8 draws: up to 65; 2^10: 17 to 2048; 2^12: 512 to 4096; 2^14: from
    1024), the last substream holding one draw or full: 0 <= sig <= S - 1, the
    window is where the model has it, and its position (0: the caller's
    array, else idx + sig L - 624) lies below the final array's, a multiple of
    624 at or past the draw's last word."""
    inv17 = pow(17, -1, ml.MT_N)
    pairs = set()
    for idx in (0, 1, 333, 623, 624):
        h = ml.MT_N - idx
        ns = {1, h // 17, h // 17 + 1}
        for r in (-1, 0, 1):
            n0 = (h + r) * inv17 % ml.MT_N  # 17 n0 - h = r (mod 624)
            while 17 * n0 <= h:
                n0 += ml.MT_N
            big = n0 + ml.MT_N * ((1 << 24) // ml.MT_N)
            ns |= {n0 - 1, n0, n0 + 1, n0 + ml.MT_N, big - 1, big, big + 1}
            assert (17 * n0 - h) % ml.MT_N == r % ml.MT_N and (17 * big - h) % ml.MT_N == r % ml.MT_N
        pairs |= {(idx, n) for n in ns if n >= 1}
    got = final_plans(builders["product"], sorted(pairs))
    below = past = 0
    for (idx, n), f in got.items():
        w, h = 17 * n, ml.MT_N - idx
        assert f["fidx"] == (idx + w if w <= h else (w - h - 1) % ml.MT_N + 1), (idx, n, f)
        assert (f["sig"] == -1) == (w <= h), (idx, n, f)
        below += w <= h
        past += w > h and (w - h) % ml.MT_N == 0
    assert below >= 6 and past >= 15  # (idx 0, 1, 333 have two w <= h each; every idx three w - h = 624 m)

    shapes = [(ki, S) for ki in range(4) for S in (1, 2, 3, 65, 66, 1025, 2049)
              if ml.supported(S, ki) and (ml.sub_len(ml.coeffs_for(S, ki, True)), ml.subs(ml.coeffs_for(S, ki, True))) == (ki, S)]
    assert shapes == [(0, 65), (0, 66), (0, 1025), (1, 1025), (1, 2049), (2, 1025), (2, 2049), (3, 1), (3, 2), (3, 3), (3, 65)]
    pairs = {(idx, ml.coeffs_for(S, ki, full)) for ki, S in shapes for full in (False, True) for idx in (0, 1, 333, 623, 624)}
    for ki, S in shapes:
        assert (ml.sub_len(ml.coeffs_for(S, ki, False)), ml.subs(ml.coeffs_for(S, ki, False))) == (ki, S)
    got = final_plans(builders["product"], sorted(pairs))
    assert got == final_plans(builders["tuning"], sorted(pairs))
    for (idx, n), f in got.items():
        ki, S, L = f["ki"], f["S"], 17 * ml.sub_draws(f["ki"])
        assert (ki, S) == (ml.sub_len(n), ml.subs(n)) and (ki, S) in shapes
        w, h = 17 * n, ml.MT_N - idx
        if w <= h:
            assert f["sig"] == -1, (idx, n, f)
            continue
        assert 0 <= f["sig"] <= S - 1 and f["sig"] == ml.final_sig(n, idx, ki, S), (idx, n, f)
        assert f["pos"] == (idx + f["sig"] * L - ml.MT_N if f["sig"] else 0), (idx, n, f)
        assert f["tf"] % ml.MT_N == 0 and f["tf"] - ml.MT_N < w - h <= f["tf"], (idx, n, f)
        assert f["pos"] < f["tf"], (idx, n, f)
        # the last substream's frame starts at stream position idx + (S - 1) L
        assert f["fin_lo"] == f["tf"] - (idx + (S - 1) * L) and f["next_lo"] == idx + w - (idx + (S - 1) * L), (idx, n, f)


def test_final_state_window_is_the_last_one():
    """mt_final_plan's `sig`, restated in the model as a closed form, against
    a scan over the windows: the largest s <= S - 1 whose window (position
    idx + s L - 624; window 0 the caller's array) starts before CPython's final
    array, the first 624-word array boundary at or past the draw's last word.
    It is -1 when the draw ends inside the caller's array and S - 1 otherwise,
    a window every draw jumps to, whatever the MT index."""
    rnd = random.Random(5)
    sizes = list(range(1, 700)) + [n + d for n in (65 << 8, 1 << 21, 1 << 24, 2049 << 14) for d in (-1, 0, 1, 2)]
    sizes += [rnd.randrange(1, 1 << 26) for _ in range(300)]
    for n in sizes:
        for idx in (0, 1, 333, 606, 607, 608, 623, 624):
            p = ml.plan(n, idx)
            words, left = 17 * n, ml.MT_N - idx
            if words <= left:
                assert p.sig == -1, (n, idx)
                continue
            final = -(-(words - left) // ml.MT_N) * ml.MT_N  # stream position of the final array
            L = 17 * p.draws
            scan = max(s for s in range(max(0, p.S - 3), p.S) if s == 0 or idx + s * L - ml.MT_N < final)
            assert p.sig == scan == p.S - 1, (n, idx, p.sig, scan)
            assert p.S == 1 or ml.window_needed(p.S - 1, p.S, p.back), (n, idx)
