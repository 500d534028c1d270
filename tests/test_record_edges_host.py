"""tests/record_edges.py against what it claims (no kernel launches).

* the parse model against the reference's record parser as oracle/py_shamir
  restates it (pinned by tests/golden) on the reference's own share bytes, and
  against shamir._share_to_bytes / _bytes_to_share on the codec suite's
  special records;
* want_resolve and want_sum against the golden secrets (f1, f2) and Python's
  Lagrange form;
* every builder's claims: window sizes, staging rows, tail lanes, LDS or
  byte-serial per (wave, wire), the bad counts;
* assert_in_bounds for every wire test_gpu_record_edges.py uploads, the
  hostile tables and the opened corrupt frames included (the GPU module asks
  again before each upload);
* the geometry constants against tests/host/wire_geom_check.cpp.
"""
import numpy as np
import pytest

import record_edges as re
from delta_node.crypto.shamir import shamir as shamir_mod
from golden.fixtures import load_npz, manifest, unpack_share_bytes
from oracle.py_shamir import parse_share
from test_gpu_codec_edges import special_records
from test_wire_geom_host import geom  # noqa: F401  (the fixture that builds and runs wire_geom_check.cpp)

P = re.P


# ---------------------------------------------------------------- geometry
def test_geometry_constants_are_the_headers(geom):  # noqa: F811
    assert geom["kWinLimit"] == re.LIMIT and geom["kMaxRecord"] == re.MAX_RECORD
    assert geom["kWinPad"] == re.WIN_PAD and geom["kDecWindow"] == re.DEC_WINDOW
    assert geom["kDecRowWords"] == re.ROW_WORDS
    assert (geom["kStageQ"], geom["kStageW"]) == (re.STAGE_Q, re.STAGE_W) == (5, 19)
    assert geom["kStageRegs"] == max(4 * re.STAGE_Q, re.STAGE_W)
    # the largest LDS window, its reads one dword below and two above, inside the padded slice
    assert re.LIMIT + 8 <= 4 * re.ROW_WORDS - re.WIN_PAD and re.WIN_PAD >= 4


# ---------------------------------------------------------------- the parse model
@pytest.fixture(scope="module")
def golden():
    out = {}
    for key in ("f1", "f2"):
        cfg = manifest()[key]
        z = load_npz(cfg["file"])
        flat, offs = z["share_bytes"], z["share_offsets"]
        recs = {x: [unpack_share_bytes(flat, offs, e * cfg["n"] + x - 1) for e in range(cfg["N"])]
                for x in range(1, cfg["n"] + 1)}
        out[key] = (cfg, [int(v) for v in z["secrets"][:cfg["N"]]], recs)
    return out


@pytest.mark.parametrize("key", ["f1", "f2"])
def test_parse_wire_equals_the_reference_parser_on_its_own_records(golden, key):
    cfg, _, recs = golden[key]
    for x, rs in recs.items():
        for shift in (0, 4):
            w = re.from_records(rs, x, shift)
            assert w.parsed() == [(True,) + parse_share(r) for r in rs], (key, x)
            assert all(px == x for _, px, _ in w.parsed()) and re.counts(w.parsed(), x) == (0, 0)
            w.checked()


def test_parse_wire_on_the_special_records():
    specials = special_records()
    recs = [r for r, _ in specials]
    for align in (16, 4):
        w = re.from_records(recs, 0, 0 if align == 16 else 4)
        got = w.parsed()
        for (r, exp), (ok, x, y) in zip(specials, got):
            if exp is None:
                assert (ok, x, y) == re.BAD, r
            else:
                assert ok and (x, y) == exp, r
                assert shamir_mod._share_to_bytes(exp) == r and shamir_mod._bytes_to_share(r) == exp
        # and on the byte-serial path: a padded record pushes the window over the limit
        far = re.from_records(recs + [re.rec(1, 5, re.LIMIT)], 0, w.shift)
        assert not far.windows()[0].lds and far.parsed()[:len(recs)] == got


def test_leading_zero_bytes_and_the_68_byte_bound():
    y68 = (1 << 544) - 1
    recs = [re.rec(3, y68), re.rec(3, y68, 40), bytes([1, 3, 1]) + bytes(68), bytes([1, 3]) + bytes(200),
            bytes([8]) + bytes(7), bytes([8]) + bytes(8)]
    want = [(True, 3, y68), (True, 3, y68), re.BAD, (True, 3, 0), re.BAD, (True, 0, 0)]
    assert re.from_records(recs, 3).parsed() == want
    assert re.from_records(recs + [re.rec(3, 1, re.LIMIT)], 3).parsed()[:len(recs)] == want  # byte-serial


# ---------------------------------------------------------------- the expectations
@pytest.mark.parametrize("key,xs", [("f1", [1, 3, 5]), ("f1", [2, 4, 5]), ("f2", [1, 2, 4, 6, 9])])
def test_want_resolve_gives_the_golden_secrets(golden, key, xs):
    cfg, secrets, recs = golden[key]
    N = cfg["N"]
    want = re.want_resolve([re.from_records(recs[x], x) for x in xs], xs, N)
    assert want["i64"] == secrets and want["field"] == [s & re.U64 for s in secrets]
    assert (want["overflow"], want["bad"], want["mis"]) == (0, 0, 0)
    assert re.lagrange_at_zero(xs) == [l % P for l in shamir_mod._lagrange_generic(xs, P)]


def test_want_resolve_counts_overflow_and_wrong_x():
    xs = [1, 3, 5]
    ys = [[5, P - 1, 1 << 64], [5, P - 1, 1 << 64], [5, P - 1, 1 << 64]]   # the constant polynomial
    wires = [re.from_records([re.rec(x if e else x + 1, y) for e, y in enumerate(v)], x) for x, v in zip(xs, ys)]
    want = re.want_resolve(wires, xs, 3)
    assert want["field"] == [5, P - 1, 1 << 64] and want["i64"] == [5, -2, 0]  # p - 1 ends in ...FFFE
    assert (want["overflow"], want["bad"], want["mis"]) == (2, 0, 3)


def test_want_sum_of_the_members_shares_reconstructs_the_sum(golden):
    cfg, secrets, recs = golden["f1"]
    n, members = 256, 4
    signs = [1, 1, 1, -1]
    sums = {}
    for x in (1, 3, 5):
        wires = [re.from_records(recs[x][n * j:n * j + n], x) for j in range(members)]
        got = re.want_sum(wires, x, n, signs)
        assert (got["bad"], got["mis"]) == (0, 0) and all(0 <= v < P for v in got["field"])
        sums[x] = got["field"]
    lam = re.lagrange_at_zero([1, 3, 5])
    u = [s & re.U64 for s in secrets]
    for e in range(n):
        total = sum(s * u[n * j + e] for j, s in enumerate(signs))
        assert sum(l * sums[x][e] for l, x in zip(lam, (1, 3, 5))) % P == total % P
    acc = [P - 1] * n
    one = re.from_records([re.rec(1, 1)] * n, 1)
    assert re.want_sum([one], 1, n, acc=acc)["field"] == [0] * n       # canonical: 0, never p


# ---------------------------------------------------------------- the builders
def intended(w, align=None):
    """The model's parse equals what the builder meant, record by record."""
    for e, (got, want) in enumerate(zip(w.parsed(align), w.want)):
        assert got == (re.BAD if want is None else (True,) + want), e


@pytest.mark.parametrize("amod,delta,align", re.LIMIT_CASES + re.TAIL_CASES)
def test_limit_wire_claims(amod, delta, align):
    w = re.limit_wire(amod, delta, align, 3)
    rep = w.checked()
    intended(w)
    assert w.n == 256 and all(int(d) == re.MAX_RECORD or e in (9, 81) for e, d in enumerate(np.diff(w.offsets)))
    win, info = w.windows()[1], rep[1]
    assert win.A % 16 == amod and win.Bend - win.A4 == re.LIMIT + delta == w.facts["size"]
    assert win.lds == (delta <= 0) == w.facts["lds"]
    assert all(i["window"].lds for i in (rep[0], rep[2], rep[3]))
    if delta <= 0:
        assert info["rows"] == re.stage_rows(align) and 1 <= info["last_row_lanes"] <= re.WAVE
        assert info["tail"] == win.Bend % align
        if delta in re.TAIL_DELTAS[align]:
            assert win.Bend % align in ((1, 15) if align == 16 else (1, 3))
        if (delta, align) != (0, 4):  # LIMIT is a multiple of 4: at the limit itself the narrow tail is empty
            assert info["tail"] > 0
    else:
        assert info["rows"] == 0 and len(info["glob"]) == re.WAVE
    if align == 16:  # the same bytes under the forced narrow staging of the tuning build
        w.checked(4)
        assert w.parsed(4) == w.parsed()


def test_tail_set_ends_on_every_claimed_residue():
    for align, residues in ((16, {1, 15}), (4, {1, 3})):
        cases = [c for c in re.LIMIT_CASES + re.TAIL_CASES if c[2] == align and c[1] in re.TAIL_DELTAS[align]]
        assert len(cases) == 6 and len(set(re.LIMIT_CASES + re.TAIL_CASES)) == len(re.LIMIT_CASES + re.TAIL_CASES)
        assert {re.limit_wire(a, d, align, 3).windows()[1].Bend % align for a, d, _ in cases} == residues


@pytest.mark.parametrize("align", [16, 4])
def test_row_edge_wire_claims(align):
    w = re.row_edge_wire(align, 3)
    rep = w.checked()
    intended(w)
    rows = re.stage_rows(align)
    assert [i["window"].Bend - i["window"].A4 for i in rep[:2]] == list(w.facts["sizes"])
    assert w.facts["sizes"] == ((18 * 256, 18 * 256 + 4) if align == 4 else (4 * 1024, 4 * 1024 + 16))
    assert (rep[0]["rows"], rep[0]["last_row_lanes"], rep[0]["tail"]) == (rows - 1, re.WAVE, 0)
    assert (rep[1]["rows"], rep[1]["last_row_lanes"], rep[1]["tail"]) == (rows, 1, 0)
    assert all(i["window"].lds for i in rep) and w.n == 148
    if align == 16:
        narrow = w.checked(4)
        assert narrow[1]["rows"] == (4 * 1024 + 16) // 256 + 1 and w.parsed(4) == w.parsed()


FULL_WIDTH_XS = (88159051, 658814259, 702745590, 311111111, 977777777)   # test_gpu_record_edges.py's SEQ_FULL
SHIFTS = (0, 4, 8, 12, 0)


@pytest.mark.parametrize("xs,shifts", [((1, 3, 5, 7, 9), SHIFTS), (FULL_WIDTH_XS, SHIFTS), ((3,) * 5, SHIFTS),
                                       ((1, 3, 5, 7, 9), (0,) * 5), (FULL_WIDTH_XS, (0,) * 5), ((3,) * 5, (0,) * 5)])
def test_sequence_wires_claims(xs, shifts):
    wires = re.sequence_wires(xs, shifts)
    assert [w.shift for w in wires] == list(shifts) and all(w.n == re.SEQ_N == 256 + 20 for w in wires)
    firsts, lasts = set(), set()
    for i, w in enumerate(wires):
        rep = w.checked()
        intended(w)
        if not any(shifts):  # what the forced narrow staging of the tuning build touches on the same bytes
            assert all(i["rows"] <= re.STAGE_W for i in w.checked(4)) and w.parsed(4) == w.parsed()
        assert w.facts["kinds"] ==[re.SEQ[(i + wv) % 5] for wv in range(4)]
        for wv, kind in enumerate(w.facts["kinds"]):
            win, info = rep[wv]["window"], rep[wv]
            got = w.parsed()[win.e0:win.eN]
            if kind == "largest":
                assert win.lds and win.Bend - win.A4 == re.LIMIT and info["rows"] == re.stage_rows(re.align_of(w.shift))
            elif kind == "tiny":
                assert win.lds and win.Bend - win.A == 2 * re.WAVE and all(ok for ok, _, _ in got)
            elif kind == "serial":
                assert not win.lds and win.Bend - win.A4 > re.LIMIT and all(ok for ok, _, _ in got)
            else:
                assert win.lds and win.Bend == win.A and got == [re.BAD] * re.WAVE
            if wv in w.facts["ends"]:
                first, last = w.facts["ends"][wv]
                firsts.add((first, kind, win.A == win.A4))
                lasts.add((last, kind))
                if first != "y68" and win.lds and win.A == win.A4:
                    assert info["lds_read"][0] == -4     # the limb loads of a short first record reach the pad
        assert rep[4]["window"].lds and rep[4]["window"].eN - rep[4]["window"].e0 == 20
    # wave 0 of wire 0 is the sequence itself, and every special begins and ends an LDS and a byte-serial window
    assert [w.facts["kinds"][0] for w in wires] == list(re.SEQ)
    assert sorted({w.facts["kinds"][1] for w in wires}) == sorted(set(re.SEQ))
    for s in ("one-byte", "header-only"):
        assert (s, "largest", True) in firsts
    for s in re.SPECIALS:
        assert {k for f, k, _ in firsts if f == s} == {"largest", "serial"} == {k for l, k in lasts if l == s}
    assert re.counts(wires[3].parsed(), xs[3])[0] == 64 and re.counts(wires[4].parsed(), xs[4])[0] == 0


@pytest.mark.parametrize("align", [16, 4])
def test_hostile_offset_tables_are_what_they_claim(align):
    tabs = re.hostile_offsets(align)
    good = tabs["good"]
    assert re.counts(good.parsed(), re.HOSTILE_X) == (0, 0) and all(i["window"].lds for i in good.checked())
    size, raw = good.in_bytes, good.packed.tobytes()
    for name, w in tabs.items():
        rep = w.checked()
        wins = {i["window"].e0: i["window"] for i in rep}
        off = w.offsets.tolist()
        f = w.facts
        if name == "start-below-A":
            for e in f["at"]:
                win = wins[e // 64 * 64]
                assert win.lds and off[e] == win.A - 3 == win.A4 and win.A4 + 3 <= off[e + 1] <= win.Bend
                assert w.parsed()[e] == re.BAD and re.parse_record(raw, off[e], off[e + 1])[0]  # but for its start
                assert w.parsed()[e - 1] == re.BAD   # and its neighbour ends before it starts
        elif name == "end-above-Bend":
            for e in f["at"]:
                win = wins[e // 64 * 64]
                assert win.lds and win.A <= off[e] < off[e + 1] == win.Bend + 1 <= size
                assert w.parsed()[e] == re.BAD and re.parse_record(raw, off[e], off[e + 1])[0]  # but for the window
        elif name == "eN-below-e0":
            for e0 in f["serial"]:
                win = wins[e0]
                assert not win.lds and win.Bend < win.A
                inside = [e for e in range(win.e0, win.eN - 1) if off[e + 1] > win.Bend]
                assert len(inside) >= 18 and all(w.parsed()[e] == good.parsed()[e] for e in inside)
                assert w.parsed()[win.eN - 1] == re.BAD
        elif name == "eN-past-in-bytes":
            for e0 in f["serial"]:
                win = wins[e0]
                assert not win.lds and win.Bend > size and w.parsed()[win.eN - 1] == re.BAD
                assert w.parsed()[win.e0:win.eN - 1] == good.parsed()[win.e0:win.eN - 1]
        elif name == "equal-runs":
            for e in f["empty"]:
                assert off[e] == off[e + 1] and w.parsed()[e] == re.BAD
            assert re.counts(w.parsed(), re.HOSTILE_X)[0] >= 13
        elif name == "limit-plus-1":
            for e0 in f["serial"]:
                win = wins[e0]
                assert win.Bend - win.A4 == re.LIMIT + 1 and win.Bend <= size and not win.lds
        if name != "good":
            assert re.counts(w.parsed(), re.HOSTILE_X)[0] >= 2 and w.parsed() != good.parsed()


def test_corrupt_frames_open_to_what_they_claim():
    n = re.FRAME_N
    frames = re.corrupt_frames()
    assert n == 4096 + 300 and set(frames) >= {"len+1", "len-1", "all255short", "truncated", "records_bytes",
                                               "all255full", "all0", "pad-nonzero", "block-last+1", "block-first-1"}
    R = re.frame_records_offset(n)
    for kind, f in frames.items():
        lens = f.frame[32:32 + n].astype(np.int64)
        assert f.frame.size == R + f.cap and f.frame[:8].tobytes() == re.FRAME_MAGIC
        assert f.offsets.tolist() == np.minimum(np.concatenate([[0], np.cumsum(lens)]), f.cap).tolist()
        assert bool((np.diff(f.offsets) >= 0).all()) and int(f.offsets.max()) <= f.cap
        w = re.frame_wire(f)
        rep = w.checked()
        w.checked(4)
        if kind == "all255full":
            assert not any(i["window"].lds for i in rep) and 0 < re.counts(w.parsed(), f.x)[0] < n
        if kind == "all0":
            assert all(i["window"].lds and i["window"].Bend == i["window"].A for i in rep)
            assert re.counts(w.parsed(), f.x) == (n, 0)
    want_bad = {"len+1": (0, 1), "len-1": (0, 1), "all255short": (0, 1), "truncated": (1, 1), "records_bytes": (1, 0),
                "all255full": (0, 0), "all0": (0, 1), "pad-nonzero": (0, 0), "block-last+1": (0, 1),
                "block-first-1": (0, 1)}
    assert {k: f.bad for k, f in frames.items()} == want_bad
    assert frames["pad-nonzero"].frame[32 + n:R].tolist() == [0xFF] * (R - 32 - n) and R - 32 - n == 4
    assert frames["pad-nonzero"].offsets.tolist() == frames["records_bytes"].offsets.tolist()
    good = re.good_frame(n, 1, 11)
    assert good.bad == (0, 0) and re.counts(re.frame_wire(good).parsed(), 1) == (0, 0)
    re.frame_wire(good).checked()


def test_the_access_model_refuses_what_reads_out_of_bounds():
    """The premise check can fail: a table that an unchecked kernel would follow past the wire."""
    w = re.ordinary_wire(3, 70, 1)
    rep = re.accesses(w.packed.tobytes(), w.offsets.tolist(), w.in_bytes - 1, w.n, 16)
    assert not rep[1]["window"].lds and (int(w.offsets[69]), int(w.offsets[70])) not in rep[1]["glob"]
    over = re.Wire(w.packed, w.offsets, 3)
    over.packed = over.packed[:-1]           # the wire lost its last byte: the model never reads it
    over.checked()
    assert over.parsed()[69] == re.BAD and over.parsed()[:64] == w.parsed()[:64]
