"""The record-reading kernels (csrc/recon_records.hip, csrc/sum_records.hip) and
the frames that feed them (csrc/codec_frame.hip) where their feature suites do
not reach: windows at the limit of the LDS slice and at the last staging row,
with the window's tail bytes live; window sequences that reuse one LDS slice
for a large, a tiny, a byte-serial and an empty window; offset tables that
point outside a window; the canonical zero; corrupted frames opened and handed
on as they stand; and the staging forms of the tuning build.

Every expectation is tests/record_edges.py's Python integers (a model of the
contract, never the library), every comparison is bit for bit, every output
sits between canaries, both record counts are compared exactly, and the inputs
must be unchanged after the call.  Before a wire is uploaded the access model
must find every access it implies in bounds (record_edges.assert_in_bounds).
Each test asserts the premise it rests on (rows reached, path taken) from
record_edges, so a change of the geometry moves the inputs, not the coverage.
"""
import numpy as np
import pytest
import torch

import record_edges as re
import wire_edges as we
from delta_node.crypto import shamir
from delta_node.crypto.shamir import _args, _native, codec, field

pytestmark = pytest.mark.gpu

P = re.P
CANARY = 0xC3
I64_CANARY = -0x0123456789ABCDEF
GUARD = 64
SS = shamir.SecretShare(2)


def dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _native.lib()


def up(a: np.ndarray, shift: int = 0):
    """A device copy of `a` whose address is `shift` bytes past a 16-byte boundary (uint8 only when shifted)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not shift:
        out = t.to(dev())
    else:
        big = torch.empty(t.numel() + 16, dtype=torch.uint8, device=dev())
        out = big[shift:shift + t.numel()]
        out.copy_(t)
    assert out.data_ptr() % 16 == shift
    return out


def upload(w: re.Wire, align=None):
    """The device pair of a wire — only once the access model has found it in bounds."""
    w.checked(align)
    return up(w.packed, w.shift), up(w.offsets)


def field_ints(vec, n):
    return we.limbs_to_ints(field.vec_to_limbs(vec.cpu().numpy(), n))


def tiled(vals):
    return up(we.tiles_of(we.ints_to_limbs(vals)))


def untouched(n):
    """Mask of the bytes of a tiled vector that belong to no element."""
    pos, _ = we.scatter_tiles(np.arange(n), np.zeros((n, we.LIMBS), dtype=np.uint32))
    mask = torch.ones(field.vec_bytes(n), dtype=torch.bool, device=dev())
    mask[up(pos)] = False
    return mask


def unchanged(pairs, keep):
    return all(torch.equal(p, kp) and torch.equal(o, ko) for (p, o), (kp, ko) in zip(pairs, keep))


def run_resolve(wires, xs, n, aligns=None, dev_wires=None):
    """dn_m521_reconstruct_records with both outputs between canaries, then the
    method with a deferred flag; everything against want_resolve.  Returns the
    weights' descriptor (the kernel family is the caller's premise)."""
    aligns = aligns or [None] * len(wires)
    want = re.want_resolve(wires, xs, n, aligns)
    pairs = dev_wires or [upload(w, a) for w, a in zip(wires, aligns)]
    keep = [(p.clone(), o.clone()) for p, o in pairs]
    lag = _native.lagrange(xs, 2)
    _, desc = _args.aligned_wires(pairs)
    vb = field.vec_bytes(n)
    big_i = torch.full((n + 2 * GUARD,), I64_CANARY, dtype=torch.int64, device=dev())
    big_f = torch.full((vb + 2 * GUARD,), CANARY, dtype=torch.uint8, device=dev())
    out_f = big_f[GUARD:GUARD + vb]
    bad = torch.zeros(2, dtype=torch.int32, device=dev())
    over = torch.zeros(1, dtype=torch.int32, device=dev())
    _native.reconstruct_records(desc, xs, lag, bad, out_fe=out_f, out_u64=big_i[GUARD:GUARD + n], overflow=over, n=n)
    what = (xs, n)
    assert bad.tolist() == [want["bad"], want["mis"]], what
    assert big_i[GUARD:GUARD + n].tolist() == want["i64"], what
    assert field_ints(out_f, n) == want["field"], what
    assert int(over.item()) == want["overflow"], what
    assert bool((big_i[:GUARD] == I64_CANARY).all()) and bool((big_i[GUARD + n:] == I64_CANARY).all()), what
    assert bool((big_f[:GUARD] == CANARY).all()) and bool((big_f[GUARD + vb:] == CANARY).all()), what
    assert bool((out_f[untouched(n)] == CANARY).all()), what
    flag = torch.zeros(2, dtype=torch.int32, device=dev())
    res, ov = SS.resolve_records_vec(pairs, xs, n, return_overflow=True, bad=flag)
    assert res.tolist() == want["i64"] and int(ov.item()) == want["overflow"], what
    assert flag.tolist() == [want["bad"], want["mis"]], what
    assert unchanged(pairs, keep), what
    return lag


def run_sum(wires, x, n, signs=None, acc=None, aligns=None, dev_wires=None):
    """sum_records_vec with a deferred flag into a canary-guarded `out`: without
    acc, or with acc separate and with acc is out; all vec_bytes(n) bytes."""
    aligns = aligns or [None] * len(wires)
    want = re.want_sum(wires, x, n, signs, acc, aligns)
    want_vec = tiled(want["field"])
    pairs = dev_wires or [upload(w, a) for w, a in zip(wires, aligns)]
    keep = [(p.clone(), o.clone()) for p, o in pairs]
    vb = field.vec_bytes(n)
    for in_place in ((False,) if acc is None else (False, True)):
        big = torch.full((vb + 2 * GUARD,), CANARY, dtype=torch.uint8, device=dev())
        out = big[GUARD:GUARD + vb]
        acc_t = None
        if acc is not None:
            acc_t = tiled(acc)
            if in_place:
                out.copy_(acc_t)
                acc_t = out
        flag = torch.zeros(2, dtype=torch.int32, device=dev())
        got = SS.sum_records_vec(pairs, x, n, signs=signs, acc=acc_t, out=out, bad=flag)
        what = (x, n, signs, in_place)
        assert got is out and flag.tolist() == [want["bad"], want["mis"]], what
        assert torch.equal(out, want_vec), what
        assert bool((big[:GUARD] == CANARY).all()) and bool((big[GUARD + vb:] == CANARY).all()), what
        if acc is not None and not in_place:
            assert torch.equal(acc_t, tiled(acc)), what
    assert unchanged(pairs, keep), what


# ---------------------------------------------------------------- 1. the window limit and the last staging row
XS3, XS4 = [1, 3, 5], [1, 3, 5, 7]
SIGNS3 = [1, -1, 1]


def edge_builders():
    out = [(f"limit-a{a}-d{d}-w{al}", al, lambda x, a=a, d=d, al=al: re.limit_wire(a, d, al, x))
           for a, d, al in re.LIMIT_CASES + re.TAIL_CASES]
    out += [(f"rows-w{al}", al, lambda x, al=al: re.row_edge_wire(al, x)) for al in (16, 4)]
    return out


EDGES = edge_builders()


def edge_premise(name, w, align):
    """The wire reaches what its name says under the staging width in use."""
    rep = w.checked(align)
    rows = re.stage_rows(align)
    if name.startswith("rows"):
        if align == re.align_of(w.shift):
            assert [(i["rows"], i["last_row_lanes"]) for i in rep[:2]] == [(rows - 1, 64), (rows, 1)]
    elif w.facts["lds"] and align == re.align_of(w.shift):
        assert rep[1]["window"].lds and rep[1]["rows"] == rows
        assert rep[1]["window"].Bend - rep[1]["window"].A4 == w.facts["size"]
    elif align == re.align_of(w.shift):
        assert not rep[1]["window"].lds


def run_edge(name, align, build, positions, force_align=None, k4=True):
    """The edge wire as wire 0, wire 1 and the last one among ordinary wires:
    resolve with K = 3 (one-limb weights: the unrolled kernel in the product
    build) and with k = 4 (the runtime-k kernel), sum with signs (+, -, +)."""
    shift = 0 if align == 16 else 4
    for pos in positions:
        for xs in ([XS3, XS4] if k4 else [XS3]):
            at = pos if pos < 2 else len(xs) - 1
            wires = [build(x) if i == at else re.ordinary_wire(x, build(x).n, 50 + i, shift if i % 2 else 0)
                     for i, x in enumerate(xs)]
            n = wires[at].n
            aligns = [force_align] * len(xs) if force_align else None
            edge_premise(name, wires[at], force_align or align)
            lag = run_resolve(wires, xs, n, aligns)
            assert lag.a_limbs == 1 and lag.k == len(xs)
        wires = [build(3) if i == pos else re.ordinary_wire(3, build(3).n, 60 + i, shift if i % 2 else 0)
                 for i in range(3)]
        run_sum(wires, 3, wires[pos].n, SIGNS3, aligns=[force_align] * 3 if force_align else None)


@pytest.mark.parametrize("name,align,build", EDGES, ids=[e[0] for e in EDGES])
def test_window_limit_and_last_staging_row(name, align, build):
    """Bend - A4 at LIMIT - 1, LIMIT and LIMIT + 1 with the first byte at 0, 1
    and 15 (mod 16), on both staging widths; windows that end on 1 and 15 (mod
    16) and on 1 and 3 (mod 4) with the last staging row in use, so that the
    tail bytes are live; and windows that end exactly one row short of the
    register file and one load into its last row."""
    run_edge(name, align, build, positions=(0, 1, 2))


# ---------------------------------------------------------------- 2. window sequences
SEQ_ONE_LIMB = (1, 3, 5, 7, 9)
SEQ_FULL = (88159051, 658814259, 702745590, 311111111, 977777777)
SEQ_SIGNS = [1, -1, -1, 1, -1]


def run_sequence(order, shifts=(0, 4, 8, 12, 0), force_align=None):
    n = re.SEQ_N
    aligns = [force_align] * 5 if force_align else None
    for xs, limbs in ((SEQ_ONE_LIMB, 1), (SEQ_FULL, 17)):
        wires = re.sequence_wires(xs, shifts)
        assert [w.facts["kinds"][0] for w in wires] == list(re.SEQ)
        pick = [wires[i] for i in order]
        lag = run_resolve(pick, [xs[i] for i in order], n, aligns)
        assert (lag.a_limbs, lag.k) == (limbs, 5)
    wires = re.sequence_wires((3,) * 5, shifts)
    acc = we.limbs_to_ints(we.ragged_limbs(n, 31))
    run_sum([wires[i] for i in order], 3, n, [SEQ_SIGNS[i] for i in order], acc, aligns)


@pytest.mark.parametrize("order", [(0, 1, 2, 3, 4), (4, 3, 2, 1, 0)], ids=["forward", "reversed"])
def test_window_sequences_share_one_lds_slice(order):
    """k = m = 5 wires at alignments 0, 4, 8, 12, 0: a wave's slice holds, wire
    after wire, the largest window, 64 two-byte records, nothing (byte-serial),
    an empty window and the largest again, while its neighbours hold rotations
    of that; one-limb and full-width weights; mixed signs onto an acc."""
    run_sequence(order)


# ---------------------------------------------------------------- 3. hostile offsets
def decode(pair, n):
    flag = torch.zeros(1, dtype=torch.int32, device=dev())
    buf = torch.zeros(field.vec_bytes(n), dtype=torch.uint8, device=dev())
    vec, _ = codec.decode_share_vec(pair[0], pair[1], n, out=buf, bad=flag)
    return vec, int(flag.item())


TABLES = sorted(re.hostile_offsets(16))


@pytest.mark.parametrize("align", [16, 4])
@pytest.mark.parametrize("table", TABLES)
def test_hostile_offsets_in_one_wire(table, align):
    """Wire 1 of 3 carries an offsets table that points below its window's A,
    above its Bend, backwards, past the wire, nowhere (equal offsets) or one
    byte over the window limit, in a full wave and in the last, partial one.
    Values and both counts are the model's; decode_share_vec then
    resolve_shares_vec / sum_shares_vec is a second witness."""
    n, x = re.HOSTILE_N, re.HOSTILE_X
    xs = [1, x, 5]
    hostile = re.hostile_offsets(align)[table]
    wires = [re.ordinary_wire(1, n, 71), hostile, re.ordinary_wire(5, n, 72)]
    run_resolve(wires, xs, n)
    want = re.want_resolve(wires, xs, n)
    pairs = [upload(w) for w in wires]
    dec = [decode(p, n) for p in pairs]
    assert sum(d[1] for d in dec) == want["bad"] == re.counts(hostile.parsed(), x)[0]
    res = SS.resolve_shares_vec([d[0] for d in dec], xs, n, out="field")
    assert field_ints(res, n) == want["field"]
    sums = [re.ordinary_wire(x, n, 73), hostile, re.ordinary_wire(x, n, 74)]
    run_sum(sums, x, n, SIGNS3)
    pairs = [upload(w) for w in sums]
    dec = [decode(p, n) for p in pairs]
    want = re.want_sum(sums, x, n, SIGNS3)
    assert sum(d[1] for d in dec) == want["bad"]
    assert torch.equal(SS.sum_shares_vec([d[0] for d in dec], signs=SIGNS3), tiled(want["field"]))


# ---------------------------------------------------------------- 4. the canonical zero
def test_a_negated_zero_is_stored_as_zero():
    """A subtracted wire whose records are y = 0, y = p and bad contributes
    p - 0 = p, p - p = 0 and p (a 68-byte multiple of p among them): the stored element is 0, never p — alone, onto
    acc = 0, and where acc = p - 1 and a wire of ones make p before it.
    (test_gpu_sum_records.py's test_value_edges_in_one_wire_set has y = 0 and
    y = p under sign -1 only inside sums of G wires whose total is not 0 mod p,
    and no bad record: none of the runs below is asserted there.)"""
    x, n = 3, 70
    kinds = [re.rec(x, 0), re.rec(x, P), bytes([9]) + bytes(12), re.rec(x, 0, 5), re.rec(x, P << 22)]
    zero = re.from_records([kinds[e % len(kinds)] for e in range(n)], x)
    assert all(y % P == 0 for _, _, y in zero.parsed()) and re.counts(zero.parsed(), x) == (n // 5, 0)
    ones = re.from_records([re.rec(x, 1)] * n, x)
    for signs, wires, acc in (([-1], [zero], None), ([-1], [zero], [0] * n), ([1, -1], [ones, zero], [P - 1] * n),
                              ([-1, 1], [zero, zero], None)):
        assert re.want_sum(wires, x, n, signs, acc)["field"] == [0] * n
        run_sum(wires, x, n, signs, acc)
    # the same records under a negative Lagrange weight
    xs = [1, 3, 5]
    lag = run_resolve([re.from_records([kinds[e % len(kinds)].replace(bytes([1, x]), bytes([1, a]), 1)
                                        for e in range(n)], a) for a in xs], xs, n)
    assert lag.neg != 0


# ---------------------------------------------------------------- 5. frames into records
KINDS = sorted(re.corrupt_frames())


@pytest.mark.parametrize("kind", KINDS)
def test_corrupt_frames_open_to_offsets_the_record_kernels_can_take(kind):
    """[good, corrupt, good] through open_frames with a deferred flag, then the
    three (packed, offsets) pairs as they stand through sum_records_vec and
    resolve_records_vec: the opened offsets are min(cumsum, cap), the frame
    counts and the record counts are exact, the results are the model's on
    those offsets, and the frames are unchanged."""
    n = re.FRAME_N
    xs = [1, 3, 5]
    model = [re.good_frame(n, 1, 11), re.corrupt_frames()[kind], re.good_frame(n, 5, 12)]
    wires = [re.frame_wire(f) for f in model]
    for w in wires:
        w.checked()
    frames = [up(f.frame) for f in model]
    keep = [f.clone() for f in frames]
    flag = torch.zeros(2, dtype=torch.int32, device=dev())
    opened = codec.open_frames(frames, n, xs, bad=flag)
    assert flag.tolist() == [sum(f.bad[0] for f in model), sum(f.bad[1] for f in model)]
    for (p, o), f in zip(opened, model):
        assert p.numel() == f.cap and p.data_ptr() % 16 == 0 and torch.equal(o, up(f.offsets)), kind
    run_sum(wires, 3, n, SIGNS3, dev_wires=opened)
    run_resolve(wires, xs, n, dev_wires=opened)
    assert all(torch.equal(a, b) for a, b in zip(frames, keep))
    for (p, o), f in zip(opened, model):
        assert torch.equal(o, up(f.offsets)), kind


# ---------------------------------------------------------------- 6. the staging forms of the tuning build
MODES = {
    "ahead": {"DN_RR_STAGE": "1", "DN_SR_STAGE": "1"},
    "direct": {"DN_RR_STAGE": "2", "DN_SR_STAGE": "2"},
    "serial-by-knob": {"DN_RR_STAGE": "0", "DN_SR_STAGE": "0"},
    "narrow": {"DN_DECODE_W4": "1"},
    "runtime-k": {"DN_RR_UNROLL": "0"},
}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_staging_forms_of_the_tuning_build(mode, monkeypatch):
    """The limit, row and sequence cases under kAhead and kDirect of both
    kernels, under the forced narrow staging of 16-byte-aligned wires, and with
    K = 3 through the runtime-k kernel: the same values and counts.  (Each edge
    wire at one position, rotating; test 1 has all three in the product form.)"""
    for name, value in MODES[mode].items():
        monkeypatch.setenv(name, value)
    narrow = mode == "narrow"
    with _native.library(_native.TUNING_LIB):
        for i, (name, align, build) in enumerate(EDGES):
            if narrow and align != 16:
                continue
            run_edge(name, align, build, positions=(i % 3,), force_align=4 if narrow else None, k4=False)
        for order in ((0, 1, 2, 3, 4), (4, 3, 2, 1, 0)):
            if narrow:
                run_sequence(order, shifts=(0,) * 5, force_align=4)
            else:
                run_sequence(order)
