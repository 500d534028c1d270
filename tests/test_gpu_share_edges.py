"""check_shares_vec, check_records_vec and resolve_shares_vec_robust (MI355X) on the abscissa sets and rows of
test_share_edges_host.py: divisor shifts of 10 and more, weights next to 2^32, every r at even and odd k,
k = 2 and 3, saturated accumulators, chosen residues in front of the final division, the non-canonical p
— and, for the two tiled-vector kernels, live lanes whose top halfword carries bits above bit 8.  n is 65 and
257: one element past a wave, one past a tile, junk in the padding lanes.  Everything against the definition
in Python integers: every comparison is exact."""
import functools
import random

import pytest
import torch

import share_check_cases as cases
import share_robust_cases as robust
import wire_edges as we
from delta_node.crypto import shamir
from delta_node.crypto.shamir import field
from delta_node.crypto.shamir import shamir as shamir_mod

pytestmark = pytest.mark.gpu

P = cases.P
SIZES = [65, 257]
TOP_JUNK = 0xFE  # bits 9..15 of the top plane's halfword, as bits 1..7 of its high byte


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", torch.cuda.current_device())


@functools.lru_cache(maxsize=None)
def reference(t, xs):
    """(rows, [(culprit byte, value or None)]) of one set: the edge rows first, then the generic ones."""
    if (t, xs) in robust.ROBUST_EDGE:
        rows = robust.edge_rows(t, xs)[0] + robust.rows(t, xs)
        return rows, [robust.want(t, xs, ys) for ys in rows]
    rows = cases.edge_rows(t, xs)[0] + cases.rows(t, xs)
    return rows, [(cases.verdict(xs, ys, t), None) for ys in rows]


@functools.lru_cache(maxsize=None)
def host_block(t, xs, n):
    """The k host vectors of n elements, element e holding row e % len(rows), junk in the padding lanes."""
    rows, _ = reference(t, xs)
    assert len(rows) <= 65  # so that n = 65 holds every row
    junk = random.Random(n)
    block = [rows[e % len(rows)] for e in range(n)] + [[junk.randrange(P) for _ in xs] for _ in range(-n % field.TILE)]
    return [field.ints_to_vec([ys[i] for ys in block]) for i in range(len(xs))]


def device_rows(t, xs, n, top_junk):
    vecs = host_block(t, xs, n)
    if top_junk:  # what the 16-bit top plane carries above bit 8 is not part of the value
        vecs = [v.copy().reshape(-1, field.TILE_BYTES) for v in vecs]
        for v in vecs:
            v[:, 64 * field.TILE + 1::2] |= TOP_JUNK
        vecs = [v.reshape(-1) for v in vecs]
        assert all(int(l[16]) >> 9 == TOP_JUNK >> 1 for l in field.vec_to_limbs(vecs[0], n))
    return [torch.from_numpy(v).to(dev()) for v in vecs]


def expected(t, xs, n):
    rows, ref = reference(t, xs)
    marks = [ref[e % len(rows)][0] for e in range(n)]
    values = [ref[e % len(rows)][1] for e in range(n)]
    return marks, values, sum(m != 0xFF for m in marks), sum(m < 0xFE for m in marks)


def values(res, out, n):
    return field.vec_to_ints(res.cpu().numpy(), n) if out == "field" else [v % (1 << 64) for v in res.cpu().tolist()]


@pytest.mark.parametrize("top_junk", [False, True], ids=["canonical", "top-junk"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("t, xs", robust.ROBUST_EDGE + cases.EDGE)
def test_check_shares_vec(t, xs, n, top_junk):
    marks, _, n_bad, n_found = expected(t, xs, n)
    vecs = device_rows(t, xs, n, top_junk)
    ss = shamir.SecretShare(t)
    assert ss.check_shares_vec(vecs, xs, n) == n_bad
    count, got = ss.check_shares_vec(torch.stack(vecs), xs, n, culprit=True)
    assert count == n_bad and got.cpu().tolist() == marks
    counts = torch.zeros(2, dtype=torch.int32, device=dev())
    ss.check_shares_vec(vecs, xs, n, culprit=True, bad=counts)
    assert counts.tolist() == [n_bad, n_found]


@pytest.mark.parametrize("top_junk", [False, True], ids=["canonical", "top-junk"])
@pytest.mark.parametrize("out", ["field", "int64"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("t, xs", robust.ROBUST_EDGE)
def test_resolve_shares_vec_robust(t, xs, n, out, top_junk):
    marks, want, n_bad, n_found = expected(t, xs, n)
    vecs = device_rows(t, xs, n, top_junk)
    ss = shamir.SecretShare(t)
    res, count, got_marks = ss.resolve_shares_vec_robust(vecs, xs, n, out=out, culprit=True)
    assert count == (n_bad, n_found) and got_marks.cpu().tolist() == marks
    got = values(res, out, n)
    assert got == [v % (P if out == "field" else 1 << 64) for v in want]
    if out == "field" and not top_junk:
        # where nothing is located: resolve_shares_vec over all k rows, bit for bit (on canonical shares, its contract)
        rows, _ = reference(t, xs)
        plain = [e for e in range(n) if marks[e] >= 0xFE and all(y < P for y in rows[e % len(rows)])]
        full = values(ss.resolve_shares_vec(vecs, xs, n, out="field"), out, n)
        assert len(plain) >= 8 and [got[e] for e in plain] == [full[e] for e in plain]


@pytest.mark.parametrize("t, xs", robust.ROBUST_EDGE + cases.EDGE)
def test_check_records_vec(t, xs):
    n = 65
    rows, _ = reference(t, xs)
    marks, _, n_bad, n_found = expected(t, xs, n)
    wires = []
    for i, x in enumerate(xs):
        packed, offsets = we.pack_records([shamir_mod._share_to_bytes((x, rows[e % len(rows)][i])) for e in range(n)])
        wires.append((torch.from_numpy(packed).to(dev()), torch.from_numpy(offsets).to(dev())))
    counts = torch.zeros(2, dtype=torch.int32, device=dev())
    rec = torch.zeros(2, dtype=torch.int32, device=dev())
    ss = shamir.SecretShare(t)
    none, got = ss.check_records_vec(wires, xs, n, culprit=True, bad=counts, bad_records=rec)
    assert none is None and got.cpu().tolist() == marks
    assert counts.tolist() == [n_bad, n_found] and rec.tolist() == [0, 0]
    assert ss.check_records_vec(wires, xs, n) == n_bad


@pytest.mark.parametrize("wire", [2, 1])
def test_a_whole_bad_wire_on_the_shift_set(wire):
    """One share of every element is another field element: every lane of every wave takes the correction,
    with the divisor 175 * 2^29 for share 2 and with the set's shift-32 divisor, 35 * 2^32, for share 1."""
    t, xs, n, rng = 2, (1, 17, 33, 129, 257), 257, random.Random(wire)
    assert [robust.odd_and_shift(v) for v in robust.divisors(xs)][1:3] == [(35, 32), (175, 29)]
    polys = [[rng.randrange(P) for _ in range(t)] for _ in range(n)]
    block = [[sum(c * x ** j for j, c in enumerate(f)) % P for x in xs] for f in polys]
    for ys in block:
        ys[wire] = (ys[wire] + 1 + rng.randrange(P - 1)) % P  # a random field element that is not the share
    vecs = [torch.from_numpy(field.ints_to_vec([ys[i] for ys in block])).to(dev()) for i in range(len(xs))]
    res, count, marks = shamir.SecretShare(t).resolve_shares_vec_robust(vecs, xs, n, out="field", culprit=True)
    assert count == (n, n) and marks.cpu().tolist() == [wire] * n
    assert values(res, "field", n) == [f[0] for f in polys]
