"""resolve_records_vec_robust / dn_m521_reconstruct_records_robust (MI355X): every value, both counts
and every culprit byte against the definition in Python integers (share_robust_cases.py) and against
the route it replaces on the same wires — decode_share_vec on every wire, then
resolve_shares_vec_robust.  Integer arithmetic: every comparison is exact."""
import functools
import random

import numpy as np
import pytest
import torch

import share_robust_cases as robust
import wire_edges as we
from delta_node.crypto import shamir
from delta_node.crypto.shamir import _native, codec, field
from delta_node.crypto.shamir import shamir as shamir_mod

pytestmark = pytest.mark.gpu

GUARD, P, XS5 = 64, robust.P, (1, 2, 3, 4, 5)


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def wire(recs, shift=0):
    """The (packed, offsets) device pair of records; `packed` lies `shift` bytes past a 16-byte boundary."""
    p, o = we.pack_records(recs)
    buf = torch.empty(p.size + 16, dtype=torch.uint8, device=dev())[shift:shift + p.size]
    buf.copy_(torch.from_numpy(p))
    assert buf.data_ptr() % 16 == shift
    return buf, torch.from_numpy(o).to(dev())


def share_wire(x, ys, shift=0):
    return wire([shamir_mod._share_to_bytes((x, y)) for y in ys], shift)


@functools.lru_cache(maxsize=None)
def reference(t, xs):
    rows = robust.rows(t, xs)
    return rows, [robust.want(t, xs, ys) for ys in rows]


def values(res, out, n):
    return field.vec_to_ints(res.cpu().numpy(), n) if out == "field" else [v % (1 << 64) for v in res.cpu().tolist()]


def zeros2():
    return torch.zeros(2, dtype=torch.int32, device=dev())


def decode_route(wires, xs, n, t, out):
    """decode_share_vec on every wire, then resolve_shares_vec_robust: (values, counts, culprit bytes)."""
    skip = torch.zeros(1, dtype=torch.int32, device=dev())
    vecs = [codec.decode_share_vec(p, o, n, out=torch.zeros(field.vec_bytes(n), dtype=torch.uint8, device=dev()),
                                   bad=skip)[0] for p, o in wires]
    res, count, marks = shamir.SecretShare(t).resolve_shares_vec_robust(vecs, xs, n, out=out, culprit=True)
    return values(res, out, n), count, marks.cpu().tolist()


def records_route(wires, xs, n, t, out):
    """The fully deferred form: (values, counts, culprit bytes, record counts)."""
    bad, rec = zeros2(), zeros2()
    res, none, marks = shamir.SecretShare(t).resolve_records_vec_robust(wires, xs, n, out=out, culprit=True, bad=bad,
                                                                        bad_records=rec)
    assert none is None and marks.dtype == torch.uint8
    return values(res, out, n), tuple(bad.tolist()), marks.cpu().tolist(), rec.tolist()


# ---------------------------------------------------------------- 1. the definition
@pytest.mark.parametrize("out", ["field", "int64"])
@pytest.mark.parametrize("t, xs, n", [(t, xs, n) for t, xs in robust.CASES for n in (1, 64, 65, 256, 257, 513)]
                         + [(t, xs, 65) for t, xs in robust.MORE])
def test_values_counts_and_culprits_match_the_definition(t, xs, n, out):
    rows, ref = reference(t, xs)
    marks = [ref[e % len(rows)][0] for e in range(n)]
    want = [ref[e % len(rows)][1] % (P if out == "field" else 1 << 64) for e in range(n)]
    count = (sum(m != 0xFF for m in marks), sum(m < 0xFE for m in marks))
    wires = [share_wire(x, [rows[e % len(rows)][i] for e in range(n)]) for i, x in enumerate(xs)]
    ss = shamir.SecretShare(t)

    # the method: the read-back form with xs read from the wires, the deferred form, the decode route
    res, got_count, got_marks = ss.resolve_records_vec_robust(wires, None, n, out=out, culprit=True)
    assert (values(res, out, n), got_count, got_marks.cpu().tolist()) == (want, count, marks)
    assert records_route(wires, xs, n, t, out) == (want, count, marks, [0, 0])
    assert decode_route(wires, xs, n, t, out) == (want, count, marks)

    # the entry point, twice into pre-loaded counters: canaries around the culprit bytes and the int64
    # words, and a marker in the padding lanes of a field output's last tile
    plan = _native.robust_plan(xs, t)
    desc = [(p.data_ptr(), p.numel(), o.data_ptr()) for p, o in wires]
    counts = torch.tensor([5, 7], dtype=torch.int32, device=dev())
    rec = torch.tensor([3, 9], dtype=torch.int32, device=dev())
    buf = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device=dev())
    words = torch.full((GUARD + n + GUARD,), -3, dtype=torch.int64, device=dev())
    fe = torch.full((field.vec_bytes(n),), 0x5A, dtype=torch.uint8, device=dev())
    for _ in range(2):
        _native.reconstruct_records_robust(desc, xs, plan, counts, rec, fe if out == "field" else None,
                                           words[GUARD:GUARD + n] if out == "int64" else None, buf[GUARD:GUARD + n], n)
    assert counts.tolist() == [5 + 2 * count[0], 7 + 2 * count[1]] and rec.tolist() == [3, 9]
    host = buf.cpu().numpy()
    assert np.all(host[:GUARD] == 0xA5) and np.all(host[GUARD + n:] == 0xA5) and host[GUARD:GUARD + n].tolist() == marks
    assert torch.all(words[:GUARD] == -3) and torch.all(words[GUARD + n:] == -3)
    assert values(fe if out == "field" else words[GUARD:GUARD + n], out, n) == want
    if out == "field" and n in (65, 257):
        last = fe.cpu().numpy()[-66 * field.TILE:]
        assert np.all(last[:64 * field.TILE].reshape(16, field.TILE, 4)[:, n % field.TILE:] == 0x5A)
        assert np.all(last[64 * field.TILE:].reshape(field.TILE, 2)[n % field.TILE:] == 0x5A)


# ---------------------------------------------------------------- 2. wires that differ
def test_wires_differ_in_alignment_and_path():
    """`packed` at 0, 4 and 12 bytes from a 16-byte boundary (both staging paths in one launch); wire
    3's records carry 30 leading zero bytes, so its full waves take the byte-serial path while its tail
    wave and the other wires stay in LDS; wire 4 is a misaligned view (copied once)."""
    t, xs, n = 3, XS5, 130
    rows, ref = reference(t, xs)
    col = [[rows[e % len(rows)][i] for e in range(n)] for i in range(5)]
    padded = wire([bytes([1, 4]) + bytes(30) + y.to_bytes(66, "big") for y in col[3]])
    wires = [share_wire(1, col[0]), share_wire(2, col[1], 4), share_wire(3, col[2], 12), padded,
             share_wire(5, col[4], 3)]
    assert [p.data_ptr() % 16 for p, _ in wires] == [0, 4, 12, 0, 3]
    o3 = padded[1].cpu().numpy()
    assert all(we.decode_window(o3, e0, n, 16) > we.DEC_WINDOW_LIMIT for e0 in (0, 64))  # its two full waves
    assert we.decode_window(o3, 128, n, 16) <= we.DEC_WINDOW_LIMIT  # (the two-record tail wave fits LDS)
    for out in ("field", "int64"):
        got = records_route(wires, xs, n, t, out)
        assert got[:3] == decode_route(wires, xs, n, t, out) and got[3] == [0, 0]
        assert got[0] == [ref[e % len(rows)][1] % (P if out == "field" else 1 << 64) for e in range(n)]
        assert got[2] == [ref[e % len(rows)][0] for e in range(n)]


# ---------------------------------------------------------------- 3. a damaged wire
@pytest.mark.parametrize("bad_wire", [0, 2, 4])
def test_a_damaged_wire_is_repaired(bad_wire):
    t, xs, n, rng = 3, XS5, 257, random.Random(bad_wire)
    polys = [[rng.randrange(P) for _ in range(t)] for _ in range(n)]
    col = [[sum(c * x ** j for j, c in enumerate(f)) % P for f in polys] for x in xs]
    col[bad_wire] = [(y + 1 + rng.randrange(P - 1)) % P for y in col[bad_wire]]  # field elements that are not the shares
    recs = [[shamir_mod._share_to_bytes((x, y)) for y in ys] for x, ys in zip(xs, col)]
    secrets = [f[0] for f in polys]
    ss = shamir.SecretShare(t)
    res, count, marks = ss.resolve_records_vec_robust([wire(r) for r in recs], xs, n, out="field", culprit=True)
    assert (values(res, "field", n), count, marks.cpu().tolist()) == (secrets, (n, n), [bad_wire] * n)
    # two unrepresentable records in that wire: an empty one, and a y of 69 bytes
    recs[bad_wire][70], recs[bad_wire][256] = b"", bytes([1, xs[bad_wire], 1]) + bytes(68)
    wires = [wire(r) for r in recs]
    got = records_route(wires, xs, n, t, "field")
    assert got == (secrets, (n, n), [bad_wire] * n, [2, 0])
    assert got[:3] == decode_route(wires, xs, n, t, "field")
    with pytest.raises(ValueError, match="^resolve_records_vec_robust: 2 records with x > 8 bytes or y > 68 bytes, "
                                         "0 records whose x is not their wire's abscissa$"):
        ss.resolve_records_vec_robust(wires, xs, n)


# ---------------------------------------------------------------- 4. one capture
def test_the_deferred_form_under_one_capture():
    t, xs, n = 3, (1, 3, 4, 7, 9), 257
    rows, ref = reference(t, xs)
    wires = [share_wire(x, [rows[e % len(rows)][i] for e in range(n)]) for i, x in enumerate(xs)]
    ss = shamir.SecretShare(t)
    eager, count, eager_marks = ss.resolve_records_vec_robust(wires, xs, n, out="field", culprit=True)
    assert values(eager, "field", n) == [ref[e % len(rows)][1] for e in range(n)]
    bad, rec = zeros2(), zeros2()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res, none, marks = ss.resolve_records_vec_robust(wires, xs, n, out="field", culprit=True, bad=bad,
                                                         bad_records=rec)
    assert none is None
    for replay in (1, 2, 3):
        res.fill_(0)
        marks.fill_(0)
        graph.replay()
        assert bad.tolist() == [replay * count[0], replay * count[1]] and rec.tolist() == [0, 0]
        assert values(res, "field", n) == values(eager, "field", n) and torch.equal(marks, eager_marks)
