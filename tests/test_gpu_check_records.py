"""check_records_vec / dn_m521_check_records (MI355X): the count and every
culprit byte against the definition in Python integers (share_check_cases.py)
and against the existing route on the same wires — decode_share_vec on every
wire, then check_shares_vec; the two record counts against resolve_records_vec.
Integer arithmetic: every comparison is exact.

The grid is one workgroup per 256 elements (csrc/check_records.hip: no cap, no
grid stride), so there is no second-unit case to test.
"""
import functools

import numpy as np
import pytest
import torch

import share_check_cases as cases
import wire_edges as we
from delta_node.crypto import shamir
from delta_node.crypto.shamir import _native, codec, field
from delta_node.crypto.shamir import shamir as shamir_mod

pytestmark = pytest.mark.gpu

P = cases.P
GUARD = 64
XS5 = (1, 2, 3, 4, 5)


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", torch.cuda.current_device())


def up(a: np.ndarray, shift: int = 0):
    """A device copy of `a` whose address is `shift` bytes past a 16-byte boundary."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not shift:
        return t.to(dev())
    out = torch.empty(t.numel() + 16, dtype=torch.uint8, device=dev())[shift:shift + t.numel()]
    out.copy_(t)
    assert out.data_ptr() % 16 == shift
    return out


def raw_wire(recs, shift: int = 0):
    """(packed, offsets) device pair of hand-built records, and the host offsets."""
    p, o = we.pack_records(recs)
    return (up(p, shift), up(o)), o


def share_wire(x, ys, shift: int = 0):
    return raw_wire([shamir_mod._share_to_bytes((x, y)) for y in ys], shift)[0]


@functools.lru_cache(maxsize=None)
def case_rows(t, xs):
    rows = cases.rows(t, xs)
    return rows, [cases.verdict(xs, ys, t) for ys in rows]


def zeros2():
    return torch.zeros(2, dtype=torch.int32, device=dev())


def decode_route(wires, xs, n, t):
    """decode_share_vec on every wire, then check_shares_vec: ([inconsistent, located], culprit bytes)."""
    skip = torch.zeros(1, dtype=torch.int32, device=dev())
    vecs = [codec.decode_share_vec(p, o, n, out=torch.zeros(field.vec_bytes(n), dtype=torch.uint8, device=dev()),
                                   bad=skip)[0] for p, o in wires]
    counts = zeros2()
    _, marks = shamir.SecretShare(t).check_shares_vec(vecs, xs, n, culprit=True, bad=counts)
    return counts.tolist(), marks.cpu().tolist()


def records_route(wires, xs, n, t):
    """check_records_vec with both flags deferred: ([inconsistent, located], culprit bytes, record counts)."""
    counts, rec = zeros2(), zeros2()
    none, marks = shamir.SecretShare(t).check_records_vec(wires, xs, n, culprit=True, bad=counts, bad_records=rec)
    assert none is None and marks.dtype == torch.uint8
    return counts.tolist(), marks.cpu().tolist(), rec.tolist()


# ---------------------------------------------------------------- 1. the definition
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
@pytest.mark.parametrize("t, xs", cases.CASES)
def test_counts_and_culprits_match_the_definition(t, xs, n):
    rows, verdicts = case_rows(t, xs)
    want = [verdicts[e % len(rows)] for e in range(n)]
    n_bad = sum(w != cases.CONSISTENT for w in want)
    n_found = sum(w < cases.UNEXPLAINED for w in want)
    wires = [share_wire(x, [rows[e % len(rows)][i] for e in range(n)]) for i, x in enumerate(xs)]
    ss = shamir.SecretShare(t)

    # the method: the read-back forms, xs given and read from the wires
    assert ss.check_records_vec(wires, xs, n) == n_bad
    count, marks = ss.check_records_vec(wires, None, n, culprit=True)
    assert count == n_bad and marks.dtype == torch.uint8 and marks.cpu().tolist() == want
    assert records_route(wires, xs, n, t) == ([n_bad, n_found], want, [0, 0])
    assert decode_route(wires, xs, n, t) == ([n_bad, n_found], want)

    # the entry point: counts are added to across two calls, the bytes around culprit stay untouched
    plan = _native.check_plan(xs, t)
    desc = [(p.data_ptr(), p.numel(), o.data_ptr()) for p, o in wires]
    counts = torch.tensor([5, 7], dtype=torch.int32, device=dev())
    rec = torch.tensor([3, 9], dtype=torch.int32, device=dev())
    buf = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device=dev())
    for _ in range(2):
        _native.check_records(desc, xs, plan, counts, rec, buf[GUARD:GUARD + n], n)
    assert counts.tolist() == [5 + 2 * n_bad, 7 + 2 * n_found] and rec.tolist() == [3, 9]
    host = buf.cpu().numpy()
    assert np.all(host[:GUARD] == 0xA5) and np.all(host[GUARD + n:] == 0xA5)
    assert host[GUARD:GUARD + n].tolist() == want

    # the deferred form under one capture, replayed: no synchronisation, counts added on the device
    bad, rec = zeros2(), zeros2()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        none, g_marks = ss.check_records_vec(wires, xs, n, culprit=True, bad=bad, bad_records=rec)
    assert none is None
    for replay in (1, 2, 3):
        g_marks.fill_(0)
        graph.replay()
        assert bad.tolist() == [replay * n_bad, replay * n_found] and rec.tolist() == [0, 0]
        assert g_marks.cpu().tolist() == want


# ---------------------------------------------------------------- 2. wires that differ
def test_wires_differ_in_header_alignment_and_path():
    """x headers of 1, 3 and 7 bytes (the 3- and 7-byte ones are not their
    wires' abscissas — no plan fits abscissas that wide — so every record of
    wires 1 and 2 is also a wrong-x record, counted and used); `packed` at 0, 4
    and 12 bytes from a 16-byte boundary (both staging paths in one launch);
    wire 3's records carry 30 leading zero bytes, so its waves take the
    byte-serial path while the others stay in LDS; wire 4 is a misaligned view
    (copied once)."""
    t, xs, n = 3, XS5, 700
    rows, verdicts = case_rows(t, xs)
    want = [verdicts[e % len(rows)] for e in range(n)]
    col = [[rows[e % len(rows)][i] for e in range(n)] for i in range(5)]
    padded, o3 = raw_wire([bytes([1, 4]) + bytes(30) + y.to_bytes(66, "big") for y in col[3]])
    wires = [share_wire(1, col[0]), share_wire(0x12345, col[1], 4), share_wire(0x01020304050607, col[2], 12), padded,
             share_wire(5, col[4], 3)]
    assert [p.data_ptr() % 16 for p, _ in wires] == [0, 4, 12, 0, 3]
    assert all(we.decode_window(o3, e0, n, 16) > we.DEC_WINDOW_LIMIT for e0 in range(0, n, 64))
    for p, o in wires[:3] + wires[4:]:
        al = 16 if p.data_ptr() % 16 == 0 else 4
        assert all(we.decode_window(o.cpu().numpy(), e0, n, al) <= we.DEC_WINDOW_LIMIT for e0 in range(0, n, 64))
    counts, marks, rec = records_route(wires, xs, n, t)
    assert (counts, marks) == decode_route(wires, xs, n, t)
    assert marks == want and rec == [0, 2 * n]


# ---------------------------------------------------------------- 3. bad and wrong-x records
BAD = {
    "xlen9": lambda x: bytes([9]) + bytes(range(1, 10)) + b"\x07",
    "xlen-past-record": lambda x: bytes([4, 1, 2]),
    "empty": lambda x: b"",
    "y69": lambda x: bytes([1, x]) + b"\x01" + bytes(68),
}


@pytest.mark.parametrize("kind", sorted(BAD) + ["decreasing", "past-in-bytes"])
def test_bad_and_wrong_x_records_in_one_wire(kind):
    """Wire 1 of five: one bad record at lane 17 of a full wave and one in the
    last, partial wave (counted, y = 0: their elements are flagged with wire 1
    as the culprit), and one record with another x (counted, its y used: its
    element stays consistent).  Every element is a genuine sharing."""
    t, xs, n = 3, XS5, 64 * 3 + 20
    at, other_x = (64 + 17, 64 * 3 + 9), 100
    rows, _ = case_rows(t, xs)
    good = rows[5:8]  # the three consistent rows: none has y = 0 in wire 1
    col = [[good[e % 3][i] for e in range(n)] for i in range(5)]
    recs = [shamir_mod._share_to_bytes((2, y)) for y in col[1]]
    recs[other_x] = shamir_mod._share_to_bytes((9, col[1][other_x]))
    if kind in BAD:
        for e in at:
            recs[e] = BAD[kind](2)
        w1 = raw_wire(recs)[0]
    else:
        p, o = we.pack_records(recs)
        if kind == "decreasing":
            for e in at:
                o[e + 1] = o[e] - 1  # record e ends before it starts; record e + 1 then starts before record e
        else:
            o[n] = p.size + 5  # the last record runs past the wire
            o[at[0] + 1] = p.size + 1000  # and one of a full wave (its wave then starts a record past the end too)
        w1 = (up(p), up(o))
    wires = [share_wire(1, col[0]), w1] + [share_wire(x, col[x - 1]) for x in (3, 4, 5)]
    ss = shamir.SecretShare(t)
    want_rec = zeros2()
    ss.resolve_records_vec(wires, xs, n, bad=want_rec)  # whatever it counts for these offsets, the check counts the same
    want_rec = want_rec.tolist()
    assert want_rec[0] >= 2 and (kind not in BAD or want_rec == [2, 1])
    counts, marks, rec = records_route(wires, xs, n, t)
    assert (counts, marks) == decode_route(wires, xs, n, t) and rec == want_rec
    assert all(marks[e] == 1 for e in (at if kind != "past-in-bytes" else (at[0], n - 1)))
    if kind in BAD:
        assert counts == [2, 2] and marks[other_x] == cases.CONSISTENT
    with pytest.raises(ValueError, match=f"^check_records_vec: {want_rec[0]} records with x > 8 bytes or y > 68 bytes, "
                                         f"{want_rec[1]} records whose x is not their wire's abscissa$"):
        ss.check_records_vec(wires, xs, n)
    flag = zeros2()
    ss.check_records_vec(wires, xs, n, bad_records=flag)  # deferred: does not raise
    ss.check_records_vec(wires, xs, n, bad_records=flag)  # and adds
    assert flag.tolist() == [2 * c for c in want_rec]
    with pytest.raises(ValueError, match=f"^check_records_vec: {2 * want_rec[0]} records with"):
        codec.check_bad_records(flag, "check_records_vec")


# ---------------------------------------------------------------- 4. values
def test_edge_values_in_the_wires():
    """y = 0 (empty y), p, p + 9, 2^521, a 68-byte y and p - 1: as constant
    polynomials (consistent after reduction), and with wire 2 carrying another
    of them (consistent only where the two are congruent)."""
    t, xs = 3, XS5
    edge = [0, P, P + 9, 1 << 521, (1 << 544) - 1, P - 1]
    n = 2 * len(edge) ** 2  # every pair, across a wave edge
    ys = [[edge[(e // 6) % 6] if i == 2 else edge[e % 6] for i in range(5)] for e in range(n)]
    want = [cases.verdict(xs, [y % P for y in row], t) for row in ys]
    assert all((w == cases.CONSISTENT) == ((row[2] - row[0]) % P == 0) for w, row in zip(want, ys))
    assert want.count(2) == n - want.count(cases.CONSISTENT) > 0
    wires = [share_wire(x, [row[i] for row in ys]) for i, x in enumerate(xs)]
    counts, marks, rec = records_route(wires, xs, n, t)
    assert marks == want and counts == [want.count(2)] * 2 and rec == [0, 0]
    assert (counts, marks) == decode_route(wires, xs, n, t)
