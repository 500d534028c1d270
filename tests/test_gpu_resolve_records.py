"""resolve_records_vec / dn_m521_reconstruct_records on the GPU: secrets
straight from wire records, against the reference's own records and secrets
(tests/golden), Python integers, and the existing two-step route on the same
inputs — decode_share_vec on every wire, then resolve_shares_vec.  Every
comparison is bit for bit.

The grid is one workgroup per 256 elements (csrc/recon_records.hip: no cap, no
grid stride), so there is no second-unit case to test.
"""
import numpy as np
import pytest
import torch

import field_edges as fe
import wire_edges as we
from delta_node.crypto import shamir
from delta_node.crypto.shamir import _native, codec, field
from delta_node.crypto.shamir import shamir as shamir_mod
from golden.fixtures import load_json, load_npz, manifest, unpack_share_bytes

pytestmark = pytest.mark.gpu

P = we.P
CANARY = 0xC3
I64_CANARY = -0x0123456789ABCDEF
GUARD = 64  # canary entries / bytes on both sides of an output


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
    assert a.dtype != np.uint8 or out.data_ptr() % 16 == shift
    return out


def wire(x: int, vals, shift: int = 0):
    """(packed, offsets) device pair of the records (x, y_e), and the host offsets."""
    p, o = we.build_records(x, we.ints_to_limbs(vals) if not isinstance(vals, np.ndarray) else vals)
    return (up(p, shift), up(o)), o


def raw_wire(recs, shift: int = 0, first_offset: int = 0):
    p, o = we.pack_records(recs, first_offset)
    return (up(p, shift), up(o)), o


def two_step(wires, xs, n, t, out):
    """The existing route: (result, overflow count, the k decodes' bad count)."""
    bad = torch.zeros(1, dtype=torch.int32, device=dev())
    vecs = []
    for p, o in wires:
        buf = torch.zeros(field.vec_bytes(n), dtype=torch.uint8, device=dev())
        vecs.append(codec.decode_share_vec(p, o, n, out=buf, bad=bad)[0])
    res, over = shamir.SecretShare(t).resolve_shares_vec(vecs, xs, n, out=out, return_overflow=True)
    return res, int(over.item()), int(bad.item())


def direct(wires, xs, n, t, out):
    """resolve_records_vec with a deferred flag: (result, overflow count, [bad, wrong x])."""
    bad = torch.zeros(2, dtype=torch.int32, device=dev())
    res, over = shamir.SecretShare(t).resolve_records_vec(wires, xs, n, out=out, return_overflow=True, bad=bad)
    return res, int(over.item()), bad.tolist()


def field_ints(vec, n):
    return we.limbs_to_ints(field.vec_to_limbs(vec.cpu().numpy(), n))


def same_as_two_step(wires, xs, n, t=2, want_bad=0, want_mis=0):
    for out in ("int64", "field"):
        want, wover, wbad = two_step(wires, xs, n, t, out)
        got, gover, (gbad, gmis) = direct(wires, xs, n, t, out)
        assert wbad == want_bad and (gbad, gmis) == (want_bad, want_mis), (xs, n, out)
        assert gover == wover, (xs, n, out)
        if out == "int64":
            assert torch.equal(got, want), (xs, n, out)
        else:  # lanes past n of the last tile are written by neither route
            assert field_ints(got, n) == field_ints(want, n), (xs, n, out)
    return got


# ---------------------------------------------------------------- 1. the reference's own records
def golden_wires(z, n_shares, xs, N):
    ws = []
    flat, offs = z["share_bytes"], z["share_offsets"]  # (an npz member is read again at every access)
    for x in xs:
        recs = [unpack_share_bytes(flat, offs, e * n_shares + x - 1) for e in range(N)]
        ws.append(raw_wire(recs)[0])
    return ws


@pytest.mark.parametrize("key,xs", [("f1", [1, 3, 5]), ("f1", [2, 4, 5]), ("f1", [1, 2, 3, 4, 5]),
                                    ("f2", [1, 2, 4, 6, 9]), ("f2", [1, 2, 3, 4, 5, 6, 7, 8, 9])])
def test_reference_records_give_the_reference_secrets(key, xs):
    cfg = manifest()[key]
    z = load_npz(cfg["file"])
    N, n, t = cfg["N"], cfg["n"], cfg["t"]
    wires = golden_wires(z, n, xs, N)
    want = torch.from_numpy(z["secrets"][:N]).to(dev())
    ss = shamir.SecretShare(t)
    got, over = ss.resolve_records_vec(wires, xs, N, return_overflow=True)
    assert torch.equal(got, want) and int(over.item()) == 0
    fe_out = ss.resolve_records_vec(wires, xs, N, out="field")
    assert field_ints(fe_out, N) == [int(v) & ((1 << 64) - 1) for v in z["secrets"][:N]]
    if key == "f1" and xs == [1, 3, 5]:  # xs=None: the abscissas come from the data
        assert torch.equal(ss.resolve_records_vec(wires, None, N), want)
        assert torch.equal(ss.resolve_records_vec(list(reversed(wires)), None, N), want)


def test_inconsistent_shares_equal_the_fixture_and_two_step():
    done = 0
    for group in load_json("f4_recon.json"):
        xs, rows = group["xs"], group["rows"]
        if len(xs) < 2:
            continue
        assert all("out" in r for r in rows)
        n, k = len(rows), len(xs)
        wires = [raw_wire([shamir_mod._share_to_bytes((x, int(r["ys"][i], 16))) for r in rows])[0]
                 for i, x in enumerate(xs)]
        want = [int(r["out"], 16) if r["out"] else 0 for r in rows]
        got, over, bad = direct(wires, xs, n, k, "field")
        assert field_ints(got, n) == want, xs
        assert over == sum(v >= (1 << 64) for v in want) and bad == [0, 0], xs
        same_as_two_step(wires, xs, n, t=k)
        done += 1
    assert done >= 10


# ---------------------------------------------------------------- 2. shapes
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_shapes_behind_canaries(n):
    """Ragged y lengths; the entry point writes n int64 / the tiles of n field
    elements and nothing around them."""
    xs = [1, 3, 5]
    wires = [wire(x, we.ragged_limbs(n, 10 * n + i))[0] for i, x in enumerate(xs)]
    same_as_two_step(wires, xs, n)
    w = _native.lagrange(xs, 2)
    desc = [(p.data_ptr(), p.numel(), o.data_ptr()) for p, o in wires]
    want_i, _, _ = two_step(wires, xs, n, 2, "int64")
    want_f, wover, _ = two_step(wires, xs, n, 2, "field")
    vb = field.vec_bytes(n)
    big_i = torch.full((n + 2 * GUARD,), I64_CANARY, dtype=torch.int64, device=dev())
    big_f = torch.full((vb + 2 * GUARD,), CANARY, dtype=torch.uint8, device=dev())
    out_f = big_f[GUARD:GUARD + vb]
    keep = out_f.clone()
    bad = torch.zeros(2, dtype=torch.int32, device=dev())
    over = torch.zeros(1, dtype=torch.int32, device=dev())
    _native.reconstruct_records(desc, xs, w, bad, out_fe=out_f, out_u64=big_i[GUARD:GUARD + n], overflow=over, n=n)
    assert torch.equal(big_i[GUARD:GUARD + n], want_i) and int(over.item()) == wover and bad.tolist() == [0, 0]
    assert bool((big_i[:GUARD] == I64_CANARY).all()) and bool((big_i[GUARD + n:] == I64_CANARY).all())
    assert bool((big_f[:GUARD] == CANARY).all()) and bool((big_f[GUARD + vb:] == CANARY).all())
    assert field_ints(out_f, n) == field_ints(want_f, n)
    # every byte of the tiled output that belongs to no element keeps its canary
    pos, _ = we.scatter_tiles(np.arange(n), np.zeros((n, we.LIMBS), dtype=np.uint32))
    mask = torch.ones(vb, dtype=torch.bool, device=dev())
    mask[up(pos)] = False
    assert torch.equal(out_f[mask], keep[mask])


# ---------------------------------------------------------------- 3. weights
B33 = 1 << 33
B40 = 1 << 40
# xs -> (a_limbs, has_inv, shift) of dn_m521_lagrange's descriptor
FORMS = [
    ([1, 3], (1, 0, 1)), ([1, 4], (1, 2, 0)), ([1040758, 758791], (1, 1, 0)),
    ([B33, B33 + 1], (2, 0, 0)), ([B33, B33 + 3], (2, 2, 0)),
    ([1, 3, 5], (1, 0, 3)), ([2, 4, 5], (1, 2, 0)), ([98, 19, 222], (1, 1, 1)),
    ([35016, 60626, 7492], (2, 1, 0)), ([88159051, 658814259, 702745590], (17, 0, 0)),
    ([1, 2, 3, 6], (1, 2, 1)), ([217, 19, 197, 46], (1, 1, 2)),
    ([1, 3, 5, 7, 9], (1, 0, 7)), ([162, 232, 144, 246, 154], (1, 1, 0)),
    ([1, 2, 3, 4, 5, 6, 8], (1, 2, 0)), ([136, 9, 74, 114, 243, 52, 54], (2, 1, 0)),
    ([128, 224, 164, 228, 136, 238, 174, 177, 179, 147, 115, 151, 24, 88, 157, 159], (17, 0, 0)),
]
N_W = 321  # five full waves and one lane: two workgroups


@pytest.mark.parametrize("xs,form", FORMS, ids=[f"k{len(x)}-A{f[0]}-inv{f[1]}-s{f[2]}" for x, f in FORMS])
def test_weight_forms_equal_two_step(xs, form):
    w = _native.lagrange(xs, 2)
    assert (w.a_limbs, w.has_inv, w.shift) == form  # the coverage is stated, not assumed
    assert w.neg != 0 or w.a_limbs == 17  # small-rational weights carry signs: a negated wire in each such case
    wires = [wire(x, we.ragged_limbs(N_W, 77 * len(xs) + i))[0] for i, x in enumerate(xs)]
    same_as_two_step(wires, xs, N_W)


def test_the_forms_cover_every_kernel_family():
    got = {(f[0], f[1]) for _, f in FORMS}
    assert got == {(1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2), (17, 0)}
    assert {len(x) for x, _ in FORMS} >= {2, 3, 4, 5, 7, 16}
    assert any(f[2] for _, f in FORMS)


def test_large_abscissas_and_k16():
    """Abscissas >= 2^40 (six-byte x headers, wider weights), k = 2 and k = 16."""
    for xs in ([B40 + 1, B40 + 4], [B40, 3, B40 + 5], list(range(B40, B40 + 16)), list(range(1, 17))):
        assert len(we.x_bytes(max(xs))) >= 6 or max(xs) == 16
        wires = [wire(x, we.ragged_limbs(130, 5 * len(xs) + i))[0] for i, x in enumerate(xs)]
        same_as_two_step(wires, xs, 130)


@pytest.mark.parametrize("has_inv,d", [(1, 0x1234567), (2, 12345)])
def test_full_width_weights_with_a_divisor(has_inv, d):
    """(17, 1) and (17, 2): forms the host never produces but the entry point
    dispatches; against dn_m521_reconstruct on the decoded vectors."""
    k, n = 3, 200
    a = fe.recon_weights(17, k, 3)[:k]
    w = fe.make_desc(a, 0b101, 17, shift=5, has_inv=has_inv, d=d)
    xs = [4, 9, 11]
    wires = [wire(x, we.ragged_limbs(n, 900 + i))[0] for i, x in enumerate(xs)]
    vecs = [codec.decode_share_vec(p, o, n)[0] for p, o in wires]
    want = torch.zeros(field.vec_bytes(n), dtype=torch.uint8, device=dev())
    got = torch.zeros_like(want)
    wo, go = (torch.zeros(1, dtype=torch.int32, device=dev()) for _ in range(2))
    _native.reconstruct(vecs, w, out_fe=want, overflow=wo, n=n)
    bad = torch.zeros(2, dtype=torch.int32, device=dev())
    _native.reconstruct_records([(p.data_ptr(), p.numel(), o.data_ptr()) for p, o in wires], xs, w, bad, out_fe=got,
                                overflow=go, n=n)
    assert torch.equal(got, want) and int(go.item()) == int(wo.item()) and bad.tolist() == [0, 0]


# ---------------------------------------------------------------- 4. wires that differ
def test_header_lengths_and_alignments_differ_per_wire():
    """x headers of 1, 3 and 7 bytes: every wire's windows start at other byte
    phases; wire 0 16-byte aligned, wire 1 shifted by 4, wire 2 by 12: both
    staging paths in one launch."""
    xs = [5, 0x12345, 0x01020304050607]
    n = 700
    wires = [wire(x, we.ragged_limbs(n, 40 + i), shift=s)[0] for i, (x, s) in enumerate(zip(xs, (0, 4, 12)))]
    assert [p.data_ptr() % 16 for p, _ in wires] == [0, 4, 12]
    same_as_two_step(wires, xs, n)


def test_a_misaligned_view_is_cloned_once():
    xs = [1, 2]
    n = 100
    wires = [wire(x, we.ragged_limbs(n, 60 + i), shift=s)[0] for i, (x, s) in enumerate(zip(xs, (0, 3)))]
    assert wires[1][0].data_ptr() % 4 == 3
    same_as_two_step(wires, xs, n)


def test_one_wire_takes_the_byte_serial_path():
    """Wire 1's records carry 30 leading zero bytes before y, so its full
    waves' windows exceed the LDS slice while wires 0 and 2 of the same waves
    stay inside it."""
    xs = [1, 3, 5]
    n = 200
    limbs = [we.ragged_limbs(n, 80 + i) for i in range(3)]
    limbs[1][:128, 16] |= 0x100  # 66-byte values in the two full waves
    vals1 = we.limbs_to_ints(limbs[1])
    recs = [bytes([1, 3]) + bytes(30) + v.to_bytes((v.bit_length() + 7) // 8, "big") for v in vals1]
    (w1, o1) = raw_wire(recs)
    (w0, o0), (w2, o2) = wire(1, limbs[0]), wire(5, limbs[2])
    assert all(we.decode_window(o1, e0, n, 16) > we.DEC_WINDOW_LIMIT for e0 in (0, 64))
    assert we.decode_window(o1, 192, n, 16) <= we.DEC_WINDOW_LIMIT  # the last, partial wave: LDS path
    assert all(we.decode_window(o, e0, n, 16) <= we.DEC_WINDOW_LIMIT for o in (o0, o2) for e0 in (0, 64, 128, 192))
    same_as_two_step([w0, w1, w2], xs, n)


# ---------------------------------------------------------------- 5. values
def test_edge_values_in_every_wire():
    """y = 0 (empty y), p, p + 9, 2^521, a 68-byte y, P - 1, in every wire."""
    xs = [1, 3, 5]
    edge = [0, P, P + 9, 1 << 521, (1 << 544) - 1, P - 1, 1, (1 << 64) - 1, 1 << 64]
    n = len(edge) ** 3  # every triple
    assert len(edge) == 9
    vals = [[edge[(e // (9 ** i)) % 9] for e in range(n)] for i in range(3)]
    wires = [raw_wire([shamir_mod._share_to_bytes((x, y)) for y in v])[0] for x, v in zip(xs, vals)]
    got = same_as_two_step(wires, xs, n, t=3)
    lam = shamir_mod._lagrange_generic(xs, P)
    want = [sum(l * v[e] for l, v in zip(lam, vals)) % P for e in range(n)]
    assert field_ints(got, n) == want
    same = [[y] * 70 for y in edge]  # the same value in every wire: the constant polynomial
    for y, col in zip(edge, same):
        wires = [raw_wire([shamir_mod._share_to_bytes((x, v)) for v in col])[0] for x in xs]
        res = shamir.SecretShare(3).resolve_records_vec(wires, xs, 70, out="field")
        assert field_ints(res, 70) == [y % P] * 70


# ---------------------------------------------------------------- 6. bad records
def y_bytes(v):
    return v.to_bytes((v.bit_length() + 7) // 8, "big")


BAD = {
    "xlen9": lambda x: bytes([9]) + bytes(range(1, 10)) + b"\x07",
    "xlen-past-record": lambda x: bytes([4, 1, 2]),
    "empty": lambda x: b"",
    "y69": lambda x: bytes([1, x]) + b"\x01" + bytes(68),
}


@pytest.mark.parametrize("kind", sorted(BAD) + ["decreasing", "past-in-bytes"])
def test_bad_records_in_one_wire(kind):
    """One bad record at lane 17 of a full wave and one in the last, partial
    wave, in wire 1 only: counted, y = 0, as the two-step route has it."""
    xs = [1, 3, 5]
    n = 64 * 3 + 20
    at = (64 + 17, 64 * 3 + 9)
    vals = [we.limbs_to_ints(we.ragged_limbs(n, 300 + i)) for i in range(3)]
    recs = [bytes([1, 3]) + y_bytes(v) for v in vals[1]]
    want_bad = 2
    if kind in BAD:
        for e in at:
            recs[e] = BAD[kind](3)
        w1 = raw_wire(recs)[0]
    else:
        p, o = we.pack_records(recs)
        if kind == "decreasing":
            for e in at:
                o[e + 1] = o[e] - 1  # record e ends before it starts; record e + 1 then starts before record e
            want_bad = None
        else:
            o[n] = p.size + 5  # the last record runs past the wire
            o[at[0] + 1] = p.size + 1000  # and one of a full wave (its wave then starts a record past the end too)
            want_bad = None
        w1 = (up(p), up(o))
    wires = [wire(1, we.ints_to_limbs(vals[0]))[0], w1, wire(5, we.ints_to_limbs(vals[2]))[0]]
    if want_bad is None:  # whatever the decoder counts for these offsets, the new call counts the same
        want_bad = two_step(wires, xs, n, 2, "int64")[2]
        assert want_bad >= 2
    same_as_two_step(wires, xs, n, want_bad=want_bad)
    ss = shamir.SecretShare(2)
    with pytest.raises(ValueError,
                       match=f"resolve_records_vec: {want_bad} records with x > 8 bytes or y > 68 bytes, 0 records"):
        ss.resolve_records_vec(wires, xs, n)
    flag = torch.zeros(2, dtype=torch.int32, device=dev())
    ss.resolve_records_vec(wires, xs, n, bad=flag)  # deferred: does not raise
    ss.resolve_records_vec(wires, xs, n, bad=flag)  # and adds
    assert flag.tolist() == [2 * want_bad, 0]
    with pytest.raises(ValueError, match=f"{2 * want_bad} records with"):
        codec.check_bad_records(flag)
    if kind in BAD:  # the good elements are the interpolant of the three wires
        got = ss.resolve_records_vec(wires, xs, n, out="field", bad=flag)
        lam = shamir_mod._lagrange_generic(xs, P)
        ints = field_ints(got, n)
        for e in (0, at[0] - 1, at[0], at[0] + 1, at[1], n - 1):
            ys = [vals[0][e], 0 if e in at else vals[1][e], vals[2][e]]
            assert ints[e] == sum(l * y for l, y in zip(lam, ys)) % P, e


# ---------------------------------------------------------------- 7. x mismatch
def test_one_wrong_x_is_counted_and_its_y_used():
    xs = [1, 3, 5]
    n = 150
    vals = [we.limbs_to_ints(we.ragged_limbs(n, 400 + i)) for i in range(3)]
    recs = [bytes([1, 3]) + y_bytes(v) for v in vals[1]]
    recs[77] = bytes([1, 4]) + y_bytes(vals[1][77])
    wires = [wire(1, we.ints_to_limbs(vals[0]))[0], raw_wire(recs)[0], wire(5, we.ints_to_limbs(vals[2]))[0]]
    got = same_as_two_step(wires, xs, n, want_mis=1)
    lam = shamir_mod._lagrange_generic(xs, P)
    assert field_ints(got, n)[77] == sum(l * v[77] for l, v in zip(lam, vals)) % P
    with pytest.raises(ValueError, match="0 records with x > 8 bytes or y > 68 bytes, 1 records whose x is not"):
        shamir.SecretShare(2).resolve_records_vec(wires, xs, n)
    # a wrong abscissa for a whole wire: every record of it
    flag = torch.zeros(2, dtype=torch.int32, device=dev())
    shamir.SecretShare(2).resolve_records_vec(wires, [1, 7, 5], n, bad=flag)
    assert flag.tolist() == [0, n]


def test_xs_none_checks_what_it_read():
    n = 10
    wires = [wire(x, we.ragged_limbs(n, 500 + x))[0] for x in (2, 2, 6)]
    with pytest.raises(ValueError, match="^shares must be distinct$"):
        shamir.SecretShare(2).resolve_records_vec(wires, None, n)
    with pytest.raises(ValueError, match="^need at least 4 shares$"):
        shamir.SecretShare(4).resolve_records_vec(wires, None, n)
    broken = raw_wire([bytes([9]) + bytes(12)] * n)[0]
    with pytest.raises(ValueError, match="the first record of wire 1 has no readable x"):
        shamir.SecretShare(2).resolve_records_vec([wires[0], broken], None, n)


# ---------------------------------------------------------------- 8. fallback
def test_k17_takes_the_decode_path(monkeypatch):
    """k = 17: decode_share_vec per wire, then the grouped full-width
    interpolation — the same results and counts."""
    n = 130

    def native(*a, **k):
        raise AssertionError("the native form was used where it does not apply")

    monkeypatch.setattr(_native, "reconstruct_records", native)
    xs = list(range(1, 18))
    wires = [wire(x, we.ragged_limbs(n, 600 + i))[0] for i, x in enumerate(xs)]
    same_as_two_step(wires, xs, n)
    # one wrong-x and one unrepresentable record through the same path
    recs = [bytes([1, 2]) + y_bytes(v) for v in we.limbs_to_ints(we.ragged_limbs(n, 700))]
    recs[5] = bytes([1, 9]) + recs[5][2:]
    recs[70] = bytes([9]) + bytes(12)
    wires[1] = raw_wire(recs)[0]
    want = two_step(wires, xs, n, 2, "int64")
    got = direct(wires, xs, n, 2, "int64")
    assert torch.equal(got[0], want[0]) and got[1] == want[1] and want[2] == 1
    assert got[2] == [1, 2]  # this path cannot tell an unrepresentable record's x from a wrong one
    with pytest.raises(ValueError, match="1 records with x > 8 bytes or y > 68 bytes, 2 records whose x"):
        shamir.SecretShare(2).resolve_records_vec(wires, xs, n)
