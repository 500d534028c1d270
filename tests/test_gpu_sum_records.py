"""sum_records_vec / dn_m521_sum_records on the GPU: the party-side sum straight
from wire records, against the reference's own records (tests/golden), Python
integers, and the existing two-step route on the same inputs — decode_share_vec
on every wire into pre-zeroed buffers, then sum_shares_vec.  Every comparison
is bit for bit and covers all vec_bytes(n) bytes of the output, the zero
padding of a partial last tile included; every output is a view with canary
bytes on both sides.

The grid is one workgroup per 256 elements (csrc/sum_records.hip: no cap, no
grid stride), so there is no second-unit case to test.
"""
import numpy as np
import pytest
import torch

import wire_edges as we
from delta_node.crypto import shamir
from delta_node.crypto.shamir import _native, codec, field
from delta_node.crypto.shamir import shamir as shamir_mod
from golden.fixtures import load_npz, manifest, unpack_share_bytes
from test_sum_records_host import group

pytestmark = pytest.mark.gpu

P = we.P
G = group()
CANARY = 0xC3
GUARD = 64  # canary bytes on both sides of an output
SS = shamir.SecretShare(2)  # the method uses neither the threshold nor the generator


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


def raw_wire(recs, shift: int = 0):
    p, o = we.pack_records(recs)
    return (up(p, shift), up(o)), o


def y_bytes(v):
    return v.to_bytes((v.bit_length() + 7) // 8, "big")


def rec(x: int, y: int, pad: int = 0) -> bytes:
    """The record of (x, y) with `pad` zero bytes in front of y."""
    xb = we.x_bytes(x)
    return bytes([len(xb)]) + xb + bytes(pad) + y_bytes(y)


def field_ints(vec, n):
    return we.limbs_to_ints(field.vec_to_limbs(vec.cpu().numpy(), n))


def tiled(vals):
    """The tiled device vector of Python ints below 2^521 (zero padding)."""
    return up(we.tiles_of(we.ints_to_limbs(vals)))


def guarded(n):
    """(buffer, its out view) — everything CANARY."""
    vb = field.vec_bytes(n)
    big = torch.full((vb + 2 * GUARD,), CANARY, dtype=torch.uint8, device=dev())
    return big, big[GUARD:GUARD + vb]


def guards_intact(big):
    return bool((big[:GUARD] == CANARY).all()) and bool((big[big.numel() - GUARD:] == CANARY).all())


def decode(w, n):
    """decode_share_vec into a pre-zeroed buffer: (vector, xs, bad count)."""
    bad = torch.zeros(1, dtype=torch.int32, device=dev())
    buf = torch.zeros(field.vec_bytes(n), dtype=torch.uint8, device=dev())
    v, xs = codec.decode_share_vec(w[0], w[1], n, out=buf, bad=bad)
    return v, xs, int(bad.item())


def two_step(wires, n, signs=None, acc=None, decoded=None):
    """The existing route: (sum vector, the m decodes' bad count)."""
    dec = decoded if decoded is not None else [decode(w, n) for w in wires]
    vecs = [d[0] for d in dec]
    sg = list(signs) if signs is not None else [1] * len(vecs)
    if acc is not None:
        vecs, sg = [acc] + vecs, [1] + sg
    return SS.sum_shares_vec(vecs, signs=sg), sum(d[2] for d in dec)


def direct(wires, x, n, signs=None, acc=None, in_place=False):
    """sum_records_vec with a deferred flag into a canary-guarded out (pre-filled
    with canary bytes, or with acc's bytes where acc is out): (out, [bad, wrong x])."""
    big, out = guarded(n)
    if in_place:
        out.copy_(acc)
        acc = out
    bad = torch.zeros(2, dtype=torch.int32, device=dev())
    got = SS.sum_records_vec(wires, x, n, signs=signs, acc=acc, out=out, bad=bad)
    assert got is out and guards_intact(big), (x, n)
    return out, bad.tolist()


def same_as_two_step(wires, x, n, signs=None, acc=None, want_bad=0, want_mis=0, decoded=None):
    want, wbad = two_step(wires, n, signs, acc, decoded)
    got, gbad = direct(wires, x, n, signs, acc)
    assert wbad == want_bad and gbad == [want_bad, want_mis], (x, n, wbad, gbad)
    assert torch.equal(got, want), (x, n)
    return got


def expect(vals, signs=None, acc=None):
    """(acc_e + sum_i +-y_{i,e}) mod p from Python integers."""
    sg = signs if signs is not None else [1] * len(vals)
    n = len(vals[0])
    return [((acc[e] if acc is not None else 0) + sum(s * v[e] for s, v in zip(sg, vals))) % P for e in range(n)]


# ---------------------------------------------------------------- 1. the reference's own records
def test_reference_records_sum_to_the_sum_of_the_secrets():
    """Fixture f1 (N = 1024, 3-of-5): four 256-element slices as four members.
    Party x's sum of the members' share-x records is sum y mod p, and any three
    parties' sums reconstruct the sum of the four slices of `secrets`: the
    wrapping int64 sum where every member is added; with member 3 subtracted
    the field value (sum_j +-u_j) mod p over the secrets' uint64 views (a
    negative total is p - |total|, whose low 64 bits are not the wrapping sum)."""
    cfg = manifest()["f1"]
    z = load_npz(cfg["file"])
    N, n_sh, t = cfg["N"], cfg["n"], cfg["t"]
    assert (N, n_sh, t) == (1024, 5, 3)
    n, members = 256, 4
    flat, offs = z["share_bytes"], z["share_offsets"]
    sec = [int(v) & ((1 << 64) - 1) for v in z["secrets"][:N]]
    ss = shamir.SecretShare(t)
    for signs in (None, [1, 1, 1, -1]):
        sums = {}
        for x in range(1, n_sh + 1):
            wires, ys = [], []
            for j in range(members):
                recs = [unpack_share_bytes(flat, offs, (n * j + e) * n_sh + x - 1) for e in range(n)]
                assert all(r[0] == 1 and r[1] == x for r in recs)
                ys.append([int.from_bytes(r[2:], "big") for r in recs])
                wires.append(raw_wire(recs)[0])
            got, bad = direct(wires, x, n, signs)
            assert bad == [0, 0] and field_ints(got, n) == expect(ys, signs), x
            sums[x] = got
        sg = signs or [1] * members
        total = [sum(s * sec[n * j + e] for j, s in enumerate(sg)) for e in range(n)]
        for xs in ([1, 3, 5], [2, 4, 5]):
            res = ss.resolve_shares_vec([sums[x] for x in xs], xs, n, out="field")
            assert field_ints(res, n) == [v % P for v in total], (xs, signs)
            if signs is None:
                want = torch.from_numpy(z["secrets"][:N].reshape(members, n)).sum(0).to(dev())  # wraps
                assert torch.equal(ss.resolve_shares_vec([sums[x] for x in xs], xs, n), want), xs
            else:  # where the total is not negative its low 64 bits are the wrapping sum here too
                low = ss.resolve_shares_vec([sums[x] for x in xs], xs, n).cpu().tolist()
                plus = [e for e in range(n) if total[e] >= 0]
                assert len(plus) > n // 4 and all((low[e] - total[e]) % (1 << 64) == 0 for e in plus), xs


# ---------------------------------------------------------------- 2. element edges
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
def test_element_edges(n):
    """Wave and tile boundaries; the lanes past n of a partial last tile are
    written as zero over the canary bytes `out` held."""
    x = 3
    vals = [we.limbs_to_ints(we.ragged_limbs(n, 10 * n + i)) for i in range(3)]
    wires = [wire(x, v)[0] for v in vals]
    got = same_as_two_step(wires, x, n, signs=[1, -1, 1])
    assert field_ints(got, n) == expect(vals, [1, -1, 1])
    pos, _ = we.scatter_tiles(np.arange(n), np.zeros((n, we.LIMBS), dtype=np.uint32))
    pad = torch.ones(field.vec_bytes(n), dtype=torch.bool, device=dev())
    pad[up(pos)] = False
    assert not bool(got[pad].any())


def test_padding_lanes_are_zero_whatever_acc_holds_there():
    n = 70  # lanes 70..127 of wave 1, waves 2 and 3 whole
    vals = [we.limbs_to_ints(we.ragged_limbs(n, 31 + i)) for i in range(2)]
    wires = [wire(7, v)[0] for v in vals]
    accv = we.limbs_to_ints(we.ragged_limbs(n, 33))
    clean = tiled(accv)
    dirty = torch.full_like(clean, CANARY)
    pos, val = we.scatter_tiles(np.arange(n), we.ints_to_limbs(accv))
    dirty[up(pos)] = up(val)
    want = tiled(expect(vals, acc=accv))
    for in_place in (False, True):
        got, bad = direct(wires, 7, n, acc=dirty.clone(), in_place=in_place)
        assert bad == [0, 0] and torch.equal(got, want), in_place
    assert torch.equal(two_step(wires, n, acc=clean)[0], want)


def test_no_elements():
    w = [(torch.zeros(0, dtype=torch.uint8, device=dev()), torch.zeros(1, dtype=torch.int64, device=dev()))] * 2
    out = SS.sum_records_vec(w, 1, 0)
    assert out.dtype == torch.uint8 and out.numel() == 0 and out.device == dev()
    flag = torch.zeros(2, dtype=torch.int32, device=dev())
    assert SS.sum_records_vec(w, 1, 0, signs=[1, -1], bad=flag).numel() == 0 and flag.tolist() == [0, 0]


# ---------------------------------------------------------------- 3. wire-count edges
N_M = 65
X_M = 5


@pytest.fixture(scope="module")
def many():
    """2G + 1 wires of 65 elements, their values, signs and decodes — built once, never changed."""
    m = 2 * G + 1
    vals = [we.limbs_to_ints(we.ragged_limbs(N_M, 2000 + i)) for i in range(m)]
    wires = [wire(X_M, v)[0] for v in vals]
    signs = [-1 if i % 3 == 1 else 1 for i in range(m)]
    decoded = [decode(w, N_M) for w in wires]
    accv = we.limbs_to_ints(we.ragged_limbs(N_M, 1999))
    return vals, wires, signs, decoded, accv


@pytest.mark.parametrize("m", [1, 2, G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1])
def test_wire_count_edges(many, m):
    """Group boundaries of the chained launches: plain, with acc, with acc is
    out, and with the wires permuted together with their signs."""
    vals, wires, signs, decoded, accv = many
    vals, wires, signs, decoded = vals[:m], wires[:m], signs[:m], decoded[:m]
    want = tiled(expect(vals, signs))
    assert torch.equal(same_as_two_step(wires, X_M, N_M, signs, decoded=decoded), want)
    acc = tiled(accv)
    want_acc = tiled(expect(vals, signs, accv))
    assert torch.equal(same_as_two_step(wires, X_M, N_M, signs, acc=acc, decoded=decoded), want_acc)
    assert torch.equal(acc, tiled(accv))  # a separate acc is only read
    got, bad = direct(wires, X_M, N_M, signs, acc=acc, in_place=True)
    assert bad == [0, 0] and torch.equal(got, want_acc)
    perm = np.random.default_rng(m).permutation(m).tolist()
    got, bad = direct([wires[i] for i in perm], X_M, N_M, [signs[i] for i in perm])
    assert bad == [0, 0] and torch.equal(got, want)


# ---------------------------------------------------------------- 4. value edges
EDGE = [0, 1, 1 << 64, P - 1, P, P + 1, 1 << 521, (1 << 544) - 1]


def test_value_edges_in_one_wire_set():
    """m = G wires; wire i holds the edge values rotated by i, then the 68-byte
    value behind 1, 2 and 40 extra leading zero bytes."""
    x = 9
    assert y_bytes(EDGE[-1]) == b"\xff" * 68 and rec(x, 0) == bytes([1, x])
    n = len(EDGE) + 3
    vals, wires = [], []
    for i in range(G):
        v = [EDGE[(e + i) % len(EDGE)] for e in range(len(EDGE))]
        recs = [rec(x, y) for y in v] + [rec(x, EDGE[-1] - i, pad) for pad in (1, 2, 40)]
        vals.append([y % P for y in v] + [(EDGE[-1] - i) % P] * 3)
        wires.append(raw_wire(recs)[0])
    signs = [-1 if i % 2 else 1 for i in range(G)]
    for sg in (None, signs):
        got = same_as_two_step(wires, x, n, sg)
        assert field_ints(got, n) == expect(vals, sg)


@pytest.mark.parametrize("y", [P - 1, (1 << 544) - 1], ids=["p-1", "2^544-1"])
def test_every_wire_the_same_extreme(y):
    """The lazy bound (G terms of p - 1 on top of an acc of p - 1) and the
    reduce before the add (G 68-byte values would overflow 17 limbs unreduced),
    with signs all +1 and all -1."""
    x, n = 2, 70
    wires = [raw_wire([rec(x, y)] * n)[0]] * G
    decoded = [decode(wires[0], n)] * G
    vals = [[y % P] * n] * G
    accv = [P - 1] * n
    acc = tiled(accv)
    for sg in ([1] * G, [-1] * G):
        got = same_as_two_step(wires, x, n, sg, decoded=decoded)
        assert field_ints(got, n) == expect(vals, sg)
        got = same_as_two_step(wires, x, n, sg, acc=acc, decoded=decoded)
        assert field_ints(got, n) == expect(vals, sg, accv)


# ---------------------------------------------------------------- 5. abscissa edges
@pytest.mark.parametrize("x", [0, 1, 255, 256, 1 << 32, (1 << 64) - 1])
def test_abscissa_edges(x):
    n = 70
    vals = [we.limbs_to_ints(we.ragged_limbs(n, 50 + i)) for i in range(2)]
    wires = [wire(x, v)[0] for v in vals]
    got = same_as_two_step(wires, x, n)
    assert field_ints(got, n) == expect(vals)
    assert torch.equal(SS.sum_records_vec(wires, None, n), got)  # x=None: read from the agreeing wires
    other = 7 if x != 7 else 8
    _, bad = direct(wires, other, n)
    assert bad == [0, 2 * n]


def test_x_none_on_disagreeing_wires_raises():
    n = 10
    wires = [wire(x, we.ragged_limbs(n, 500 + x))[0] for x in (2, 2, 6)]
    with pytest.raises(ValueError, match="sum_records_vec: the wires' first records carry different abscissas"):
        SS.sum_records_vec(wires, None, n)
    broken = raw_wire([bytes([9]) + bytes(12)] * n)[0]
    with pytest.raises(ValueError, match="sum_records_vec: the first record of wire 1 has no readable x"):
        SS.sum_records_vec([wires[0], broken], None, n)


def test_one_wrong_x_is_counted_and_its_y_used():
    x, n = 3, 150
    vals = [we.limbs_to_ints(we.ragged_limbs(n, 400 + i)) for i in range(3)]
    recs = [rec(x, v) for v in vals[1]]
    recs[77] = rec(4, vals[1][77])
    wires = [wire(x, vals[0])[0], raw_wire(recs)[0], wire(x, vals[2])[0]]
    got = same_as_two_step(wires, x, n, want_mis=1)
    assert field_ints(got, n) == expect(vals)
    with pytest.raises(ValueError, match="^sum_records_vec: 0 records with x > 8 bytes or y > 68 bytes, "
                                         "1 records whose x is not their wire's abscissa$"):
        SS.sum_records_vec(wires, x, n)


# ---------------------------------------------------------------- 6. alignment
def test_alignments_differ_per_wire():
    """packed at 0, 4, 8 and 12 bytes past a 16-byte boundary in one call: the per-wire staging bit."""
    x, n = 0x12345, 300
    vals = [we.limbs_to_ints(we.ragged_limbs(n, 40 + i)) for i in range(4)]
    wires = [wire(x, v, shift=s)[0] for v, s in zip(vals, (0, 4, 8, 12))]
    assert [p.data_ptr() % 16 for p, _ in wires] == [0, 4, 8, 12]
    got = same_as_two_step(wires, x, n, signs=[1, 1, -1, 1])
    assert field_ints(got, n) == expect(vals, [1, 1, -1, 1])


def test_a_misaligned_view_is_cloned_once():
    x, n = 1, 100
    vals = [we.limbs_to_ints(we.ragged_limbs(n, 60 + i)) for i in range(2)]
    wires = [wire(x, v, shift=s)[0] for v, s in zip(vals, (0, 1))]
    assert wires[1][0].data_ptr() % 4 == 1
    got = same_as_two_step(wires, x, n)
    assert field_ints(got, n) == expect(vals)


# ---------------------------------------------------------------- 7. window paths
def test_one_wire_takes_the_byte_serial_path():
    """Wire 1's records carry 30 leading zero bytes before y, so its full
    waves' windows exceed the LDS slice while wires 0 and 2 of the same waves
    stay inside it."""
    x, n = 3, 200
    limbs = [we.ragged_limbs(n, 80 + i) for i in range(3)]
    limbs[1][:128, 16] |= 0x100  # 66-byte values in the two full waves
    vals = [we.limbs_to_ints(l) for l in limbs]
    (w1, o1) = raw_wire([rec(x, v, 30) for v in vals[1]])
    (w0, o0), (w2, o2) = wire(x, limbs[0]), wire(x, limbs[2])
    assert all(we.decode_window(o1, e0, n, 16) > we.DEC_WINDOW_LIMIT for e0 in (0, 64))
    assert we.decode_window(o1, 192, n, 16) <= we.DEC_WINDOW_LIMIT  # the last, partial wave: LDS path
    assert all(we.decode_window(o, e0, n, 16) <= we.DEC_WINDOW_LIMIT for o in (o0, o2) for e0 in (0, 64, 128, 192))
    got = same_as_two_step([w0, w1, w2], x, n, signs=[1, -1, 1])
    assert field_ints(got, n) == expect(vals, [1, -1, 1])


# ---------------------------------------------------------------- 8. records the kernel must bound
BAD = {
    "xlen9": lambda x: bytes([9]) + bytes(range(1, 10)) + b"\x07",
    "y69": lambda x: bytes([1, x]) + b"\x01" + bytes(68),
}


@pytest.mark.parametrize("kind", sorted(BAD) + ["decreasing", "past-in-bytes"])
def test_bad_records_in_one_wire(kind):
    """One bad record at lane 17 of a full wave and one in the last, partial
    wave, in wire 1 only: counted in [0], y = 0 (p under sign -1), the result
    and the count those of the two-step route."""
    x = 3
    n = 64 * 3 + 20
    at = (64 + 17, 64 * 3 + 9)
    vals = [we.limbs_to_ints(we.ragged_limbs(n, 300 + i)) for i in range(3)]
    recs = [rec(x, v) for v in vals[1]]
    if kind in BAD:
        for e in at:
            recs[e] = BAD[kind](x)
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
    wires = [wire(x, vals[0])[0], w1, wire(x, vals[2])[0]]
    want_bad = decode(w1, n)[2]  # whatever the decoder counts for these records, the new call counts the same
    assert want_bad >= 2 and (kind not in BAD or want_bad == 2)
    for sg in (None, [1, -1, 1]):
        got = same_as_two_step(wires, x, n, sg, want_bad=want_bad)
        if kind in BAD:  # the good elements are the sum of the three wires, the bad ones lack wire 1
            ints = field_ints(got, n)
            s1 = -1 if sg else 1
            for e in (0, at[0] - 1, at[0], at[0] + 1, at[1], n - 1):
                assert ints[e] == (vals[0][e] + (0 if e in at else s1 * vals[1][e]) + vals[2][e]) % P, e
    with pytest.raises(ValueError, match=f"^sum_records_vec: {want_bad} records with x > 8 bytes or y > 68 bytes, "
                                         "0 records"):
        SS.sum_records_vec(wires, x, n)


# ---------------------------------------------------------------- 9. the deferred flag
def test_deferred_flag_adds_and_the_call_can_be_captured():
    x, n = 3, 150
    vals = [we.limbs_to_ints(we.ragged_limbs(n, 700 + i)) for i in range(3)]
    recs = [rec(x, v) for v in vals[1]]
    recs[5] = bytes([9]) + bytes(12)  # unrepresentable
    recs[77] = rec(4, vals[1][77])    # another x
    recs[78] = rec(5, vals[1][78])
    wires = [wire(x, vals[0])[0], raw_wire(recs)[0], wire(x, vals[2])[0]]
    flag = torch.zeros(2, dtype=torch.int32, device=dev())
    SS.sum_records_vec(wires, x, n, bad=flag)  # deferred: does not raise
    SS.sum_records_vec(wires, x, n, bad=flag)  # and adds
    assert flag.tolist() == [2, 4]
    with pytest.raises(ValueError, match="^sum_records_vec: 2 records with .*, 4 records whose x is not"):
        codec.check_bad_records(flag, what="sum_records_vec")
    # nothing in the deferred form reads back: a read-back would end the capture with an error
    want, _ = direct(wires, x, n, [1, -1, 1])
    big, out = guarded(n)
    flag.zero_()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        SS.sum_records_vec(wires, x, n, signs=[1, -1, 1], out=out, bad=flag)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want) and guards_intact(big) and flag.tolist() == [1, 2]


# ---------------------------------------------------------------- 10. re-encode
def test_the_sum_re_encodes_to_a_wire_that_decodes_to_it():
    x, n = 258, 300
    vals = [we.limbs_to_ints(we.ragged_limbs(n, 800 + i)) for i in range(3)]
    wires = [wire(x, v)[0] for v in vals]
    total = SS.sum_records_vec(wires, x, n)
    packed, offsets = codec.encode_share_vec(total, n, x)
    back, xs, bad = decode((packed, offsets), n)
    assert bad == 0 and torch.equal(back, total) and bool((xs == x).all())
    host = [bytes(r) for r in codec.records_to_list(packed.cpu(), offsets.cpu())]
    assert host == [shamir_mod._share_to_bytes((x, v)) for v in expect(vals)]
    # and is itself a wire this method reads
    again = SS.sum_records_vec([(packed, offsets)], None, n)
    assert torch.equal(again, total)
