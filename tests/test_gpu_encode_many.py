"""encode_shares_many (MI355X): the wires of a tensor list's share rows in one pass.

The wire of share x for a tensor list is the tensors' records back to back in
element order with one offsets[n_total + 1]: `codec.encode_share_vec` on every
(tensor, row), concatenated, the offsets rebased — and, record by record, the
reference's `_share_to_bytes((x, y_e))` (shamir.py:28-33).  Checked here
against that loop, against the reference's own golden bytes and
oracle.py_shamir.share_to_bytes, for reads of padding lanes, for writes outside
the outputs (where a tensor's partial last tile meets the next tensor's first
record inside one dword), for every store alignment, for row selection past
one launch group, past one pass of the tile scan, and as a round trip through
resolve_records_vec.  Every comparison is bit for bit.
"""
import random

import numpy as np
import pytest
import torch

from delta_node.crypto import shamir
from delta_node.crypto.shamir import _native, codec, field
from golden.fixtures import P, load_npz, manifest, secrets_int64
from oracle.py_shamir import share_to_bytes

pytestmark = pytest.mark.gpu

# an empty tensor, one-element tensors, sizes just below, at and above a wave
# and a tile, whole multi-tile tensors (tests/test_gpu_many.py's LIST_A: 8864
# elements, 46 tiles), and a list whose tensors all end on a wave boundary
LIST_A = [1, 63, 64, 65, 0, 127, 128, 1, 1, 1, 300, 257, 256, 1000, 4097, 2500]
LIST_B = [64, 192, 256, 320, 1024, 4096, 2048, 832]
EDGES = [0, 1, 255, 256, 2**64 - 1, 2**512, 2**520, P - 1]
XS3 = (1, 300, 2**40 + 3)  # 1, 2 and 6 abscissa bytes: three header lengths in one call


def dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _native.lib()


def _no_loop(*args, **kwargs):
    raise AssertionError("encode_shares_many fell back to the per-tensor encode_share_vec loop")


def many(monkeypatch, *args, **kwargs):
    """codec.encode_shares_many(...) with the per-tensor encoder made an error."""
    with monkeypatch.context() as m:
        m.setattr(codec, "encode_share_vec", _no_loop)
        return codec.encode_shares_many(*args, **kwargs)


def row_of(block, row):
    return block[row] if block.dim() == 2 else block


def the_loop(blocks, ns, xs, rows=None):
    """The per-(tensor, row) calls the many-call stands for: one (packed,
    offsets[n_total + 1]) per x, concatenated on the device, offsets rebased."""
    rows = [x - 1 for x in xs] if rows is None else rows
    wires = []
    for x, r in zip(xs, rows):
        parts, offs, base = [], [], 0
        for b, n in zip(blocks, ns):
            if not n:
                continue
            p, o = codec.encode_share_vec(row_of(b, r), n, x)
            parts.append(p)
            offs.append(o[:n] + base)
            base += p.numel()
        offs.append(torch.tensor([base], dtype=torch.int64, device=dev()))
        wires.append((torch.cat(parts) if parts else torch.empty(0, dtype=torch.uint8, device=dev()), torch.cat(offs)))
    return wires


def assert_wires(got, want):
    assert len(got) == len(want)
    for i, ((gp, go), (wp, wo)) in enumerate(zip(got, want)):
        assert gp.dtype == torch.uint8 and go.dtype == torch.int64 and gp.is_cuda and go.is_cuda, i
        assert go.shape == wo.shape and torch.equal(go, wo), i
        assert gp.shape == wp.shape and torch.equal(gp, wp), i


def live_mask(n: int) -> np.ndarray:
    """bool [vec_bytes(n)]: the bytes of a tiled vector that belong to its n elements."""
    nt = (n + 255) // 256
    m = np.zeros((nt, 66 * 256), dtype=bool)
    live = (np.arange(nt * 256) < n).reshape(nt, 256)
    m[:, :16 * 1024].reshape(nt, 16, 256, 4)[:] = live[:, None, :, None]
    m[:, 16 * 1024:].reshape(nt, 256, 2)[:] = live[:, :, None]
    return m.reshape(-1)


def ragged_values(sizes, n_rows, seed):
    """vals[row][k]: the tensors' field elements — many byte lengths (top limb
    zero in most: the low-limb length path), the edge values at every tensor's
    start and end and in the one-element tensors."""
    rng = random.Random(seed)
    vals = []
    for r in range(n_rows):
        per, ones = [], 0
        for k, n in enumerate(sizes):
            v = [rng.randrange(P) >> rng.randrange(0, 521) for _ in range(n)]
            if n == 1:
                v[0] = EDGES[(ones + 3 * r) % len(EDGES)]  # row 0: 0, 1, 255, 256: records of 2-3 bytes at x = 1
                ones += 1
            elif n > 1:
                v[0], v[-1] = EDGES[(k + r) % len(EDGES)], EDGES[(k + r + 3) % len(EDGES)]
            per.append(v)
        vals.append(per)
    return vals


def blocks_of(vals, sizes):
    """One device block [rows, vec_bytes(n_k)] per tensor from vals[row][k]."""
    return [torch.from_numpy(np.stack([field.ints_to_vec(vals[r][k]) if n else np.zeros(0, dtype=np.uint8)
                                       for r in range(len(vals))])).to(dev()) for k, n in enumerate(sizes)]


@pytest.fixture(scope="module")
def ragged():
    """LIST_A's blocks of 3 rows (never written), their values, and the loop's wires for XS3 on rows 0..2."""
    vals = ragged_values(LIST_A, 3, 20240611)
    blocks = blocks_of(vals, LIST_A)
    return blocks, vals, the_loop(blocks, LIST_A, XS3, rows=[0, 1, 2])


# ------------------------------------------------------------ 1. the reference's own bytes
@pytest.mark.parametrize("key,cuts", [("f1", [1, 255, 256, 257, 0, 255]), ("f2", [64, 1, 191])])
def test_reference_share_bytes(key, cuts, monkeypatch):
    cfg = manifest()[key]
    z = load_npz(cfg["file"])
    N, n, t = cfg["N"], cfg["n"], cfg["t"]
    assert sum(cuts) == N
    flat, offs = z["share_bytes"], z["share_offsets"]  # (an npz member is read again at every access)
    ss = shamir.SecretShare(t)
    ss.random.seed(cfg["mt_seed"])
    blocks = ss.make_shares_vec_many(list(torch.split(torch.from_numpy(z["secrets"]), cuts)), n)
    wires = many(monkeypatch, blocks, cuts)
    assert len(wires) == n
    for x, (packed, o) in zip(range(1, n + 1), wires):
        want = [flat[offs[e * n + x - 1]:offs[e * n + x]].tobytes() for e in range(N)]
        assert codec.records_to_list(packed.cpu(), o.cpu()) == want, x
        assert bytes(packed.cpu().numpy()) == b"".join(want), x
    assert_wires(wires, the_loop(blocks, cuts, list(range(1, n + 1))))


# ------------------------------------------------------------ 2. ragged and aligned lists
def test_ragged_list_edge_values_three_header_lengths(ragged, monkeypatch):
    blocks, vals, want = ragged
    got = many(monkeypatch, blocks, LIST_A, XS3, rows=[0, 1, 2])
    assert_wires(got, want)
    n_total = sum(LIST_A)
    for r, (x, (packed, o)) in enumerate(zip(XS3, got)):  # the reference's codec restated, record by record
        recs = [share_to_bytes(x, y) for per in vals[r] for y in per]
        assert o.shape == (n_total + 1,) and int(o[n_total]) == packed.numel()
        assert bytes(packed.cpu().numpy()) == b"".join(recs), x
        assert o.tolist() == list(np.cumsum([0] + [len(b) for b in recs])), x
    # the cases the list is there for did occur: a one-element tensor whose 2-3
    # byte record lies inside one aligned chunk between its neighbours' records
    # (the byte path), and records whose top limb is zero
    o = got[0][1].tolist()
    starts = np.cumsum([0] + LIST_A)
    lone = [int(starts[k]) for k, n in enumerate(LIST_A) if n == 1 and k > 0]
    inside = [e for e in lone if o[e + 1] - o[e] <= 3 and (o[e] + 15) // 16 * 16 > o[e + 1] // 16 * 16]
    assert inside, [(o[e], o[e + 1]) for e in lone]
    assert sum(1 for per in vals[0] for y in per if y < 2**512) > 1000


def test_aligned_list(monkeypatch):
    vals = ragged_values(LIST_B, 3, 7)
    blocks = blocks_of(vals, LIST_B)
    got = many(monkeypatch, blocks, LIST_B, XS3, rows=[0, 1, 2])
    assert_wires(got, the_loop(blocks, LIST_B, XS3, rows=[0, 1, 2]))
    packed, o = got[1]
    assert bytes(packed.cpu().numpy()) == b"".join(share_to_bytes(300, y) for per in vals[1] for y in per)


# ------------------------------------------------------------ 3. padding lanes are never read
def test_padding_lanes_do_not_influence_the_wires(ragged, monkeypatch):
    blocks, _, want = ragged
    dirty = []
    for b, n in zip(blocks, LIST_A):
        d = b.clone()
        if n:
            d[:, torch.from_numpy(~live_mask(n)).to(dev())] = 0xFF
        dirty.append(d)
    assert any(not torch.equal(d, b) for d, b in zip(dirty, blocks))
    assert_wires(many(monkeypatch, dirty, LIST_A, XS3, rows=[0, 1, 2]), want)


# ------------------------------------------------------------ 4. nothing outside the outputs
def _guarded(n_total, xs, shifts):
    """Per wire: (big out buffer of 0xA5, the out view at `shift` bytes past a
    16-byte boundary with capacity + 64 bytes, big offsets of -7 with 64 guard
    entries on both sides, the offsets view)."""
    bufs = []
    for x, sh in zip(xs, shifts):
        cap = codec.encoded_capacity(n_total, x)
        big = torch.full((cap + 64 + 16,), 0xA5, dtype=torch.uint8, device=dev())
        assert big.data_ptr() % 16 == 0
        out = big[sh:sh + cap + 64]
        obig = torch.full((n_total + 1 + 128,), -7, dtype=torch.int64, device=dev())
        bufs.append((big, out, obig, obig[64:64 + n_total + 1]))
    return bufs


def _check_guards(bufs, got, want, shifts):
    for (big, out, obig, oview), (gp, go), (wp, wo), sh in zip(bufs, got, want, shifts):
        total = wp.numel()
        assert gp.data_ptr() == out.data_ptr() and go.data_ptr() == oview.data_ptr()
        assert torch.equal(out[:total], wp) and torch.equal(oview, wo)
        assert bool((big[:sh] == 0xA5).all()) and bool((big[sh + total:] == 0xA5).all())  # at and beyond offsets[n_total]
        assert bool((obig[:64] == -7).all()) and bool((obig[64 + wo.numel():] == -7).all())


def test_canaries_around_out_and_offsets_and_blocks_unwritten(ragged, monkeypatch):
    blocks, _, want = ragged
    before = [b.clone() for b in blocks]
    shifts = [4, 0, 8]
    bufs = _guarded(sum(LIST_A), XS3, shifts)
    got = many(monkeypatch, blocks, LIST_A, XS3, rows=[0, 1, 2], outs=[b[1] for b in bufs],
               offsets=[b[3] for b in bufs])
    assert [g[0].numel() for g in got] == [w[0].numel() for w in want]  # trimmed views of the caller's buffers
    _check_guards(bufs, got, want, shifts)
    for b0, b1 in zip(before, blocks):
        assert torch.equal(b0, b1)


@pytest.mark.parametrize("shifts", [[4, 0, 8, 12, 0], [0, 12, 0, 4, 8]], ids=["4-0-8-12-0", "0-12-0-4-8"])
def test_out_alignments_mixed_in_one_call(shifts, monkeypatch):
    """Wires whose out is 4, 8 and 12 bytes past a 16-byte boundary (the 4-byte
    store path) beside 16-byte aligned ones (the wide path), in one call."""
    sizes = LIST_A
    sec = torch.from_numpy(secrets_int64(3, sum(sizes)))
    ss = shamir.SecretShare(3)
    ss.random.seed(5)
    blocks = ss.make_shares_vec_many(list(torch.split(sec, sizes)), 5)
    xs = [1, 2, 3, 4, 5]
    want = the_loop(blocks, sizes, xs)
    bufs = _guarded(sum(sizes), xs, shifts)
    assert [b[1].data_ptr() % 16 for b in bufs] == shifts
    got = many(monkeypatch, blocks, sizes, outs=[b[1] for b in bufs], offsets=[b[3] for b in bufs])
    _check_guards(bufs, got, want, shifts)


# ------------------------------------------------------------ 5. row selection
def test_row_selection_foreign_abscissa_and_one_dimensional_blocks(monkeypatch):
    sizes = LIST_A
    sec = torch.from_numpy(secrets_int64(11, sum(sizes)))
    ss = shamir.SecretShare(3)
    ss.random.seed(6)
    blocks = ss.make_shares_vec_many(list(torch.split(sec, sizes)), 5)
    assert_wires(many(monkeypatch, blocks, sizes, [2, 5]), the_loop(blocks, sizes, [2, 5]))
    # a row under an abscissa that is not its index + 1 (as a sum_shares_vec result carries)
    xs, rows = [7, 2**33 + 1, 0, 2**64 - 1], [0, 3, 4, 4]
    assert_wires(many(monkeypatch, blocks, sizes, xs, rows=rows), the_loop(blocks, sizes, xs, rows=rows))
    # 1-D blocks count as S = 1: the default abscissa is 1, the row 0
    flat = [b[2].clone() for b in blocks]
    assert_wires(many(monkeypatch, flat, sizes), the_loop(flat, sizes, [1], rows=[0]))
    assert_wires(many(monkeypatch, flat, sizes, [3], rows=[0]), the_loop(blocks, sizes, [3]))


def test_seventeen_rows_past_one_launch_group(monkeypatch):
    sizes = [1, 300, 64]
    sec = torch.from_numpy(secrets_int64(13, sum(sizes)))
    ss = shamir.SecretShare(2)
    ss.random.seed(8)
    blocks = ss.make_shares_vec_many(list(torch.split(sec, sizes)), 17)
    got = many(monkeypatch, blocks, sizes)
    assert len(got) == 17
    assert_wires(got, the_loop(blocks, sizes, list(range(1, 18))))


# ------------------------------------------------------------ 6. past one pass of the tile scan
def test_more_tiles_than_one_scan_pass(monkeypatch):
    """8192 tile totals are staged per scan pass: 2^21 elements fill one pass
    exactly, the two tensors behind them (a partial last tile each) lie in the
    second.  Shares from the device PRNG split; compared on the device."""
    sizes = [1 << 21, 4097, 255]
    assert sum((n + 255) // 256 for n in sizes) > 8192 and sizes[0] // 256 == 8192
    ss = shamir.SecretShare(2)
    g = torch.Generator(device=dev()).manual_seed(17)
    blocks = []
    for k, n in enumerate(sizes):
        sec = torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, device=dev(), generator=g)
        block, _ = ss.make_shares_vec_prng(sec, 2, key=bytes(range(32)), nonce=k)
        blocks.append(block.clone())
    (packed, o), = many(monkeypatch, blocks, sizes, [1])
    (wp, wo), = the_loop(blocks, sizes, [1])
    assert torch.equal(o, wo)
    assert packed.shape == wp.shape and torch.equal(packed, wp)


# ------------------------------------------------------------ 7. caller buffers, trim, empty input
def test_caller_buffers_and_trim(ragged, monkeypatch):
    blocks, _, want = ragged
    n_total = sum(LIST_A)
    caps = [codec.encoded_capacity(n_total, x) for x in XS3]
    outs = [torch.zeros(c, dtype=torch.uint8, device=dev()) for c in caps]
    offs = [torch.zeros(n_total + 5, dtype=torch.int64, device=dev()) for _ in XS3]
    got = many(monkeypatch, blocks, LIST_A, XS3, rows=[0, 1, 2], trim=False, outs=outs, offsets=offs)
    for (gp, go), (wp, wo), out, off, cap in zip(got, want, outs, offs, caps):
        assert gp.data_ptr() == out.data_ptr() and gp.numel() == cap  # full capacity, in the given buffer
        assert go.data_ptr() == off.data_ptr() and go.shape == (n_total + 1,)
        assert torch.equal(go, wo) and torch.equal(gp[: int(go[n_total])], wp)
    # allocated, untrimmed: full-capacity tensors, the same bytes below offsets[n_total]
    got = many(monkeypatch, blocks, LIST_A, XS3, rows=[0, 1, 2], trim=False)
    for (gp, go), (wp, wo), cap in zip(got, want, caps):
        assert gp.numel() == cap and torch.equal(go, wo) and torch.equal(gp[: int(go[n_total])], wp)
    # allocated, trimmed (the default) equals the loop's trimmed result
    assert_wires(many(monkeypatch, blocks, LIST_A, XS3, rows=[0, 1, 2]), want)
    with pytest.raises(ValueError, match="outs\\[1\\]"):
        many(monkeypatch, blocks, LIST_A, XS3, rows=[0, 1, 2], outs=[outs[0], outs[1][:-1], outs[2]])
    with pytest.raises(ValueError, match="4-byte aligned"):
        big = torch.zeros(caps[0] + 16, dtype=torch.uint8, device=dev())
        many(monkeypatch, blocks, LIST_A, XS3, rows=[0, 1, 2], outs=[big[2:], outs[1], outs[2]])
    with pytest.raises(ValueError, match="offsets\\[2\\]"):
        many(monkeypatch, blocks, LIST_A, XS3, rows=[0, 1, 2], offsets=[offs[0], offs[1], offs[2][:n_total]])


def test_empty_list_and_list_of_empty_tensors(monkeypatch):
    for trim in (True, False):
        got = many(monkeypatch, [], [], [1, 300], trim=trim)
        assert len(got) == 2
        for packed, o in got:
            assert packed.is_cuda and packed.dtype == torch.uint8 and o.dtype == torch.int64 and o.tolist() == [0]
            assert packed.numel() == 0 or not trim
    assert many(monkeypatch, [], []) == []
    empties = [torch.empty((5, 0), dtype=torch.uint8, device=dev()) for _ in range(2)]
    got = many(monkeypatch, empties, [0, 0])
    assert len(got) == 5
    for packed, o in got:
        assert packed.numel() == 0 and packed.is_cuda and o.tolist() == [0]
    obuf = torch.full((4,), -7, dtype=torch.int64, device=dev())
    (packed, o), = many(monkeypatch, empties, [0, 0], [3], offsets=[obuf])
    assert o.data_ptr() == obuf.data_ptr() and obuf.tolist() == [0, -7, -7, -7]


# ------------------------------------------------------------ 8. through the receiver
def test_round_trip_through_resolve_records_vec(monkeypatch):
    sizes = LIST_A
    n_total = sum(sizes)
    sec = torch.from_numpy(secrets_int64(21, n_total)).to(dev())
    tensors = list(torch.split(sec, sizes))
    ss = shamir.SecretShare(3)
    ss.random.seed(9)
    blocks = ss.make_shares_vec_many(tensors, 5)
    wires = many(monkeypatch, blocks, sizes)
    for xs in ([1, 3, 5], [2, 4, 5]):
        bad = torch.zeros(2, dtype=torch.int32, device=dev())
        got, over = ss.resolve_records_vec([wires[x - 1] for x in xs], xs, n_total, return_overflow=True, bad=bad)
        assert torch.equal(got, torch.cat(tensors)), xs
        assert bad.tolist() == [0, 0] and int(over.item()) == 0, xs
        for g, x in zip(torch.split(got, sizes), tensors):  # the caller splits by views
            assert torch.equal(g, x)
