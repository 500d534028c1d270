"""sum_shares_vec (MI355X): members' share vectors summed mod p in one launch.

out_e = (sum_i +-y_{i,e}) mod p, canonical, for every lane of every tile —
checked against Python integers on inputs built to reach the carry, bound and
canonical-form edges (field_edges.edge_values(), p itself included), against
today's private route (`_native.reconstruct` with all-ones weights), against
the reference's own golden shares, as the party-side step of a protocol round
trip, over vectors, blocks and a flat list buffer alike, in place and between
guard bytes, with every wave striding over several tiles, and on a
non-default stream without host synchronisation.  Integer field arithmetic:
every comparison is bit-exact.
"""
import functools
import os
import random
import re

import numpy as np
import pytest
import torch

import field_edges as fe
from delta_node.crypto import shamir
from delta_node.crypto.shamir import _native, field
from golden.fixtures import load_npz, manifest, secrets_int64

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = fe.P
TB = field.TILE_BYTES


def sum_group() -> int:
    """DN_M521_SUM_GROUP as include/dn_shamir.h defines it (its one definition)."""
    with open(os.path.join(ROOT, "include", "dn_shamir.h")) as f:
        found = re.findall(r"^#define\s+DN_M521_SUM_GROUP\s+(\d+)\s*$", f.read(), flags=re.M)
    assert len(found) == 1, found
    return int(found[0])


GROUP = sum_group()
EDGE_MS = [1, 2, 3, 5, 16, 17, GROUP - 1, GROUP, GROUP + 1, 2 * GROUP + 1]


def tiles_for(m: int) -> int:
    return 5 if m <= 17 else 2


def dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _native.lib()


SS = shamir.SecretShare(3)


# ------------------------------------------------------------ the edge rows
# Pinned columns: (name, column values for m rows, predicate on the integer sum).
def _pins(m: int):
    pins = [("all-p", [P] * m, lambda S: S == m * P),
            ("all-p-1", [P - 1] * m, lambda S: S % P == (-m) % P)]
    if m >= 2:
        y = fe.edge_values()[37]
        assert 0 < y < P
        pins.append(("y-and-p-y", [y, P - y] + [0] * (m - 2), lambda S: S == P))
        # y_0 + y_1 = 2^521 + X, X = limbs 0..k all ones: the fold adds 1 to limb 0 and the carry runs
        # through k more all-ones limbs (k = 15: into the 9-bit top limb)
        for k in (0, 1, 7, 15):
            X = (1 << (32 * (k + 1))) - 1
            pred = fe.pred_carry0 if k == 0 else fe.pred_carry_multi
            pins.append((f"carry-{k}", [(1 << 520) + X, 1 << 520] + [0] * (m - 2), pred))
    return pins


def _pin_lanes(j: int, tiles: int):
    return [5 + 36 * j, 256 * (tiles - 1) + 250 - 36 * j]  # one in the first tile, one in the last


@functools.lru_cache(maxsize=None)
def edge_case(m: int):
    """(rows as Python ints [m][lanes], device tensor [m, tiles * TB]): row i,
    lane e takes edge[(e (2 i + 1) + i) % len], the pinned columns on top.
    Built once per m and never written."""
    tiles = tiles_for(m)
    lanes = 256 * tiles
    pool = fe.edge_values()
    assert P in pool
    L = len(pool)
    e = np.arange(lanes, dtype=np.int64)
    idx = np.stack([(e * (2 * i + 1) + i) % L for i in range(m)])  # [m, lanes]
    rows = [[pool[k] for k in idx[i]] for i in range(m)]
    for j, (name, col, pred) in enumerate(_pins(m)):
        assert pred(sum(col)), (name, m)  # the coverage is stated, not assumed
        for lane in _pin_lanes(j, tiles):
            for i in range(m):
                rows[i][lane] = col[i]
    host = np.stack([field.ints_to_vec(r) for r in rows])
    return rows, torch.from_numpy(host).to(dev())


def expected_vec(rows, signs=None) -> torch.Tensor:
    m, lanes = len(rows), len(rows[0])
    sg = signs or [1] * m
    want = [sum(s * rows[i][e] for i, s in enumerate(sg)) % P for e in range(lanes)]
    return torch.from_numpy(field.ints_to_vec(want))


# ------------------------------------------------------------ 1. exact at the edges
@pytest.mark.parametrize("m", EDGE_MS)
def test_exact_against_python_integers_at_the_edges(m):
    rows, blk = edge_case(m)
    got = SS.sum_shares_vec(list(blk.unbind(0)))
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == blk[0].shape and got.is_contiguous()
    want = expected_vec(rows)
    assert torch.equal(got.cpu(), want)
    # the pinned columns, spelled out: multiples of p give 0 (not p), m (p - 1) gives -m
    tiles = tiles_for(m)
    res = field.vec_to_ints(got.cpu().numpy(), 256 * tiles)
    for j, (name, col, _) in enumerate(_pins(m)):
        for lane in _pin_lanes(j, tiles):
            exp = {"all-p": 0, "y-and-p-y": 0, "all-p-1": (-m) % P}.get(name, sum(col) % P)
            assert res[lane] == exp, (name, lane)
    assert all(0 <= v < P for v in res)


# ------------------------------------------------------------ 2. signs
@pytest.mark.parametrize("m", [1, 2, 5, 17, GROUP, GROUP + 1])
def test_signs(m):
    rows, blk = edge_case(m)
    rng = random.Random(4000 + m)
    for signs in ([rng.choice((1, -1)) for _ in range(m)], [-1] * m, [1] * m):
        got = SS.sum_shares_vec(blk, signs=signs)
        assert torch.equal(got.cpu(), expected_vec(rows, signs)), signs[:8]


def test_minus_zero_and_minus_p_are_canonical_zero():
    vals = [0, P] * 128  # one tile, m = 1, subtracted: p - 0 = p and p - p = 0 must both store 0
    v = torch.from_numpy(field.ints_to_vec(vals)).to(dev())
    for signs in ([-1], [1]):
        got = SS.sum_shares_vec([v], signs=signs)
        assert not got.any().item(), signs


# ------------------------------------------------------------ 3. equals today's private path
def live_mask(n: int) -> np.ndarray:
    """bool [vec_bytes(n)]: the bytes of a tiled vector that belong to its n elements."""
    nt = (n + 255) // 256
    m = np.zeros((nt, 66 * 256), dtype=bool)
    live = (np.arange(nt * 256) < n).reshape(nt, 256)
    m[:, :16 * 1024].reshape(nt, 16, 256, 4)[:] = live[:, None, :, None]
    m[:, 16 * 1024:].reshape(nt, 256, 2)[:] = live[:, :, None]
    return m.reshape(-1)


@functools.lru_cache(maxsize=None)
def drawn_rows(m: int, n: int) -> torch.Tensor:
    """m tiled vectors of n random field elements in [1, p - 1] on the device (never written)."""
    ys = _native.mt_draw_coeffs(random.Random(9000 + m), n, m)
    return torch.from_numpy(np.ascontiguousarray(ys).reshape(m, field.vec_bytes(n))).to(dev())


def ones_path(rows: torch.Tensor, n: int) -> torch.Tensor:
    """The private route: one reconstruct with all-ones weights (at most 16 rows)."""
    ref = torch.empty(field.vec_bytes(n), dtype=torch.uint8, device=rows.device)
    _native.reconstruct(list(rows.unbind(0)), _native.ones_weights(rows.shape[0]), out_fe=ref, n=n)
    return ref


@pytest.mark.parametrize("m", [2, 3, 5, 7, 16])
def test_equals_the_ones_weights_reconstruct(m):
    n = 1000
    rows = drawn_rows(m, n)
    got = SS.sum_shares_vec(rows)
    ref = ones_path(rows, n)
    mask = torch.from_numpy(live_mask(n)).to(dev())
    assert torch.equal(got[mask], ref[mask])
    assert not rows[:, ~mask].any().item() and not got[~mask].any().item()  # zero padding in, zero padding out


# ------------------------------------------------------------ 4. reference pins
@pytest.mark.parametrize("key,overflowing", [("f1", 247), ("f2", 63)])
def test_reference_shares_summed_over_four_members(key, overflowing):
    """The reference's own shares, cut into 4 members of consecutive elements:
    the summed rows equal the Python-integer sums, and every golden subset of
    the summed rows reconstructs the members' wrapping int64 sum."""
    cfg = manifest()[key]
    z = load_npz(cfg["file"])
    N, n = cfg["N"], cfg["n"]
    q = N // 4
    limbs = z["share_limbs"]  # [N, n, 17]
    blocks = [torch.from_numpy(np.stack([field.limbs_to_vec(limbs[j * q:(j + 1) * q, s, :]) for s in range(n)])).to(dev())
              for j in range(4)]
    summed = shamir.SecretShare(cfg["t"]).sum_shares_vec(blocks)
    assert tuple(summed.shape) == (n, field.vec_bytes(q))
    for s in range(n):
        ints = [field.limbs_to_ints(limbs[j * q:(j + 1) * q, s, :]) for j in range(4)]
        want = [sum(col) % P for col in zip(*ints)]
        assert field.vec_to_ints(summed[s].cpu().numpy(), q) == want, s
    want_sum = torch.from_numpy(z["secrets"].reshape(4, -1).sum(0, dtype=np.int64)).to(dev())  # wraps
    ss = shamir.SecretShare(cfg["t"])
    for sub, size in zip(z["recon_subsets"], z["recon_sizes"]):
        xs = [int(x) for x in sub[:size]]
        got, over = ss.resolve_shares_vec([summed[x - 1] for x in xs], xs, q, return_overflow=True)
        assert torch.equal(got, want_sum), xs
        assert int(over.item()) == overflowing, xs  # the elements whose unsigned sums reach 2^64


# ------------------------------------------------------------ 5. protocol round trip
def test_protocol_round_trip():
    t, shares, n, members = 3, 5, 1000, 7
    vb = field.vec_bytes(n)
    secs = [torch.from_numpy(secrets_int64(300 + j, n)).to(dev()) for j in range(members)]
    blocks = []
    for j, sec in enumerate(secs):
        ss = shamir.SecretShare(t)
        ss.random.seed(500 + j)
        blocks.append(ss.make_shares_vec(sec, shares, out=torch.empty((shares, vb), dtype=torch.uint8, device=dev())))
    ss = shamir.SecretShare(t)
    party = {}
    for x in (2, 4, 5):  # party x holds row x - 1 of every member's block
        as_tensor = ss.sum_shares_vec(torch.stack([b[x - 1] for b in blocks]))
        as_list = ss.sum_shares_vec([b[x - 1] for b in blocks])
        assert tuple(as_tensor.shape) == (vb,) and torch.equal(as_tensor, as_list)
        party[x] = as_list
    xs = [2, 4, 5]
    got = ss.resolve_shares_vec([party[x] for x in xs], xs, n)
    assert torch.equal(got, torch.stack(secs).sum(0))  # int64, wrapping


# ------------------------------------------------------------ 6. shapes in one call
def test_vectors_blocks_and_the_flat_list_buffer_agree():
    sizes, shares, members = [1, 255, 256, 257, 1000], 5, 3
    vbs = [field.vec_bytes(n) for n in sizes]
    flats, views = [], []
    for j in range(members):
        flat = torch.zeros(shares * sum(vbs), dtype=torch.uint8, device=dev())
        outs = [p.view(shares, vb) for p, vb in zip(torch.split(flat, [shares * vb for vb in vbs]), vbs)]
        ss = shamir.SecretShare(3)
        ss.random.seed(60 + j)
        tensors = list(torch.split(torch.from_numpy(secrets_int64(70 + j, sum(sizes))).to(dev()), sizes))
        got = ss.make_shares_vec_many(tensors, shares, outs=outs)
        assert all(g is o for g, o in zip(got, outs))
        flats.append(flat)
        views.append(outs)
    whole = SS.sum_shares_vec(flats)  # one call over the whole list buffer
    assert tuple(whole.shape) == (shares * sum(vbs),)
    parts = torch.split(whole, [shares * vb for vb in vbs])
    for k, vb in enumerate(vbs):
        as_block = SS.sum_shares_vec([v[k] for v in views])  # [shares, vb]
        assert tuple(as_block.shape) == (shares, vb)
        assert torch.equal(as_block.reshape(-1), parts[k]), k
        for s in range(shares):
            as_vec = SS.sum_shares_vec([v[k][s] for v in views])  # [vb]
            assert torch.equal(as_vec, as_block[s]), (k, s)
    # and it is the sum: every tensor of the list reconstructs the members' sum
    xs = [1, 3, 4]
    for k, n in enumerate(sizes):
        got = shamir.SecretShare(3).resolve_shares_vec([parts[k].view(shares, vbs[k])[x - 1] for x in xs], xs, n)
        lo = sum(sizes[:k])
        want = sum(torch.from_numpy(secrets_int64(70 + j, sum(sizes))[lo:lo + n]) for j in range(members))
        assert torch.equal(got.cpu(), want), k


# ------------------------------------------------------------ 7. in place and bounds
@pytest.mark.parametrize("m,at", [(5, 0), (2 * GROUP + 1, GROUP + 3)], ids=["out-is-block-0", "out-is-block-GROUP+3"])
def test_in_place_between_guard_bytes(m, at):
    rows, blk = edge_case(m)
    size, guard = blk.shape[1], 4096
    rng = random.Random(m)
    signs = [rng.choice((1, -1)) for _ in range(m)]
    want = SS.sum_shares_vec(blk, signs=signs)  # out of place
    assert torch.equal(want.cpu(), expected_vec(rows, signs))
    buf = torch.full((guard + size + guard,), 0xA5, dtype=torch.uint8, device=dev())
    out = buf[guard:guard + size]
    out.copy_(blk[at])
    inputs = [out if i == at else blk[i] for i in range(m)]
    before = blk.clone()
    got = SS.sum_shares_vec(inputs, signs=signs, out=out)
    assert got is out
    assert torch.equal(out, want)
    assert torch.equal(blk, before)  # every other input unchanged
    host = buf.cpu()
    assert bool((host[:guard] == 0xA5).all()) and bool((host[guard + size:] == 0xA5).all())
    # out of place into a guarded buffer as well
    buf2 = torch.full((guard + size + guard,), 0xA5, dtype=torch.uint8, device=dev())
    got2 = SS.sum_shares_vec(blk, signs=signs, out=buf2[guard:guard + size])
    assert torch.equal(got2, want)
    host = buf2.cpu()
    assert bool((host[:guard] == 0xA5).all()) and bool((host[guard + size:] == 0xA5).all())


# ------------------------------------------------------------ 8. stride loop
@pytest.mark.parametrize("cap", [2, 3])
def test_every_wave_strides_over_several_tiles(cap, monkeypatch):
    """The tuning build under DN_GRID_CAP: 4 * cap waves (8, 12) over 29 tiles
    — every wave takes more than one tile and the last pass is a partial one,
    whether the kernel's unit of work is a tile, half a tile or a quarter (29,
    58 and 116 are multiples of neither 8 nor 12) — against the all-ones
    reconstruct of the product build."""
    n, m = 29 * 256 - 19, 7
    rows = drawn_rows(m, n)
    ref = ones_path(rows, n)
    monkeypatch.setenv("DN_GRID_CAP", str(cap))
    with _native.library(_native.TUNING_LIB):
        got = SS.sum_shares_vec(rows, signs=[1] * m)
        neg = SS.sum_shares_vec(rows, signs=[-1] * m)
    mask = torch.from_numpy(live_mask(n)).to(dev())
    assert torch.equal(got[mask], ref[mask])
    back = SS.sum_shares_vec([neg], signs=[-1])  # -(-S) = S, by the product build
    assert torch.equal(back[mask], ref[mask])


# ------------------------------------------------------------ 9. streams
def test_non_default_stream_and_back_to_back_calls():
    n = 1000
    a, b = drawn_rows(5, n), drawn_rows(16, n)
    ref_a, ref_b = ones_path(a, n), ones_path(b, n)
    mask = torch.from_numpy(live_mask(n)).to(dev())
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got_a = SS.sum_shares_vec(a)
        got_b = SS.sum_shares_vec(b)  # no host synchronisation in between
        acc = SS.sum_shares_vec([got_a, got_b], out=got_a)  # and a third, in place on the first result
    stream.synchronize()
    assert torch.equal(got_b[mask], ref_b[mask])
    both = SS.sum_shares_vec([ref_a, ref_b])
    torch.cuda.synchronize()
    assert acc is got_a and torch.equal(acc[mask], both[mask])


# ------------------------------------------------------------ 10. full size
@pytest.mark.slow
def test_full_size_equals_the_ones_weights_reconstruct():
    n, m = 1 << 24, 10
    rows = torch.empty((m, field.vec_bytes(n)), dtype=torch.uint8, device=dev())
    assert _native.mt_draw_coeffs_device(random.Random(77), n, m, rows)
    got = SS.sum_shares_vec(rows)
    ref = ones_path(rows, n)
    assert torch.equal(got, ref)  # 2^24 is whole tiles: no padding lanes
