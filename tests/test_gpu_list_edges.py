"""The tensor-list kernels where segments meet substreams and strides (MI355X).

make_shares_vec_many's segmented emission (emit_split_seg, emit_pieces and the
seg_find / seg_step cursor) on the lists of tests/list_edges.py — groups of 64
one-element tensors inside a backward substream, segment boundaries on and
beside substream boundaries, one 64-element tensor per group, pieces that cross
a tile inside a group, a last partial group of several segments — at t = 2, 3
and 5, from a freshly seeded generator and from one that is mid-array, through
the two-wave kernels of the product build and the one-wave kernels of the
tuning build, and at the 2^12-draw substream length.  resolve_shares_vec_many's
strided tile loop and forward cursor under every wave schedule with 4 to 32
waves over 115 tiles.  The reference is Python integers (list_edges.py, pinned
to the reference implementation's fixtures by test_list_edges_host.py); at the
2^12 length, the host draw and the non-fused split.  Integer field arithmetic:
every comparison is bit for bit.
"""
import functools
import random
import sys

import numpy as np
import pytest
import torch

import field_edges as fe
import list_edges as le
from delta_node.crypto import shamir
from delta_node.crypto.shamir import _native, codec, field
from golden.fixtures import INT64_MAX, INT64_MIN, secrets_int64

pytestmark = pytest.mark.gpu

shamir_mod = sys.modules["delta_node.crypto.shamir.shamir"]
P = fe.P
TB = field.TILE_BYTES
GUARD, CANARY = 4096, 0xA5
SEED = 4242
SHAPES = [(2, 3), (3, 5), (3, 7), (5, 9)]
NMAX = {2: 3, 3: 7, 5: 9}  # the most shares a threshold is run with: one reference per (list, t, pre)


def dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _native.lib()


def _not_the_loop(*args, **kwargs):
    raise AssertionError("the many-call fell back to the per-tensor path")


# ------------------------------------------------------------ inputs and references (built once, never written)
def list_secrets(n_total: int, seed: int) -> np.ndarray:
    sec = secrets_int64(seed, n_total)
    sec[0], sec[-1] = INT64_MIN, INT64_MAX
    sec[n_total // 2], sec[n_total // 3] = -1, 0
    sec.setflags(write=False)
    return sec


@functools.lru_cache(maxsize=None)
def split_case(name: str, t: int, pre: int):
    """(sizes, int64 secrets, expected share limbs uint32 [NMAX[t], n_total, 17],
    the generator's state after the draw) of list `name` at threshold t with
    `pre` words drawn before the call."""
    sizes = le.build(name, t)
    n_total = sum(sizes)
    sec = list_secrets(n_total, 100 * t + len(name))
    r = le.replayed(SEED + t, pre)
    rows = le.split_reference([int(s) for s in sec], [n_total], t, NMAX[t], r)
    limbs = np.stack([field.ints_to_limbs(row[0]) for row in rows])
    limbs.setflags(write=False)
    return sizes, sec, limbs, r.getstate()


def seeded(t: int, pre: int) -> shamir.SecretShare:
    ss = shamir.SecretShare(t)
    ss.random.seed(SEED + t)
    if pre:
        ss.random.getrandbits(32 * pre)
    return ss


def guarded_blocks(sizes, shares: int):
    """One canary-filled buffer, a [shares, vec_bytes(n_k)] block per tensor
    carved from it with GUARD bytes before, between and after."""
    vbs = [field.vec_bytes(n) for n in sizes]
    total = GUARD + sum(shares * vb + GUARD for vb in vbs)
    buf = torch.full((total,), CANARY, dtype=torch.uint8, device=dev())
    outs, offs, off = [], [], GUARD
    for vb in vbs:
        outs.append(buf[off:off + shares * vb].view(shares, vb))
        offs.append(off)
        off += shares * vb + GUARD
    assert off == total
    return buf, outs, offs


def block_limbs(v: np.ndarray, shares: int, n: int) -> np.ndarray:
    """Host bytes of a [shares, vec_bytes(n)] block -> uint32 [shares, n, 17] (the n live elements)."""
    nt = (n + 255) // 256
    v = v.reshape(shares, nt, TB)
    lo = np.ascontiguousarray(v[:, :, :64 * 256]).view("<u4").reshape(shares, nt, 16, 256)
    hi = np.ascontiguousarray(v[:, :, 64 * 256:]).view("<u2").reshape(shares, nt, 256)
    out = np.empty((shares, nt, 256, 17), dtype=np.uint32)
    out[..., :16] = lo.transpose(0, 1, 3, 2)
    out[..., 16] = hi
    return out.reshape(shares, nt * 256, 17)[:, :n]


def gathered_limbs(host: np.ndarray, offs, sizes, shares: int) -> np.ndarray:
    """The blocks' live elements, tensors in order: uint32 [shares, n_total, 17]."""
    got = np.empty((shares, sum(sizes), 17), dtype=np.uint32)
    e = 0
    for off, n in zip(offs, sizes):
        if n:
            got[:, e:e + n] = block_limbs(host[off:off + shares * field.vec_bytes(n)], shares, n)
            e += n
    return got


def where_it_differs(got: np.ndarray, want: np.ndarray, sizes, t: int) -> str:
    """The first differing (share, element, limb) as (tensor, local element) and
    (substream, direction, group, lane, table entry) of the draw's geometry."""
    bad = np.argwhere(got != want)
    if not len(bad):
        return "equal"
    s, e, limb = (int(v) for v in bad[0])
    n_total = sum(sizes)
    draws, S, backward = le.substream_plan(n_total, t)
    E = le.elems_per_substream(t, draws)
    begins = le.seg_begins(sizes)
    k = le.seg_of(begins, e)
    live = [j for j, n in enumerate(sizes) if n]
    sub = e // E
    return (f"{len(bad)} limbs differ, first: share {s + 1} element {e} limb {limb} = tensor {live[k]} "
            f"(table entry {k}, size {sizes[live[k]]}) element {e - begins[k]}; substream {sub} of {S} "
            f"({'backward' if sub in backward else 'forward'}) group {(e % E) // 64} lane {e % 64}; "
            f"got {got[s, e, limb]:#x} want {want[s, e, limb]:#x}")


def assert_guards(host: np.ndarray, offs, sizes, shares: int) -> None:
    end = 0
    for off, n in zip(offs, sizes):
        assert (host[end:off] == CANARY).all(), ("guard before the block at", off)
        end = off + shares * field.vec_bytes(n)
    assert (host[end:] == CANARY).all(), "the last guard"


def run_split_list(name: str, t: int, n: int, pre: int):
    """make_shares_vec_many on list `name` into guarded caller blocks, checked
    against the Python-integer reference.  Returns (ss, outs, the secrets' views)."""
    sizes, sec, limbs, state = split_case(name, t, pre)
    flat = torch.from_numpy(sec.copy()).to(dev())
    views = list(torch.split(flat, sizes))  # consecutive views of one device buffer
    buf, outs, offs = guarded_blocks(sizes, n)
    ss = seeded(t, pre)
    ss.make_shares_vec = _not_the_loop
    got = ss.make_shares_vec_many(views, n, outs=outs)
    assert len(got) == len(outs) and all(g is o for g, o in zip(got, outs))
    host = buf.cpu().numpy()
    have, want = gathered_limbs(host, offs, sizes, n), limbs[:n]
    assert np.array_equal(have, want), where_it_differs(have, want, sizes, t)
    assert_guards(host, offs, sizes, n)
    assert ss.random.getstate() == state
    assert ss.last_draw_rejected is False
    assert torch.equal(flat.cpu(), torch.from_numpy(sec.copy()))  # the secrets are only read
    return ss, outs, views


# ------------------------------------------------------------ a. the lists through the product kernels
@pytest.mark.parametrize("pre", [0, 333], ids=["fresh", "mid-array"])
@pytest.mark.parametrize("name", le.MAIN_LISTS)
@pytest.mark.parametrize("t,n", SHAPES, ids=["2of3", "3of5", "3of7", "5of9"])
def test_many_on_the_edge_lists(t, n, name, pre):
    run_split_list(name, t, n, pre)


@pytest.mark.parametrize("t,n", [(2, 3), (3, 5), (5, 9)], ids=["2of3", "3of5", "5of9"])
def test_many_with_empty_tensors_at_both_ends(t, n):
    run_split_list("EMPTY_ENDS", t, n, 333)


@pytest.mark.parametrize("t,n", [(2, 3), (3, 5), (5, 9)], ids=["2of3", "3of5", "5of9"])
def test_many_of_a_single_tensor_equals_make_shares_vec(t, n):
    _, outs, views = run_split_list("SINGLE", t, n, 0)
    size = views[0].numel()
    single = seeded(t, 0).make_shares_vec(views[0], n)
    a = block_limbs(outs[0].cpu().numpy().reshape(-1), n, size)
    b = block_limbs(single.cpu().numpy().reshape(-1), n, size)
    assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------ b. the one-wave SEG kernels
@pytest.mark.parametrize("name", ["ONES", "BOUNDS"])
@pytest.mark.parametrize("t,n", SHAPES, ids=["2of3", "3of5", "3of7", "5of9"])
def test_one_wave_seg_kernels(t, n, name, monkeypatch):
    """mt_gen_kernel<T, ..., SEG> (the tuning build under DN_MT_PC_FORCE=0: one
    wave per substream generates and emits) — both share-count forms of t = 3."""
    monkeypatch.setenv("DN_MT_PC_FORCE", "0")
    with _native.library(_native.TUNING_LIB):
        run_split_list(name, t, n, 0)


# ------------------------------------------------------------ c. the 2^12-draw length
def dev_planes(blk: torch.Tensor, shares: int, n: int):
    """A device block [shares, vec_bytes(n)] untiled: (int32 [shares, 16, n], int16 [shares, n])."""
    nt = (n + 255) // 256
    v = blk.reshape(shares, nt, TB)
    lo = v[:, :, :64 * 256].contiguous().view(torch.int32).view(shares, nt, 16, 256)
    lo = lo.permute(0, 2, 1, 3).reshape(shares, 16, nt * 256)[:, :, :n]
    hi = v[:, :, 64 * 256:].contiguous().view(torch.int16).view(shares, nt * 256)[:, :n]
    return lo, hi


def test_many_at_the_2e12_draw_length():
    """t = 5, n = 9, 2^19 + 77 elements = 2^21 + 308 coefficients: 513
    substreams of 2^12 draws (E = 1024), a group of 64 one-element tensors in
    every group of backward substream 2, cuts at 4E and 5E, a last partial
    group of four segments — against the host draw and the non-fused split of
    the concatenation, compared on the device over the live elements."""
    t, n, pre = 5, 9, 333
    sizes = le.big_list()
    N = sum(sizes)
    assert le.substream_plan(N, t)[0] == 1 << 12
    sec = torch.from_numpy(list_secrets(N, 77).copy()).to(dev())
    ref = le.replayed(SEED, pre)
    co = torch.from_numpy(_native.mt_draw_coeffs(ref, N, t - 1)).to(dev())
    want = torch.zeros((n, field.vec_bytes(N)), dtype=torch.uint8, device=dev())
    _native.split_u64(sec, co, want, N, t, n)
    want_lo, want_hi = dev_planes(want, n, N)
    del co
    vbs = [field.vec_bytes(k) for k in sizes]
    buf = torch.full((sum(n * vb for vb in vbs),), CANARY, dtype=torch.uint8, device=dev())
    outs = [p.view(n, vb) for p, vb in zip(torch.split(buf, [n * vb for vb in vbs]), vbs)]
    ss = shamir.SecretShare(t)
    ss.random.seed(SEED)
    ss.random.getrandbits(32 * pre)
    ss.make_shares_vec = _not_the_loop
    got = ss.make_shares_vec_many(list(torch.split(sec, sizes)), n, outs=outs)
    assert all(g is o for g, o in zip(got, outs))
    planes = [dev_planes(o, n, k) for o, k in zip(outs, sizes) if k]
    got_lo = torch.cat([p[0] for p in planes], dim=2)
    got_hi = torch.cat([p[1] for p in planes], dim=1)
    if not torch.equal(got_lo, want_lo):
        s, limb, e = (int(v) for v in (got_lo != want_lo).nonzero()[0])
        raise AssertionError(f"share {s + 1} element {e} limb {limb}: substream {e // 1024}, group "
                             f"{(e % 1024) // 64}, lane {e % 64}, table entry {le.seg_of(le.seg_begins(sizes), e)}")
    assert torch.equal(got_hi, want_hi)
    assert ss.random.getstate() == ref.getstate()
    assert ss.last_draw_rejected is False


# ------------------------------------------------------------ d. resolve_shares_vec_many under strides
# 115 tiles in 53 non-empty tensors: runs of 11, 9, 10 and 13 one-element tensors (one tile each: a stride of 4,
# 8, 12 or 32 tiles crosses as many table entries in one recon_seg_step), empties (one pair), a tile less one,
# a tile, a tile and one, two tiles and one, sixteen tiles and one, a last tensor of one element
RLIST = ([1] * 11 + [0, 255, 256, 0, 0, 257] + [1] * 9 + [513, 4097] + [1] * 10 + [0, 4097, 2500, 513]
         + [1] * 13 + [4097, 0, 1])
RTILES = sum((n + 255) // 256 for n in RLIST)
EDGE_YS = [0, 1, (1 << 64) - 1, 1 << 520, P - 1]
# (id, xs, DN_RECON_UNROLL, the descriptor's (k, a_limbs, has_inv, shift))
RFORMS = [("135", [1, 3, 5], None, (3, 1, 0, 3)),  # unrolled K = 3, no divisor
          ("245", [2, 4, 5], None, (3, 1, 2, 0)),  # unrolled K = 3, a small odd divisor
          ("k5", [2, 3, 5, 8, 9], None, (5, 1, 2, 0)),  # unrolled K = 5
          ("runtime-k", [1, 3, 5], "0", (3, 1, 0, 3)),  # the runtime-k kernel on one-limb weights
          ("full-width", [88159051, 658814259, 702745590], None, (3, 17, 0, 0))]  # (of test_gpu_resolve_many.FORMS)


def effective_schedule(cap: int, mode: int) -> int:
    """The wave schedule dn_m521_reconstruct_many launches with under
    DN_GRID_CAP=cap, DN_TILE_MAP=mode (csrc/shamir_m521.hip grid_for,
    tile_map_for): schedule 1 needs a grid that is a multiple of 8."""
    grid = min(cap, (RTILES + 3) // 4)
    return 0 if mode == 1 and grid % 8 else mode


def test_stride_list_and_knob_fallbacks():
    assert RTILES == 115 and RTILES >= 100 and RLIST[-1] == 1 and RLIST.count(0) == 5
    assert {255, 256, 257, 513, 4097} <= set(RLIST)
    runs, run = [], 0
    for n in RLIST + [0]:
        if n == 1:
            run += 1
        elif run:
            runs.append(run)
            run = 0
    assert runs == [11, 9, 10, 13, 1]
    # which (cap, schedule) pairs run as asked: all but schedule 1 at caps 1, 2 and 3, which run schedule 0
    assert [(c, m) for c in (1, 2, 3, 8) for m in range(4) if effective_schedule(c, m) != m] == [(1, 1), (2, 1), (3, 1)]
    # every wave of every grid takes at least three tiles, so the cursor steps in every wave
    assert RTILES // (4 * 8) >= 3


# results a solved row steers every third element to: both sides of 2^63 and of 2^64 (an int64 secret's
# two's-complement view is below 2^64 whatever its sign; what is counted is a result at or above 2^64)
OUT_TARGETS = [0, 1, (1 << 63) - 1, 1 << 63, (1 << 64) - 1, 1 << 64, (1 << 64) + 1, P - 1]


@functools.lru_cache(maxsize=None)
def _resolve_rows(xs: tuple):
    rng = random.Random(20251)
    lam = fe.lagrange_at_zero(xs)
    k = len(xs)
    last_inv = pow(lam[k - 1], -1, P)
    ints, blocks, e_all = [], [], 0
    for j, n in enumerate(RLIST):
        rows = [[rng.randint(0, P - 1) for _ in range(n)] for _ in range(k)]
        for e in range(1, n - 1):
            e_all += 1
            if e_all % 3 == 0:
                part = sum(lam[i] * rows[i][e] for i in range(k - 1))
                rows[k - 1][e] = (OUT_TARGETS[(e_all // 3) % len(OUT_TARGETS)] - part) * last_inv % P
        if n:
            for i in range(k):
                rows[i][0] = EDGE_YS[(i + j) % 5]
                rows[i][n - 1] = EDGE_YS[(i + 2 * j + 1) % 5]
        ints.append(rows)
        host = np.stack([field.ints_to_vec(r) for r in rows]) if n else np.zeros((k, 0), dtype=np.uint8)
        blocks.append(torch.from_numpy(host).to(dev()))
    return ints, blocks


def resolve_rows(form: str):
    """Per tensor the k share rows of weight form `form` (never written):
    random field elements — inconsistent shares, Lagrange at zero is linear —
    with the edge values in the first and last live word of every tensor
    (rotating through rows and values) and, at every third element between,
    the last row solved so that the result is one of OUT_TARGETS.
    Returns (Python ints [tensor][row][element], device blocks [k, vb])."""
    return _resolve_rows(tuple([f for f in RFORMS if f[0] == form][0][1]))


@functools.lru_cache(maxsize=None)
def resolve_expected(form: str):
    """Per tensor the Python-integer results of weight form `form`."""
    xs = [f for f in RFORMS if f[0] == form][0][1]
    ints, _ = resolve_rows(form)
    return [le.lagrange_reference(rows, xs) if n else [] for rows, n in zip(ints, RLIST)]


def guarded_outputs(out: str):
    sizes = [8 * n if out == "int64" else field.vec_bytes(n) for n in RLIST]
    buf = torch.full((GUARD + sum(s + GUARD for s in sizes),), CANARY, dtype=torch.uint8, device=dev())
    outs, spans, off = [], [], GUARD
    for s in sizes:
        o = buf[off:off + s]
        outs.append(o.view(torch.int64) if out == "int64" else o)
        spans.append((off, off + s))
        off += s + GUARD
    return buf, outs, spans


@pytest.mark.parametrize("mode", [0, 1, 2, 3], ids=["cyclic", "xcd", "blocked", "coop"])
@pytest.mark.parametrize("cap", [1, 2, 3, 8])
def test_resolve_many_under_grid_caps_and_schedules(cap, mode, monkeypatch):
    """The tuning build with 4, 8, 12 and 32 waves over 115 tiles: every wave
    takes several tiles, the forward cursor crosses up to 32 table entries in
    one step.  Schedule 1 is real only at cap 8 (effective_schedule)."""
    monkeypatch.setenv("DN_GRID_CAP", str(cap))
    monkeypatch.setenv("DN_TILE_MAP", str(mode))
    monkeypatch.setattr(shamir_mod, "_resolve_vectors", _not_the_loop)
    ss = shamir.SecretShare(2)
    for form, xs, unroll, desc in RFORMS:
        w = _native.lagrange(xs, 2)
        assert (w.k, w.a_limbs, w.has_inv, w.shift) == desc, form  # the coverage is stated, not assumed
        _, blocks = resolve_rows(form)
        before = [b.clone() for b in blocks]
        want = resolve_expected(form)
        # the rule of include/dn_shamir.h and of the existing tests: a result at or above 2^64 counts (2^63 ..
        # 2^64 - 1 are the negative int64 secrets); the targets put results on both sides of both powers
        want_over = [sum(v >> 64 != 0 for v in wj) for wj in want]
        assert all(0 < c < n for c, n in zip(want_over, RLIST) if n > 64) and len(set(want_over)) > 5
        assert any(1 << 63 <= v < 1 << 64 for wj in want for v in wj)
        shares = [list(b.unbind(0)) for b in blocks]
        for out in ("int64", "field"):
            buf, outs, spans = guarded_outputs(out)
            with monkeypatch.context() as m:
                if unroll is not None:
                    m.setenv("DN_RECON_UNROLL", unroll)
                with _native.library(_native.TUNING_LIB):
                    got, over = ss.resolve_shares_vec_many(shares, xs, RLIST, out=out, outs=outs, return_overflow=True)
            assert all(g is o for g, o in zip(got, outs))
            host = buf.cpu().numpy().copy()
            for j, ((a, b), n) in enumerate(zip(spans, RLIST)):
                if out == "int64":
                    have = host[a:b].view("<i8").tolist()
                    assert have == [fe.to_i64(v & fe.M64) for v in want[j]], (form, out, j, n)
                    host[a:b] = CANARY
                elif n:
                    assert field.vec_to_ints(host[a:b], n) == want[j], (form, out, j, n)
                    host[a:b][live_mask(n)] = CANARY  # (lanes past n_j of a last tile are not written)
            assert (host == CANARY).all(), (form, out)
            assert over.dtype == torch.int32 and over.tolist() == want_over, (form, out)
        for b0, b1 in zip(before, blocks):
            assert torch.equal(b0, b1), form


@functools.lru_cache(maxsize=None)
def live_mask(n: int) -> np.ndarray:
    """bool [vec_bytes(n)]: the bytes of a tiled vector that belong to its n elements."""
    nt = (n + 255) // 256
    m = np.zeros((nt, 66 * 256), dtype=bool)
    live = (np.arange(nt * 256) < n).reshape(nt, 256)
    m[:, :16 * 1024].reshape(nt, 16, 256, 4)[:] = live[:, None, :, None]
    m[:, 16 * 1024:].reshape(nt, 256, 2)[:] = live[:, :, None]
    return m.reshape(-1)


# ------------------------------------------------------------ e. round trip on ONES
def test_round_trip_over_the_one_element_groups(monkeypatch):
    """ONES at 3-of-5: split, then (1) the wires of shares 1, 3, 5 in one pass,
    each equal to encode_share_vec per (tensor, row) concatenated, and
    reconstructed straight from the records; (2) rows 2, 4, 5 of the same
    blocks through the one-launch reconstruct.  Both give the secrets."""
    t, n = 3, 5
    ss, blocks, views = run_split_list("ONES", t, n, 0)
    sizes = [v.numel() for v in views]
    n_total = sum(sizes)
    sec = torch.cat(views)
    xs = [1, 3, 5]
    wires = codec.encode_shares_many(blocks, sizes, xs)
    assert len(wires) == 3
    for x, (packed, offsets) in zip(xs, wires):
        parts, offs, base = [], [torch.zeros(1, dtype=torch.int64, device=dev())], 0
        for blk, k in zip(blocks, sizes):
            if k:
                p, o = codec.encode_share_vec(blk[x - 1], k, x)
                parts.append(p)
                offs.append(o[1:] + base)
                base += p.numel()
        assert tuple(offsets.shape) == (n_total + 1,) and torch.equal(offsets, torch.cat(offs)), x
        assert torch.equal(packed, torch.cat(parts)), x
    monkeypatch.setattr(shamir_mod, "_resolve_vectors", _not_the_loop)
    got, over = ss.resolve_records_vec(wires, xs, n_total, return_overflow=True)
    assert torch.equal(got, sec) and int(over.item()) == 0
    ys = [2, 4, 5]
    got, over = ss.resolve_shares_vec_many([[b[y - 1] for y in ys] for b in blocks], ys, sizes, return_overflow=True)
    assert len(got) == len(sizes) and torch.equal(torch.cat(got), sec)
    assert over.tolist() == [0] * len(sizes)
