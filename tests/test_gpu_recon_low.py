"""The five-limb reconstruct (MI355X): dn_m521_reconstruct and
dn_m521_reconstruct_many asked for the int64 words alone read limbs 0, 1, 2,
15 and hi of every share row (reconstruct_low_kernel, csrc/shamir_m521.hip).

The words must equal the full path's — the same call with an overflow
counter, which keeps every limb, and the tuning build under DN_RECON_LOW=0 —
at every size around a quarter and a tile, for K = 2..5 with and without the
division by 2^e, under every wave schedule; the five-limb path must really be
the one taken (planes 3..14 do not matter); nothing outside the n outputs is
written and no lane at or past n is needed.  Integer arithmetic: every
comparison is bit-exact.  The rows are random field elements (no sharing):
per element the two paths may differ with probability (A + 2) / 2^41
(DESIGN.md §4.2), and the seeds are fixed.
"""
import random

import numpy as np
import pytest
import torch

from delta_node.crypto import shamir
from delta_node.crypto.shamir import _native, field

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 769, 3077]
# K -> (xs with e = 0, xs with e = 3): one-limb weights, d = 1
XS = {2: ([1, 2], [1, 9]), 3: ([1, 2, 3], [1, 3, 5]), 4: ([1, 2, 3, 4], [1, 4, 5, 9]),
      5: ([1, 2, 3, 4, 5], [1, 2, 3, 5, 7])}
CANARY = 0x5A5A5A5A5A5A5A5A
GUARD = 64  # int64 words before and after the output


def dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _native.lib()


def live_mask(n: int) -> np.ndarray:
    """bool [vec_bytes(n)]: the bytes of a tiled vector that belong to its n elements."""
    nt = (n + 255) // 256
    m = np.zeros((nt, 66 * 256), dtype=bool)
    live = (np.arange(nt * 256) < n).reshape(nt, 256)
    m[:, :16 * 1024].reshape(nt, 16, 256, 4)[:] = live[:, None, :, None]
    m[:, 16 * 1024:].reshape(nt, 256, 2)[:] = live[:, :, None]
    return m.reshape(-1)


def middle_mask(n: int) -> np.ndarray:
    """bool [vec_bytes(n)]: limb planes 3..14 of every tile."""
    nt = (n + 255) // 256
    m = np.zeros((nt, 66 * 256), dtype=bool)
    m[:, 3 * 1024:15 * 1024] = True
    return m.reshape(-1)


_ROWS = {}


def host_rows(n: int) -> np.ndarray:
    """uint8 [5, vec_bytes(n)]: five rows of n random field elements in
    [1, p - 1]; the lanes past n of the last tile hold 0xFF (not a field
    element: the hi plane has bits 9..15 set there)."""
    if n not in _ROWS:
        ys = np.ascontiguousarray(_native.mt_draw_coeffs(random.Random(7000 + n), n, 5)).reshape(5, field.vec_bytes(n))
        ys = ys.copy()
        ys[:, ~live_mask(n)] = 0xFF
        _ROWS[n] = ys
    return _ROWS[n]


def rows_on_device(n: int, k: int, host=None):
    block = torch.from_numpy(host_rows(n) if host is None else host).to(dev())
    return [block[i] for i in range(k)]


def guarded(n: int):
    buf = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.int64, device=dev())
    return buf, buf[GUARD:GUARD + n]


def assert_guards(buf, n):
    assert bool((buf[:GUARD] == CANARY).all()) and bool((buf[GUARD + n:] == CANARY).all()), n


def low(rows, w, n):
    """The int64-only call: (words, the guarded buffer)."""
    buf, rec = guarded(n)
    _native.reconstruct(rows, w, out_u64=rec, n=n)
    return rec, buf


def full(rows, w, n):
    """The same call with a counter (every limb is read): (words, count)."""
    buf, rec = guarded(n)
    over = torch.zeros(1, dtype=torch.int32, device=dev())
    _native.reconstruct(rows, w, out_u64=rec, overflow=over, n=n)
    assert_guards(buf, n)
    return rec, int(over.item())


def weights(k, e):
    xs = XS[k][1 if e else 0]
    w = _native.lagrange(xs, 2)
    assert (w.k, w.a_limbs, w.has_inv, w.shift) == (k, 1, 0, e)  # the coverage is stated, not assumed
    return w


# ------------------------------------------------------------ 1. equals the full path
@pytest.mark.parametrize("k,e", [(k, e) for k in (2, 3, 4, 5) for e in (0, 3)])
def test_words_equal_the_full_path(k, e, monkeypatch):
    """Product library: int64 alone against the call with a counter; tuning
    build: the same against DN_RECON_LOW=0.  Poisoned lanes past n, canaries
    around the output."""
    w = weights(k, e)
    for n in SIZES:
        rows = rows_on_device(n, k)
        want, count = full(rows, w, n)
        assert count > 0  # random rows: results beyond 64 bits
        got, buf = low(rows, w, n)
        assert_guards(buf, n)
        assert torch.equal(got, want), (k, e, n)
        with _native.library(_native.TUNING_LIB):
            tuned, buf = low(rows, w, n)
            assert_guards(buf, n)
            monkeypatch.setenv("DN_RECON_LOW", "0")
            off, buf = low(rows, w, n)
            assert_guards(buf, n)
            monkeypatch.delenv("DN_RECON_LOW")
        assert torch.equal(tuned, want) and torch.equal(off, want), (k, e, n)


@pytest.mark.parametrize("cap", [1, 2])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_wave_schedules(cap, mode, monkeypatch):
    """DN_GRID_CAP = 1, 2 (4 and 8 waves over 13 and 4 tiles: several passes
    per wave, the partial tile last) under DN_TILE_MAP = 0..3 (3: each wave a
    quarter of its workgroup's tile)."""
    for k, e, n in [(3, 3, 3077), (5, 0, 3077), (2, 3, 769), (4, 0, 255)]:
        w = weights(k, e)
        rows = rows_on_device(n, k)
        want, _ = full(rows, w, n)
        monkeypatch.setenv("DN_GRID_CAP", str(cap))
        monkeypatch.setenv("DN_TILE_MAP", str(mode))
        with _native.library(_native.TUNING_LIB):
            got, buf = low(rows, w, n)
        monkeypatch.delenv("DN_GRID_CAP")
        monkeypatch.delenv("DN_TILE_MAP")
        assert_guards(buf, n)
        assert torch.equal(got, want), (k, e, n, cap, mode)


# ------------------------------------------------------------ 2. the path is really taken
@pytest.mark.parametrize("k,e", [(3, 3), (5, 0)])
def test_planes_3_to_14_are_not_read(k, e):
    """A 3-of-5 sharing of int64 secrets, and the same rows with planes 3..14
    overwritten by garbage: the int64-only words are the secrets both times.
    With a counter (the full path) the clean rows give the same words and no
    overflow, the garbage rows an overflow in every element — there the
    garbage is read."""
    n = 3077
    w = weights(k, e)
    g = torch.Generator().manual_seed(k)
    sec = torch.randint(-2 ** 63, 2 ** 63 - 1, (n,), dtype=torch.int64, generator=g)
    ss = shamir.SecretShare(3)
    ss.random.seed(k)
    block = ss.make_shares_vec(sec, 9)
    clean = np.stack([block[x - 1].cpu().numpy() for x in XS[k][1 if e else 0]])
    dirty = clean.copy()
    noise = np.random.default_rng(314).integers(0, 256, size=dirty.shape, dtype=np.uint8)
    mid = middle_mask(n)
    dirty[:, mid] = noise[:, mid]
    a, _ = low(rows_on_device(n, k, clean), w, n)
    b, _ = low(rows_on_device(n, k, dirty), w, n)
    assert torch.equal(a.cpu(), sec) and torch.equal(b, a)
    fa, clean_count = full(rows_on_device(n, k, clean), w, n)
    fb, dirty_count = full(rows_on_device(n, k, dirty), w, n)
    # (fb's words are not compared: garbage subtracted from a small result
    # wraps to within A 2^480 of p, the sliver outside the contract)
    assert torch.equal(fa, a) and fb.shape == a.shape
    assert clean_count == 0 and dirty_count == n


def test_lanes_past_n_are_not_needed():
    """Two poisons in the lanes past n (0xFF and 0x00) and in the output's
    surroundings: the n words are the same and nothing else is written."""
    for n in (1, 65, 257, 3077):
        w = weights(3, 3)
        zeros = host_rows(n).copy()
        zeros[:, ~live_mask(n)] = 0
        a, bufa = low(rows_on_device(n, 3), w, n)
        b, bufb = low(rows_on_device(n, 3, zeros), w, n)
        assert_guards(bufa, n)
        assert_guards(bufb, n)
        assert torch.equal(a, b), n


# ------------------------------------------------------------ 3. the tensor list
SEGS = [1, 255, 256, 257, 1000]


@pytest.fixture(scope="module")
def split_list():
    """(secrets, share blocks) of make_shares_vec_many over SEGS at 3-of-5."""
    g = torch.Generator().manual_seed(99)
    secs = [torch.randint(-2 ** 63, 2 ** 63 - 1, (n,), dtype=torch.int64, generator=g) for n in SEGS]
    ss = shamir.SecretShare(3)
    ss.random.seed(17)
    blocks = ss.make_shares_vec_many(secs, 5)
    return secs, blocks


def test_resolve_many_equals_the_per_vector_calls_and_the_secrets(split_list):
    secs, blocks = split_list
    ss = shamir.SecretShare(3)
    for xs in ([1, 3, 5], [1, 2, 3], [2, 3, 4, 5], [1, 2, 3, 4, 5]):
        shares = [[b[x - 1] for x in xs] for b in blocks]
        many = ss.resolve_shares_vec_many(shares, xs, SEGS)
        for sh, n, s, m in zip(shares, SEGS, secs, many):
            one = ss.resolve_shares_vec(sh, xs, n)
            assert torch.equal(m, one) and torch.equal(m.cpu(), s), (xs, n)


def test_resolve_many_with_overflow_is_the_full_path(split_list):
    """return_overflow=True keeps every limb: on rows with garbage in planes
    3..14 the counts are non-zero and equal the per-vector calls', the words
    too; without it the garbage does not show."""
    secs, blocks = split_list
    xs = [1, 3, 5]
    ss = shamir.SecretShare(3)
    dirty = []
    for j, (b, n) in enumerate(zip(blocks, SEGS)):
        h = b.cpu().numpy().copy()
        noise = np.random.default_rng(2000 + j).integers(0, 256, size=h.shape, dtype=np.uint8)
        mid = middle_mask(n) & live_mask(n)
        h[:, mid] = noise[:, mid]
        dirty.append(torch.from_numpy(h).to(dev()))
    shares = [[b[x - 1] for x in xs] for b in dirty]
    many, over = ss.resolve_shares_vec_many(shares, xs, SEGS, return_overflow=True)
    for j, (sh, n) in enumerate(zip(shares, SEGS)):
        one, c = ss.resolve_shares_vec(sh, xs, n, return_overflow=True)
        assert torch.equal(many[j], one) and int(over[j].item()) == int(c.item()) > 0, n
    plain = ss.resolve_shares_vec_many(shares, xs, SEGS)
    for m, s in zip(plain, secs):
        assert torch.equal(m.cpu(), s)


# ------------------------------------------------------------ 4. round trip
@pytest.mark.parametrize("t", [2, 3, 5])
def test_round_trip_through_the_python_api(t):
    n = 1000
    g = torch.Generator().manual_seed(t)
    sec = torch.randint(-2 ** 63, 2 ** 63 - 1, (n,), dtype=torch.int64, generator=g)
    sec[:6] = torch.tensor([0, 1, 2, 3, -1, -2 ** 63])
    ss = shamir.SecretShare(t)
    ss.random.seed(t)
    shares = ss.make_shares_vec(sec, 5)
    xs = [1, 3, 5, 2, 4][:t]
    w = _native.lagrange(xs, t)
    assert (w.a_limbs, w.has_inv) == (1, 0)
    rec = ss.resolve_shares_vec([shares[x - 1] for x in xs], xs, n)
    assert torch.equal(rec.cpu(), sec)
