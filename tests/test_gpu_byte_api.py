"""The byte API's device route: `_eval_at` for GF(2^521 - 1) with
1 <= x <= 65535 and at most 64 coefficients runs the device split
(`_eval_many` -> `dn_m521_split_fe` on one element, x share rows), every other
input the library's host Horner.  Both are compared here with Python integers
and with each other on the same inputs, on the edge pool of
tests/field_edges.py, with negative coefficients and coefficients >= p (which
`_eval_at` reduces first), on both sides of the two limits that switch the
route; and `make_shares` / `resolve_shares` (host) are tied to
`make_shares_vec` / `resolve_shares_vec` (device) at one point.  Every
comparison is exact.

The first run of this module found a defect: with more coefficients than x
(the reference's own `_eval_at(coeffs, 1, prime)` of a t-coefficient
polynomial) the device route raised "threshold should be little equal than
shares", because the split was asked for x rows.  `_eval_many` now computes
max(x, t) rows; every count above 1 at x = 1 and x = 2 pins it.
"""
import random

import pytest
import torch

import field_edges as fe
from delta_node.crypto import shamir
from delta_node.crypto.shamir import _native, field
from delta_node.crypto.shamir.shamir import _eval_at, _eval_many, _share_to_bytes, _to_device_vecs
from field_edges import P

pytestmark = pytest.mark.gpu

ROWS = 16
COUNTS = [1, 2, 3, 5, 8, 9, 64]
XS = [1, 2, 255, 256, 4097]


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _native.lib()


def python_eval_at(cs, x, p=P):
    acc = 0
    for c in reversed(cs):
        acc = (acc * x + c) % p
    return acc


def coefficient_rows(t: int, seed: int = 0):
    """ROWS rows of t coefficients from the edge pool (p itself included);
    in every row but the first a third of the entries are moved outside
    [0, p): negated, or raised by p, 2 p or a multiple of 2^521."""
    rng = random.Random(1000 * t + seed)
    pool = fe.edge_values()
    rows = []
    for r in range(ROWS):
        row = [pool[(r * 23 + j * 7 + rng.randrange(len(pool))) % len(pool)] for j in range(t)]
        if r:
            for j in range(t):
                kind = rng.randrange(12)
                if kind == 0:
                    row[j] = -row[j]
                elif kind == 1:
                    row[j] += P * rng.choice((1, 2, 1 << 64))
                elif kind == 2:
                    row[j] = -(row[j] + (rng.getrandbits(64) << 521))
                elif kind == 3:
                    row[j] = rng.choice((P - 1, P, P + 1, 2 * P, -P, -1, 0))
        rows.append(row)
    rows[1][0], rows[2][-1] = -1, P  # a negative secret; a leading coefficient that reduces to 0
    return rows


def test_rows_hold_what_the_tests_rely_on():
    for t in COUNTS:
        rows = coefficient_rows(t)
        flat = [c for row in rows for c in row]
        assert len(rows) == ROWS and all(len(row) == t for row in rows)
        assert any(c < 0 for c in flat) and any(c >= P for c in flat) and any(0 <= c < P for c in flat)


@pytest.mark.parametrize("t", COUNTS)
def test_eval_at_device_route_equals_python_and_the_host_route(t):
    assert t <= _native.MAX_THRESHOLD
    for x in XS:
        assert 1 <= x <= _native.MAX_SHARES
        for r, row in enumerate(coefficient_rows(t)):
            want = python_eval_at(row, x)
            assert _eval_at(row, x, P) == want, (t, x, r)
            assert _native.host_eval_at(row, x, P) == want, (t, x, r)


@pytest.fixture(scope="module")
def at_the_last_share():
    """The one large case: x = 65535 is the last of 65535 share rows of one
    single-tile vector each (about 1.1 GB of output)."""
    row = [P - 1, -(P - 2)]
    return row, _eval_at(row, _native.MAX_SHARES, P)


def test_eval_at_last_device_abscissa(at_the_last_share):
    row, got = at_the_last_share
    assert _native.MAX_SHARES == 65535
    assert got == python_eval_at(row, 65535) == _native.host_eval_at(row, 65535, P)


def test_eval_at_is_continuous_across_the_route_switch(at_the_last_share):
    row, got = at_the_last_share
    # x = 65535 on the device, x = 65536 on the host: the same polynomial, each its own value
    assert _eval_at(row, 65536, P) == python_eval_at(row, 65536)
    assert (python_eval_at(row, 65536) - got) % P == 2  # f(x) = -1 - (p - 2) x: one step adds 2 mod p
    # 64 coefficients on the device, 65 on the host, at the same x
    rows64 = coefficient_rows(64, seed=1)
    for x in (3, 4097):
        for row in rows64[:4]:
            more = row + [rows64[5][0] or 1]
            assert _eval_at(row, x, P) == python_eval_at(row, x), x
            assert _eval_at(more, x, P) == python_eval_at(more, x), x
            assert _eval_at(row + [0], x, P) == python_eval_at(row, x), x  # a zero on top: the same value by the host
    # x = 0 and a negative x go to the host as well
    assert _eval_at(rows64[1], 0, P) == rows64[1][0] % P
    assert _eval_at(rows64[1][:3], -2, P) == python_eval_at(rows64[1][:3], -2)
    assert _eval_at([], 5, P) == 0


def test_empty_vector_block_and_one_share():
    dev = torch.device("cuda", torch.cuda.current_device())
    empty = _to_device_vecs([], dev)
    assert empty.dtype == torch.uint8 and tuple(empty.shape) == (0, field.vec_bytes(1)) and empty.device == dev
    one = _to_device_vecs([P - 1], dev)
    assert tuple(one.shape) == (1, field.vec_bytes(1)) and field.vec_to_ints(one[0].cpu().numpy(), 1) == [P - 1]
    for row in coefficient_rows(5)[:4] + coefficient_rows(1)[:4]:
        cs = [c % P for c in row]
        assert _eval_many(cs, 1) == [sum(cs) % P]
    cs = [c % P for c in coefficient_rows(3)[3]]
    assert _eval_many(cs, 7) == [python_eval_at(cs, x) for x in range(1, 8)]


def test_byte_shares_equal_the_vector_paths_element():
    """One secret, t = 3, n = 5, the same seed: the host route's records are
    `_share_to_bytes` of element 0 of the device block, and each route
    resolves the other's shares."""
    secret = -0x0123456789ABCDEF
    t, n, seed = 3, 5, 20251
    vec = shamir.SecretShare(t)
    vec.random.seed(seed)
    blk = vec.make_shares_vec(torch.tensor([secret], dtype=torch.int64), n)
    ys = [field.vec_to_ints(blk[x - 1].cpu().numpy(), 1)[0] for x in range(1, n + 1)]
    byte = shamir.SecretShare(t)
    byte.random.seed(seed)
    value = secret.to_bytes(8, "big", signed=True)
    shares = byte.make_shares(value, n)
    assert shares == [_share_to_bytes((x, ys[x - 1])) for x in range(1, n + 1)]
    assert byte.random.getstate() == vec.random.getstate()
    ref = random.Random(seed)
    cs = [int.from_bytes(value, "big")] + [ref.randint(1, P - 1) for _ in range(t - 1)]
    assert ys == [python_eval_at(cs, x) for x in range(1, n + 1)]
    for xs in ([1, 2, 3], [1, 3, 5], [2, 4, 5], [1, 2, 3, 4, 5]):
        assert byte.resolve_shares([shares[x - 1] for x in xs]) == value
        got = vec.resolve_shares_vec([blk[x - 1] for x in xs], xs, 1)
        assert got.cpu().tolist() == [secret]
        # the byte records decoded and handed to the device route
        back = [torch.from_numpy(field.ints_to_vec([shamir.shamir._bytes_to_share(shares[x - 1])[1]])).to(blk.device)
                for x in xs]
        assert vec.resolve_shares_vec(back, xs, 1).cpu().tolist() == [secret]
