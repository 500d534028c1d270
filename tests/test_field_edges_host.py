"""The edge-input helper (tests/field_edges.py) checked without a GPU: its
expected values against the reference restatement, its hand-built Lagrange
descriptors against the library's, the host byte API on the edge pool, and
the conditions the GPU file's inputs must meet (so that a change to the
helper cannot quietly stop the GPU tests from reaching the rare branches).
"""
import random

import pytest

import field_edges as fe
from delta_node.crypto.shamir import _native
from field_edges import P
from oracle import py_shamir


def _int_bytes(v: int) -> bytes:
    return v.to_bytes((v.bit_length() + 7) // 8, "big")


# ------------------------------------------------------------ the pool itself
def test_pool_holds_the_listed_values():
    pool = fe.edge_values()
    assert len(pool) == len(set(pool)) and all(0 <= v < (1 << 521) for v in pool)
    s = set(pool)
    assert {0, 1, 2, P, P - 1, P - 2, 1 << 520, (1 << 520) - 1, (1 << 520) + 1} <= s
    for k in [31, 32, 33, 63, 64, 65, 255, 256, 257, 479, 480, 481, 511, 512, 513, 520]:
        assert {(1 << k) - 1, 1 << k, (1 << k) + 1, P - (1 << k), P - (1 << k) - 1, P - (1 << k) + 1} <= s, k
    ones = [(0x1FF if j == 16 else fe.M32) << (32 * j) for j in range(17)]
    for j in range(17):
        assert ones[j] in s and (P ^ ones[j]) in s and sum(ones[:j + 1]) in s, j
    assert sum(ones[0::2]) in s and sum(ones[1::2]) in s


def test_layout_kinds():
    kinds = fe.layout_kinds()
    assert len(kinds) == fe.N_LAYOUT == 4 * 256 + 37
    assert set(kinds[:256]) == {"E"} and set(kinds[512:768]) == {"R"} and set(kinds[1024:]) == {"E"}
    for q in range(4):  # tile 1: exactly one edge element per 64-lane quarter
        quarter = kinds[256 + 64 * q:256 + 64 * (q + 1)]
        assert quarter.count("L") == 1 and quarter.count("R") == 63
    assert [kinds[256 + w] for w in (0, 127)] == ["L", "L"]  # lane 0 and lane 63 of their quarters
    assert {"E", "R"} == set(kinds[768:1024])
    vals = fe.layout_values()
    pool = set(fe.edge_values())
    assert all((v in pool) == (k != "R") for v, k in zip(vals, kinds))


# ------------------------------------------------------------ expected helpers vs the reference restatement
@pytest.mark.parametrize("t,n", [(2, 3), (3, 5), (5, 9)])
def test_split_expected_equals_reference_eval_at(t, n):
    case = fe.split_case(t, n, fe=True)
    for i in range(0, case.N, 7):
        for x in (1, 2, n):
            assert fe.split_expected(case.rows[i], x) == py_shamir.eval_at(case.rows[i], x), (i, x)


@pytest.mark.parametrize("xs", [[1, 2, 3], [1, 3, 5], [2, 4, 5], [1, 2, 4, 5], [2, 3, 5, 8, 9], [7, 100, 255],
                                [1, 256, 1000]])
def test_recon_expected_equals_reference_resolve_shares(xs):
    k = len(xs)
    a, neg, d, shift = fe.desc_parts(fe.desc_from_xs(xs))
    if xs == [1, 3, 5]:
        assert shift > 0
    if xs in ([2, 4, 5], [7, 100, 255], [1, 256, 1000]):
        assert d > 1
    ys = [fe.layout_values(fe.N_LAYOUT, 40 + i, 50 * i) for i in range(k)]
    lams = fe.lagrange_at_zero(xs)
    ref = py_shamir.RefSecretShare(k)
    for e in range(0, fe.N_LAYOUT, 11):
        y = [ys[i][e] for i in range(k)]
        want = int.from_bytes(ref.resolve_shares([py_shamir.share_to_bytes(xs[i], y[i]) for i in range(k)]), "big")
        assert fe.recon_expected(y, a, neg, d, shift) == want, e
        assert sum(l * v for l, v in zip(lams, y)) % P == want, e


# ------------------------------------------------------------ crafted descriptors vs the library
def test_crafted_descriptors_equal_the_librarys():
    seen = set()
    for xs in [[1, 2, 3], [2, 3], [1, 3, 5], [2, 4, 5], [1, 2, 4, 5], [2, 3, 5, 8, 9], [7, 100, 255], [1, 256, 1000],
               [17, 33, 65, 129, 200, 250], [3, 2**20 + 1, 2**21], [1, 65537, 131075], [1, 65537],
               [2**33, 2**33 + 1], [1, 2**32 + 1], list(range(1, 17))]:
        lib = _native.lagrange(xs, len(xs))
        assert lib.a_limbs in (1, 2), xs
        assert fe.desc_fields(fe.desc_from_xs(xs)) == fe.desc_fields(lib), xs
        seen.add((lib.a_limbs, lib.has_inv))
    assert seen == {(A, inv) for A in (1, 2) for inv in (0, 1, 2)}


def test_fd_needs_fold_restatement():
    # the restated bound: sum_{j<t} (n + t)^j < 2^23, in exact integers (the
    # doubles are exact far beyond 2^23 at these sizes)
    for t in range(1, 9):
        for n in [t, t + 1, 17, 18, 48, 49, 198, 199, 2892, 2893, 65535]:
            if n >= t:
                assert fe.fd_needs_fold(t, n) == (sum((n + t) ** j for j in range(t)) >= 1 << 23), (t, n)
    assert [fe.fd_max_n(t) for t in (3, 4, 5, 6, 7)] == [2892, 198, 48, 18, 7]
    assert fe.fd_max_n(2) == 65535


def test_fd_needs_fold_is_conservative():
    """Where the unfolded table would truly overflow (fd_overflow_n) the
    split folds, and the fused draw + split declines the shape; the stated
    bound leaves only a few share counts of slack below that point."""
    L = _native.lib()
    for t in range(3, 8):
        n = fe.fd_overflow_n(t)
        assert fe.split_unreduced([0] + [P - 1] * (t - 1), n) >= 1 << 544
        assert fe.split_unreduced([fe.M64] + [P] * (t - 1), n - 1) < 1 << 544
        assert fe.fd_max_n(t) < n <= fe.fd_max_n(t) + 8, (t, n)
        assert all(fe.fd_needs_fold(t, m) for m in range(fe.fd_max_n(t) + 1, n + 1))
    assert [fe.fd_overflow_n(t) for t in (3, 4, 5)] == [2896, 203, 54]
    for t in (2, 3, 5):
        n = fe.fd_max_n(t)
        assert L.dn_mt19937_split_supported(300, t, n) == 1
        if n < 65535:
            assert L.dn_mt19937_split_supported(300, t, n + 1) == 0
            assert L.dn_mt19937_split_supported(300, t, fe.fd_overflow_n(t)) == 0


# ------------------------------------------------------------ the host byte API on the pool
@pytest.mark.parametrize("t,n", [(1, 2), (2, 3), (3, 5), (5, 9), (9, 12)])
def test_host_make_shares_and_eval_at_on_pool(t, n):
    case = fe.split_case(t, n, fe=True)
    for i in list(range(0, 256, 5)) + list(range(256, case.N, 3)):
        row = case.rows[i]
        recs = _native.host_make_shares(_int_bytes(row[0]), row[1:], P, t, n)
        got = [py_shamir.parse_share(r) for r in recs]
        assert got == [(x, fe.split_expected(row, x)) for x in range(1, n + 1)], i
        for x in (1, n, 65535, P - 1, P, P + 1):
            assert _native.host_eval_at(row, x, P) == fe.split_expected(row, x % P if x >= P else x), (i, x)


@pytest.mark.parametrize("xs", [[1, 3, 5], [2, 4, 5], [1, 2, 4, 5], [2, 3, 5, 8, 9], [7, 100, 255], [2, 3]])
def test_host_resolve_shares_on_pool(xs):
    k = len(xs)
    lams = fe.lagrange_at_zero(xs)
    ys = [fe.layout_values(fe.N_LAYOUT, 60 + i, 91 * i + k) for i in range(k)]
    # the last share solved: results at the output edges, 0 from a non-zero multiple of p included
    targets = [0, 1, fe.M64, 1 << 64, (1 << 64) + 1, P - 1]
    linv = pow(lams[-1], -1, P)
    for e in range(0, fe.N_LAYOUT, 3):
        y = [ys[i][e] % P for i in range(k)]
        if e % 2:
            part = sum(l * v for l, v in zip(lams[:-1], y[:-1]))
            y[-1] = (targets[(e // 2) % len(targets)] - part) * linv % P
        want = sum(l * v for l, v in zip(lams, y)) % P
        got = _native.host_resolve_shares([py_shamir.share_to_bytes(xs[i], y[i]) for i in range(k)], k, P)
        assert got == _int_bytes(want), e


# ------------------------------------------------------------ conditions on the GPU file's inputs
def _check_census(case, lone: bool):
    census = fe.predicate_census(case)
    for name, c in census.items():
        assert c["count"] >= 8, (name, c)
        assert c["full"] and c["partial"], (name, c)
        if lone:
            assert c["lone"], (name, c)


@pytest.mark.parametrize("t,n", [s for s in fe.SPLIT_U64_SHAPES + fe.SPLIT_HORNER_SHAPES if s[0] >= 2])
def test_every_predicate_occurs_u64(t, n):
    """(t = 1 is left out by reasoning: F is the 64-bit secret itself, so
    nothing folds, carries or reaches p.)"""
    case = fe.split_case(t, n)
    assert all(0 <= r[0] <= fe.M64 and all(0 <= c < (1 << 521) for c in r) for r in case.rows)
    _check_census(case, lone=True)


@pytest.mark.parametrize("t,n", fe.SPLIT_FE_SHAPES)
def test_every_predicate_occurs_field_secret(t, n):
    case = fe.split_case(t, n, fe=True)
    assert all(0 <= c < (1 << 521) for r in case.rows for c in r)
    assert P in case.secrets()
    _check_census(case, lone=True)


@pytest.mark.parametrize("t", [3, 4, 5, 6, 7])
@pytest.mark.parametrize("over", [0, 1])
def test_every_predicate_occurs_at_the_forward_difference_bound(t, over):
    """The bound shapes run on N = 300: one full tile of edges and a partial
    one (no lone lanes there: those are covered by the N = 1061 shapes)."""
    _check_census(fe.SplitCase(t, fe.fd_max_n(t) + over, 300), lone=False)


def test_forward_difference_table_reaches_its_bound():
    """With every coefficient p - 1 the largest entry the difference table
    ever holds needs all 544 bits at the last shape that does not fold (t = 3,
    4, 5): the shapes of the GPU bound test sit exactly at the bound."""
    for t, top in [(3, 544), (4, 544), (5, 544), (6, None), (7, None)]:
        n = fe.fd_max_n(t)
        f = [fe.split_unreduced([P - 1] * t, x) for x in range(1, n + t)]
        D, peak = f[:t], 0
        for k in range(1, t):  # the table at x = 1: D[k] = Delta^k f(1)
            for j in range(t - 1, k - 1, -1):
                D[j] = D[j] - D[j - 1]
        for _ in range(n):
            peak = max(peak, max(D))
            for k in range(t - 1):
                D[k] += D[k + 1]
        assert peak.bit_length() <= 544
        assert top is None or peak.bit_length() == top, (t, n, peak.bit_length())


@pytest.mark.parametrize("t,n,least", [(2, 3, 0.25), (3, 5, 0.50), (5, 9, 0.50)])
def test_steered_secrets_carry_past_limb_one(t, n, least):
    N = 2000
    vb = _native.vec_bytes(N)
    from delta_node.crypto.shamir import field

    co = _native.mt_draw_coeffs(random.Random(7), N, t - 1)
    assert co.shape == (t - 1, vb)
    cols = [field.vec_to_ints(co[j], N) for j in range(t - 1)]
    rows = [[c[e] for c in cols] for e in range(N)]
    sec = fe.steer_secrets(rows, n)
    for e in range(0, N, 97):
        assert fe.split_unreduced([sec[e]] + rows[e], 1 + e % n) & fe.M64 == fe.M64
    share = fe.steered_multi_share(rows, sec, n)
    print(f"steered (t, n) = ({t}, {n}): multi-limb carry at the target share for {100 * share:.1f} %")
    assert share >= least


def test_recon_cases_cover_what_they_claim():
    cases = fe.recon_cases()
    names = [c[0] for c in cases]
    assert len(names) == len(set(names))
    assert {(c[1], c[2]) for c in cases} == {(A, inv) for A in (1, 2, 17) for inv in (0, 1, 2)}
    assert {c[3] for c in cases if c[1] == 1} >= {2, 3, 4, 5, 6, 16}
    assert {c[4] for c in cases if c[2] == 2} >= set(fe.INV2_DIVISORS)
    assert {c[4] for c in cases if c[2] == 1} >= set(fe.INV1_DIVISORS)
    assert {c[5] for c in cases if c[1] == 1 and c[2] == 0} >= set(range(1, 32))
    for inv in (1, 2):
        assert {c[5] for c in cases if c[2] == inv} >= {1, 9, 10, 31}
    many = fe.recon_many_specs()
    assert {(c[1], c[2]) for c in many} == {(A, inv) for A in (1, 2, 17) for inv in (0, 1, 2)}
    assert {c[3] for c in many if c[1] == 1} >= {2, 3, 4, 5, 6, 16}
    assert 3 * len(many) >= len(cases) - 3 * len(many)  # about a third
    # the solved last share makes the residue before the division the chosen r*
    for spec in (cases[0], [c for c in cases if c[0] == "inv2-d65521"][0], [c for c in cases if c[0] == "shift9"][0]):
        case = fe.recon_case_of(spec)
        rs, kinds = fe.rstar_values(case.d, case.shift), fe.layout_kinds(case.N)
        e = 0
        for i in range(case.N):
            if kinds[i] == "R":
                continue
            ys = [case.ys[j][i] for j in range(case.k)]
            assert fe.recon_expected(ys, case.a, case.neg) == rs[e % len(rs)], (spec[0], i)
            e += 1
        low = [r for r in rs if r & ((1 << max(case.shift, 1)) - 1) == (1 << max(case.shift, 1)) - 1]
        assert len(low) >= 8
