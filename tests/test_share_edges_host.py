"""The share check family's arithmetic (csrc/check_core.hpp, csrc/robust_core.hpp) where the older sets never
take it: divisor shifts of 10 and more (robust_rotr's split wrap-around, robust_divide's 31-bit steps), weights
and Lagrange magnitudes next to 2^32, every r at even and odd k, k = 2 and 3, and rows made for the
accumulators and for the residue in front of the final division (share_check_cases.edge_rows,
share_robust_cases.edge_rows).  The stand-alone programs of tests/host/, built plainly and under ASan + UBSan,
against the definition in Python integers; each set's property is asserted from the project's own plan, so
that another set cannot quietly empty the test."""
import math
from fractions import Fraction

import pytest

import host_program
import share_check_cases as cases
import share_robust_cases as robust
from delta_node.crypto.shamir import _native

P = cases.P
ONE_SPARE = "one spare share detects only"
ODD_PART = "a divisor with an odd part of 2^16 or more"  # (not the |A| < 2^32 bound, which comes first in the planner)


@pytest.fixture(scope="module", params=[[], host_program.SANITIZE], ids=["plain", "sanitized"])
def programs(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("share_edges")
    return {name: host_program.compile_program(tmp, name, request.param)
            for name in ("check_core_check", "robust_core_check")}


def check_facts(t, xs):
    """(k, r, largest c, largest xp) of the plan the project builds."""
    plan = _native.check_plan(xs, t)
    cells = [(j, i) for j in range(plan.r) for i in range(plan.k)]
    assert plan.neg == sum(1 << i for i, s in enumerate(cases.negated(xs)) if s)
    return plan.k, plan.r, max(plan.c[j][i] for j, i in cells), max(plan.xp[j][i] for j, i in cells)


def run_check(programs, t, xs, rows):
    """The check program's verdicts: (culprit byte, byte of the form without culprit) per row."""
    return [tuple(map(int, line.split())) for line in programs["check_core_check"](host_program.share_lines(t, xs, rows))]


# What makes each robust set worth having, as a predicate over (k, r, largest c, largest xp, negate,
# largest |A|, the k + 1 (odd part, shift) pairs, D_all's last).
ROBUST_PROPERTY = {
    (2, (1, 2, 5, 17)): lambda k, r, c, xp, neg, a, div: (
        (k, r, neg) == (4, 2, 1) and [e for _, e in div] == [5, 11, 7, 5, 5] and any(10 <= e <= 31 for _, e in div)
        and (min(d for d, _ in div), max(d for d, _ in div)) == (9, 405)),
    (2, (1, 17, 33, 129, 257)): lambda k, r, c, xp, neg, a, div: (
        [e for _, e in div] == [24, 32, 29, 25, 24, 24] and any(10 <= e <= 31 for _, e in div)
        and any(e > 31 for _, e in div) and (min(d for d, _ in div), max(d for d, _ in div)) == (35, 3675)
        and a >= 1 << 29),
    (2, tuple(8191 * i for i in range(1, 6))): lambda k, r, c, xp, neg, a, div: (
        r == 3 and c == 4293918784 and 1 << 31 <= c < 1 << 32 and xp == 40955 ** 2),
    (3, (360, 361, 362, 363, 364)): lambda k, r, c, xp, neg, a, div: a == 4292968680 and 1 << 31 <= a < 1 << 32,
    (2, (1, 2, 3, 8)): lambda k, r, c, xp, neg, a, div: (
        (k, r, neg) == (4, 2, 1) and all(e == 0 for _, e in div)
        and (min(d for d, _ in div), max(d for d, _ in div)) == (35, 1225)),
    (3, (1, 2, 3, 4, 5, 6)): lambda k, r, c, xp, neg, a, div: (k, r, neg) == (6, 3, 1),
    (1, (1, 2, 3)): lambda k, r, c, xp, neg, a, div: (k, r, neg) == (3, 2, 0),
}

# (k, r) of each check-only set, whether its largest c is at least 2^31, and the robust planner's refusal
CHECK_PROPERTY = {
    (1, (1, 2)): (2, 1, False, ONE_SPARE),
    (5, (10, 11, 24, 29, 47, 95)): (6, 1, True, ONE_SPARE),
    (4, (9, 37, 46, 57, 79, 88)): (6, 2, True, ODD_PART),
    (1, (158, 208, 231, 245)): (4, 3, True, ODD_PART),
    (12, (2, 3, 5, 7, 8, 9, 10, 11, 13, 14, 15, 16, 17, 18, 19, 20)): (16, 4, True, ODD_PART),
}


def test_every_set_has_a_property():
    assert set(robust.ROBUST_EDGE) == set(ROBUST_PROPERTY) and set(cases.EDGE) == set(CHECK_PROPERTY)
    assert len(robust.ROBUST_EDGE) == len(ROBUST_PROPERTY) and len(cases.EDGE) == len(CHECK_PROPERTY)


@pytest.mark.parametrize("t, xs", robust.ROBUST_EDGE)
def test_robust_sets(programs, t, xs):
    k, r, c_max, xp_max = check_facts(t, xs)
    edge, marks = robust.edge_rows(t, xs)
    rows = edge + robust.rows(t, xs)
    out = programs["robust_core_check"](host_program.share_lines(t, xs, rows))

    # the plan, line by line against exact rationals (never against the plan's own fields), and the set's property
    chk = _native.check_plan(xs, t)
    lam = [math.prod(Fraction(xs[j], xs[j] - xs[m]) for j in range(k) if j != m) for m in range(k)]
    d_all = math.lcm(*[f.denominator for f in lam])
    divisors = robust.divisors(xs)
    assert divisors[k] == d_all and out[0] == f"plan {1 - k % 2}"
    mags, div = [], []
    for i, line in enumerate(out[1:k + 2]):
        a, d, shift, d_inv32, p_inv_d, recip, *w = map(int, line.split())
        if i < k:
            assert a == abs(lam[i] * d_all) and divisors[i] == chk.c[0][i] * d_all
            mags.append(a)
        assert (d, shift) == robust.odd_and_shift(divisors[i]) and d < 1 << 16
        if d > 1:
            assert (d * d_inv32 % (1 << 32), P * p_inv_d % d, recip) == (1, 1, ((1 << 64) - 1) // d)
            assert w == [pow(2, 32 * l, d) for l in range(17)]
        div.append((d, shift))
    assert ROBUST_PROPERTY[t, xs](k, r, c_max, xp_max, 1 - k % 2, max(mags), div), (k, r, c_max, xp_max, mags, div)

    # the rows are the cases they were made to be ...
    want = [robust.want(t, xs, ys) for ys in rows]
    assert all(m is None or m == v for m, (v, _) in zip(marks, want))
    assert len(marks) == len(edge) and {m for m in marks if m is not None} == {0xFF, 0, k - 1}
    assert [v for v, _ in want[len(edge):]] == [1, 0, 2, k - 2, 0xFE, 0xFF, 0xFF, 0xFF, k - 1, 0, k - 1]
    # ... and the finish gives each the definition's culprit and value
    assert [(int(v), int(f, 16)) for v, f in (line.split() for line in out[k + 2:])] == want
    # the check alone on the same rows
    assert run_check(programs, t, xs, rows) == [(v, 0xFF if v == 0xFF else 0xFE) for v, _ in want]


@pytest.mark.parametrize("t, xs", cases.EDGE)
def test_check_only_sets(programs, t, xs):
    k, r, c_max, _ = check_facts(t, xs)
    want_k, want_r, heavy, refusal = CHECK_PROPERTY[t, xs]
    assert (k, r) == (want_k, want_r) and (not heavy or 1 << 31 <= c_max < 1 << 32), (k, r, c_max)

    # the robust planner refuses the set, in the stand-alone program's code and words
    head, code, message = programs["robust_core_check"](host_program.share_lines(t, xs))[0].split(" ", 2)
    assert (head, int(code)) == ("error", _native.DN_ERR_UNSUPPORTED) and refusal in message
    with pytest.raises(NotImplementedError) as err:
        _native.robust_plan(xs, t)
    assert str(err.value) == message

    edge, marks = cases.edge_rows(t, xs)
    rows = edge + cases.rows(t, xs)
    want = [cases.verdict(xs, ys, t) for ys in rows]
    assert len(marks) == len(edge) and all(m is None or m == v for m, v in zip(marks, want))
    one = r >= 2  # with one spare share nothing is attributed
    assert want[len(edge):] == [1 if one else 0xFE, 0 if one else 0xFE, 2 if one else 0xFE, k - 2 if one else 0xFE,
                                0xFE, 0xFF, 0xFF, 0xFF, k - 1 if one else 0xFE]
    assert run_check(programs, t, xs, rows) == [(w, 0xFF if w == 0xFF else 0xFE) for w in want]
