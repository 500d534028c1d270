"""resolve_shares_vec_robust without a device: the planner (csrc/robust_plan.hpp)
against fractions.Fraction, the kernel's finish (csrc/robust_core.hpp) in a
stand-alone program, built plainly and under ASan + UBSan, against the definition
in Python integers; refusals by code and message; the method's argument errors."""
import math
from fractions import Fraction

import pytest
import torch

import host_program
import share_robust_cases as robust
from delta_node.crypto import shamir
from delta_node.crypto.shamir import _native, field

P = robust.P


@pytest.fixture(scope="module", params=[[], host_program.SANITIZE], ids=["plain", "sanitized"])
def program(request, tmp_path_factory):
    run = host_program.compile_program(tmp_path_factory.mktemp("resolve_robust"), "robust_core_check", request.param)
    return lambda t, xs, rows=(): run(host_program.share_lines(t, xs, rows))


@pytest.mark.parametrize("t, xs", robust.CASES + robust.MORE)
def test_plan_and_finish_against_the_definition(program, t, xs):
    k, chk = len(xs), _native.check_plan(xs, t)
    rows = robust.rows(t, xs) + [[P if chk.neg >> i & 1 else 0 for i in range(k)]]  # the non-canonical input p
    out = program(t, xs, rows)
    # the plan: lambda_m = A_m / D_all in lowest terms, and each divisor's constants
    lam = [math.prod(Fraction(xs[j], xs[j] - xs[m]) for j in range(k) if j != m) for m in range(k)]
    d_all = math.lcm(*[f.denominator for f in lam])
    assert out[0] == f"plan {1 - k % 2}"
    for i, line in enumerate(out[1:k + 2]):
        a, d, shift, d_inv32, p_inv_d, recip, *w = map(int, line.split())
        if i < k:
            sign = (-1) ** (k - 1) * (-1 if chk.neg >> i & 1 else 1)
            assert sign * a == lam[i] * d_all
        assert d % 2 == 1 and d < 1 << 16 and d << shift == (chk.c[0][i] * d_all if i < k else d_all)
        if d > 1:
            assert (d * d_inv32 % (1 << 32), P * p_inv_d % d, recip) == (1, 1, ((1 << 64) - 1) // d)
            assert w == [pow(2, 32 * l, d) for l in range(17)]
    # the finish
    want = [robust.want(t, xs, ys) for ys in rows]
    assert [v for v, _ in want[:9]] == [1, 0, 2, k - 2, 0xFE, 0xFF, 0xFF, 0xFF, k - 1]
    assert [v for v, _ in want[9:]] == [0, k - 1, 0xFF]
    assert [(int(v), int(f, 16)) for v, f in (line.split() for line in out[k + 2:])] == want


@pytest.mark.parametrize("t, xs, code, exc, text", [
    (3, (1, 2, 3, 4), _native.DN_ERR_UNSUPPORTED, NotImplementedError, "one spare share detects only"),
    (3, (1, 2, 3), _native.DN_ERR_UNSUPPORTED, NotImplementedError, "no spare share"),
    (3, (1, 2, 2, 3, 4), _native.DN_ERR_DISTINCT, ValueError, "shares must be distinct"),
    (3, (1, 2), _native.DN_ERR_TOO_FEW, ValueError, "need at least 3 shares"),
    # dn_m521_check_plan accepts this set; D_all's odd part is 6933465
    (3, (3, 8, 17, 26, 37), _native.DN_ERR_UNSUPPORTED, NotImplementedError, "odd part of 2\\^16 or more"),
])
def test_refusals(program, t, xs, code, exc, text):
    head, _, message = program(t, xs)[0].partition(f" {code} ")
    assert head == "error" and text.replace("\\", "") in message
    with pytest.raises(exc, match=text):
        _native.robust_plan(xs, t)


def test_argument_errors_fire_before_any_device_use(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("resolve_shares_vec_robust reached the device before its argument checks")

    monkeypatch.setattr(_native, "require_device", no_device)
    monkeypatch.setattr(_native, "reconstruct_robust", no_device)
    rows = [torch.zeros(field.vec_bytes(10), dtype=torch.uint8) for _ in range(5)]
    r = shamir.SecretShare(3).resolve_shares_vec_robust
    with pytest.raises(ValueError, match="^resolve_shares_vec_robust: one abscissa per share vector$"):
        r(rows, [1, 2, 3, 4], 10)
    with pytest.raises(ValueError, match="^shares must be distinct$"):
        r(rows, [1, 2, 3, 4, 1], 10)
    for xs, text in [([1, 2, 3, 4], "one spare share"), ([1, 2, 3], "no spare share"), ([0, 1, 2, 3, 4], "abscissa 0"),
                     ([1, 2, 3, 4, 1 << 64], "must fit 64 bits")]:
        with pytest.raises(NotImplementedError, match=text):
            r(rows[:1] * len(xs), xs, 10)
