"""The two-error robust reconstruct without a device: the kernel's pair finish (csrc/robust_pair.hpp) and
the plan's new bounds (robust_plan_build2) in a stand-alone program, built plainly and under
ASan + UBSan, against Python integers; the method's errors= argument."""
import pytest
import torch

import host_program
import robust2_cases as cases
from delta_node.crypto import shamir
from delta_node.crypto.shamir import _native, field

P = cases.P


@pytest.fixture(scope="module", params=[[], host_program.SANITIZE], ids=["plain", "sanitized"])
def program(request, tmp_path_factory):
    return host_program.compile_program(tmp_path_factory.mktemp("resolve_robust2"), "robust_pair_check", request.param)


def plan_line(errors, t, xs):
    return f"plan {errors} {t} {len(xs)} " + " ".join(map(str, xs))


@pytest.mark.parametrize("t, xs", cases.SETS)
def test_the_finish_on_crafted_syndromes(program, t, xs):
    """(S_0 .. S_3, T') as check_mac leaves them, unreduced, from Python integers: each share y or p - y by
    its weight's sign, times |w_i| x_i^m and |A_i|."""
    rows, marks, values = cases.block(t, xs)
    plan = _native.robust_plan(xs, t, 2)
    chk, k = plan.check, len(xs)
    assert (plan.max_errors, _native.robust_plan(xs, t).max_errors) == (2, 0)
    lines = [plan_line(2, t, xs)]
    for ys in rows:
        Y = [P - y if chk.neg >> i & 1 else y for i, y in enumerate(ys)]
        chains = [sum(chk.c[m][i] * Y[i] for i in range(k)) for m in range(4)] + [sum(plan.a[i] * Y[i] for i in range(k))]
        lines.append("fin " + " ".join(f"{c:x}" for c in chains))
    out = program(lines)
    assert out[0] == "ok 2 1"
    got = [(int(v), int(hits), int(f, 16)) for v, hits, f in (line.split() for line in out[1:])]
    assert got == [(m, 1 if 16 <= m < 0xFE else 0, v) for m, v in zip(marks, values)]


@pytest.mark.parametrize("v", [1, 2, 3, 6, 3 << 15, 65535, 65537])
def test_divisor_constants_on_the_fly(program, v):
    d, shift = v, 0
    while d % 2 == 0:
        d, shift = d // 2, shift + 1
    line = program([f"div {v}"])[0]
    if d >= 1 << 16:
        assert line == "reject"
    elif d == 1:
        assert line.split()[:2] == ["1", str(shift)]
    else:
        want = [d, shift, pow(d, -1, 1 << 32), pow(P, -1, d), ((1 << 64) - 1) // d] + [pow(2, 32 * l, d) for l in range(17)]
        assert list(map(int, line.split())) == want


@pytest.mark.parametrize("errors, t, xs, code, exc, text", [
    (2, 3, (1, 2, 3, 4, 5, 6), _native.DN_ERR_UNSUPPORTED, NotImplementedError, "exactly four spare shares"),
    (2, 3, (1, 2, 3, 4, 5), _native.DN_ERR_UNSUPPORTED, NotImplementedError, "exactly four spare shares"),
    (2, 3, (1, 2, 3, 4), _native.DN_ERR_UNSUPPORTED, NotImplementedError, "one spare share detects only"),
    (2, 3, (1, 2, 2, 3, 4, 5, 6), _native.DN_ERR_DISTINCT, ValueError, "shares must be distinct"),
    (3, 3, (1, 2, 3, 4, 5, 6, 7), _native.DN_ERR_ARG, ValueError, "errors must be 1 or 2"),
])
def test_refusals(program, errors, t, xs, code, exc, text):
    head, _, message = program([plan_line(errors, t, xs)])[0].partition(f" {code} ")
    assert head == "error" and text.replace("\\", "") in message
    with pytest.raises(exc, match=text):
        _native.robust_plan(xs, t, errors)


@pytest.mark.parametrize("xs, text", [
    ((2, (1 << 32) - 2), "x_i + x_j or x_i x_j of 2^32 or more"), ((3, 65536, 65537), "x_i + x_j or x_i x_j of 2^32"),
    ((1, 2, 1 + (65537 << 3)), "difference x_j - x_i with an odd part of 2^16 or more"), ((1 + (65535 << 4), 1), None),
])
def test_pair_bounds_each_with_its_message(program, xs, text):
    """(Through dn_m521_robust_plan2 the r = 4 weight bound x^3 < 2^32 refuses such abscissas first.)"""
    line = program([f"bounds {len(xs)} " + " ".join(map(str, xs))])[0]
    assert line == "ok" if text is None else line.startswith(f"error {_native.DN_ERR_UNSUPPORTED} ") and text in line


@pytest.mark.parametrize("t, xs", cases.SETS + [(3, (1, 2, 3, 4, 5)), (12, tuple(range(1, 17)))])
def test_one_error_through_the_new_entry_is_the_old_plan(program, t, xs):
    assert program([plan_line(1, t, xs)]) == ["ok 0 1"]
    old, new = _native.robust_plan(xs, t), _native.RobustPlan()
    arr = (_native.ctypes.c_uint64 * len(xs))(*xs)
    _native.check(_native.lib().dn_m521_robust_plan2(arr, len(xs), t, 1, _native.ctypes.byref(new)))
    assert bytes(old) == bytes(new)


def test_argument_errors_fire_before_any_device_use(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the robust reconstruct reached the device before its argument checks")

    for name in ("require_device", "reconstruct_robust", "reconstruct_records_robust"):
        monkeypatch.setattr(_native, name, no_device)
    ss = shamir.SecretShare(3)
    rows = [torch.zeros(field.vec_bytes(10), dtype=torch.uint8)] * 7
    for errors, k, exc, text in [(3, 7, ValueError, "errors must be 1 or 2"), (0, 7, ValueError, "errors must be 1 or 2"),
                                 (2, 6, NotImplementedError, "exactly four spare shares"),
                                 (2, 4, NotImplementedError, "one spare share detects only")]:
        with pytest.raises(exc, match=text):
            ss.resolve_shares_vec_robust(rows[:k], list(range(1, k + 1)), 10, errors=errors)
