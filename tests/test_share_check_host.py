"""check_shares_vec without a device: the planner's weights and error codes, the
kernel's arithmetic (csrc/check_core.hpp) in a stand-alone program under ASan +
UBSan against the definition in Python integers, the method's argument errors."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

import share_check_cases as cases
from delta_node.crypto import shamir
from delta_node.crypto.shamir import _native, field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = cases.P


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path_factory.mktemp("share_check") / "check_core_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "delta-node_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "host", "check_core_check.cpp"), "-o", exe]
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr

    def run(lines):
        done = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert done.returncode == 0, done.stdout + done.stderr
        return done.stdout.splitlines()

    return run


@pytest.mark.parametrize("xs, t, signed", [
    ((1, 2, 3, 4, 5), 3, [[1, -4, 6, -4, 1], [1, -8, 18, -16, 5]]),
    ((1, 3, 4, 7, 9), 3, [[5, -30, 32, -10, 3], [5, -90, 128, -70, 27]]),
])
def test_planner_weights(xs, t, signed):
    plan = _native.check_plan(xs, t)
    got = [[(-1 if plan.neg >> i & 1 else 1) * plan.c[j][i] for i in range(plan.k)] for j in range(plan.r)]
    assert (plan.k, plan.r, got) == (len(xs), len(xs) - t, signed)
    # ... and they are parity checks: every polynomial of degree < t sums to zero
    for j, row in enumerate(signed):
        for d in range(t):
            assert sum(w * x ** d for w, x in zip(row, xs)) == 0, (j, d)


@pytest.mark.parametrize("xs, t, code, exc, text", [
    ((), 3, _native.DN_ERR_ARG, ValueError, "not enough values to unpack"),
    ((1, 2), 3, _native.DN_ERR_TOO_FEW, ValueError, "need at least 3 shares"),
    ((1, 2, 2, 3), 3, _native.DN_ERR_DISTINCT, ValueError, "shares must be distinct"),
    ((7,), 1, _native.DN_ERR_EMPTY, TypeError, "reduce\\(\\) of empty iterable"),
    ((1, 2, 3), 0, _native.DN_ERR_ARG, ValueError, "threshold below 1"),
    (tuple(range(1, 18)), 14, _native.DN_ERR_UNSUPPORTED, NotImplementedError, "more than 16 shares"),
    ((1, 2, 3), 3, _native.DN_ERR_UNSUPPORTED, NotImplementedError, "no spare share"),
    (tuple(range(1, 9)), 3, _native.DN_ERR_UNSUPPORTED, NotImplementedError, "more than 4 spare shares"),
    ((0, 1, 2, 3), 3, _native.DN_ERR_UNSUPPORTED, NotImplementedError, "abscissa 0"),
    ((1, 2, 3, 1 << 40), 2, _native.DN_ERR_UNSUPPORTED, NotImplementedError, "2\\^63 or more"),
    ((1, 2, 3, 100000), 2, _native.DN_ERR_UNSUPPORTED, NotImplementedError, "2\\^32 or more"),
    (tuple((1 << 63) + 1000 * i for i in range(16)), 14, _native.DN_ERR_UNSUPPORTED, NotImplementedError,
     "leave 128 bits"),
])
def test_planner_error_codes(xs, t, code, exc, text):
    arr = (ctypes.c_uint64 * max(1, len(xs)))(*xs)
    assert _native.lib().dn_m521_check_plan(arr, len(xs), t, ctypes.byref(_native.CheckPlan())) == code
    with pytest.raises(exc, match=text):
        _native.check_plan(xs, t)


@pytest.mark.parametrize("t, xs", cases.CASES)
def test_core_against_the_definition(program, t, xs):
    k, plan = len(xs), _native.check_plan(xs, t)
    # ... and a zero syndrome with limbs all 0: y = 0 under the positive weights, the non-canonical p under the others
    rows = cases.rows(t, xs) + [[P if plan.neg >> i & 1 else 0 for i in range(k)]]
    want = [cases.verdict(xs, ys, t) for ys in rows]
    one = k - t >= 2  # with one spare share nothing is attributed
    assert want == [1 if one else 0xFE, 0 if one else 0xFE, 2 if one else 0xFE, k - 2 if one else 0xFE, 0xFE,
                    0xFF, 0xFF, 0xFF, k - 1 if one else 0xFE, 0xFF]
    out = program([f"{t} {k} " + " ".join(map(str, xs))] + [" ".join(f"{y:x}" for y in ys) for ys in rows])
    got = [tuple(map(int, line.split())) for line in out]
    assert got == [(w, 0xFF if w == 0xFF else 0xFE) for w in want]


def test_argument_errors_fire_before_any_device_use(monkeypatch):
    def no_device():
        raise AssertionError("check_shares_vec reached the device before its argument checks")

    monkeypatch.setattr(_native, "require_device", no_device)
    monkeypatch.setattr(_native, "check_shares", lambda *a, **k: no_device())
    vb = field.vec_bytes(10)
    rows = [torch.zeros(vb, dtype=torch.uint8) for _ in range(5)]
    c = shamir.SecretShare(3).check_shares_vec
    with pytest.raises(NotImplementedError, match="GF\\(2\\^521 - 1\\) only"):
        shamir.SecretShare(3, prime=(1 << 127) - 1).check_shares_vec(rows, [1, 2, 3, 4, 5], 10)
    with pytest.raises(ValueError, match="^check_shares_vec: one abscissa per share vector$"):
        c(rows, [1, 2, 3, 4], 10)
    with pytest.raises(ValueError, match="^not enough values to unpack"):
        c([], [], 10)
    with pytest.raises(ValueError, match="^need at least 3 shares$"):
        c(rows[:2], [1, 2], 10)
    with pytest.raises(ValueError, match="^shares must be distinct$"):
        c(rows, [1, 2, 3, 4, 1], 10)
    with pytest.raises(TypeError, match="^reduce\\(\\) of empty iterable with no initial value$"):
        shamir.SecretShare(1).check_shares_vec(rows[:1], [1], 10)
    for xs, text in [([1, 2, 3], "no spare share"), ([0, 1, 2, 3], "abscissa 0"),
                     ([1, 2, 3, 1 << 64], "must fit 64 bits"), (list(range(1, 9)), "more than 4 spare shares")]:
        with pytest.raises(NotImplementedError, match=text):
            c(rows[:1] * len(xs), xs, 10)
