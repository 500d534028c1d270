"""The five-limb reconstruct on the host (no kernel launches).

csrc/recon_low.hpp (the per-element arithmetic reconstruct_low_kernel runs)
and recon_low_eligible / recon_low_covers (csrc/recon_plan.hpp, the routing
decision) are compiled into tools/recon_low_check.cpp by the host compiler,
once plainly and once with AddressSanitizer and UndefinedBehaviorSanitizer
(a stand-alone program, not loaded into this process).  Every query goes
through both builds; the words are compared with Python big integers:

    out = (sum_i lambda_i y_i mod p) mod 2^64,  lambda_i exact rationals,

which does not look at the descriptor the library made.

The contract's boundary: with R = S mod p (before the division by 2^e) the
words are exact for every R < p - (A + 2) 2^480, A = sum |a_i|.  Every case
here computes R and asserts on which side it lies, so none is silently
dropped; for the one value inside the sliver (p - 5) nothing else is asserted.
"""
import os
import random
import shutil
import subprocess
from fractions import Fraction

import pytest

from delta_node.crypto.shamir import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = (1 << 521) - 1
M64 = (1 << 64) - 1

# ({2,3,5} has the integer weights 5, -5, 1: d = 1, so it is routed to the five-limb path too)
ELIGIBLE_XS = [(1, 3, 5), (1, 2, 3), (1, 2), (2, 4, 6, 8), (1, 2, 3, 4, 5), (2, 3, 5)]
# d = 3 by exact division; two-limb weights times d^-1; full-width weights
INELIGIBLE_XS = [(1, 2, 4), (1, 100000, 200001), (1, 70000, 140001, 300007)]
SECRETS = [0, 1, 2, 3, 7, 1 << 63, (1 << 64) - 1, (1 << 64) - 2, (1 << 300) + 5, (1 << 479) - 1]


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    out = tmp_path_factory.mktemp("recon_low")
    base = [cxx, "-std=c++17", "-I", os.path.join(ROOT, "delta-node_amd", "csrc"),
            os.path.join(ROOT, "tools", "recon_low_check.cpp")]
    plain, san = str(out / "recon_low_check"), str(out / "recon_low_check_san")
    build = subprocess.run(base + ["-O2", "-o", plain], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    cmd = base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", san]
    # the sanitizer runtimes linked statically where the compiler can (the
    # program then runs whatever else the environment loads into processes)
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return plain, san


def ask(tools, lines):
    """The tool's answers to the query lines, the same from both builds."""
    text = "".join(line + "\n" for line in lines)
    outs = []
    for exe in tools:
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (exe, r.stdout[-2000:], r.stderr[-2000:])
        outs.append(r.stdout.split("\n")[:-1])
    assert outs[0] == outs[1], "the sanitizer build answers differently"
    assert len(outs[0]) == len(lines)
    return outs[0]


def lambdas(xs):
    """Lagrange-at-0 weights as exact rationals (shamir.py:77-89)."""
    out = []
    for i, xi in enumerate(xs):
        lam = Fraction(1)
        for j, xj in enumerate(xs):
            if j != i:
                lam *= Fraction(xj, xj - xi)
        out.append(lam)
    return out


def exact(xs, ys):
    """f(0) mod p, canonical."""
    acc = 0
    for lam, y in zip(lambdas(xs), ys):
        acc += lam.numerator * pow(lam.denominator, -1, P) * y
    return acc % P


def call_line(w, u64=1, fe=0, ovf=0, a_limbs=None, has_inv=None):
    a_limbs = w.a_limbs if a_limbs is None else a_limbs
    has_inv = w.has_inv if has_inv is None else has_inv
    return "C %x %x %x %x %x %x %x %x " % (u64, fe, ovf, a_limbs, has_inv, w.k, w.shift, w.neg) + \
        " ".join("%x" % w.a[i][0] for i in range(w.k))


def elem_line(ys):
    words = []
    for y in ys:
        words += [y & 0xFFFFFFFF, (y >> 32) & 0xFFFFFFFF, (y >> 64) & 0xFFFFFFFF, (y >> 480) & 0xFFFFFFFF, y >> 512]
    return "E " + " ".join("%x" % v for v in words)


def in_sliver(w, xs, ys):
    """Whether R = S mod p, the residue before the division by 2^shift, lies
    within (A + 2) 2^480 of p."""
    A = sum(w.a[i][0] for i in range(w.k))
    R = exact(xs, ys) * (1 << w.shift) % P
    return R >= P - (A + 2) * (1 << 480)


def share(rnd, xs, secret):
    coeffs = [secret] + [rnd.randrange(1, P) for _ in xs[1:]]
    return [sum(c * pow(x, j, P) for j, c in enumerate(coeffs)) % P for x in xs]


def check_rows(tools, xs, rows):
    """Every element's word from the tool equals the exact one; none is in the sliver."""
    w = _native.lagrange(list(xs), len(xs))
    got = ask(tools, [call_line(w)] + [elem_line(ys) for ys in rows])
    assert got[0].split()[:3] == ["R", "1", "1"], (xs, got[0])
    assert int(got[0].split()[3], 16) == sum(w.a[i][0] for i in range(w.k))
    for ys, line in zip(rows, got[1:]):
        assert not in_sliver(w, xs, ys), (xs, ys)
        assert line == "W %x" % (exact(xs, ys) & M64), (xs, ys)


def test_descriptors_are_what_the_cases_assume():
    """d = 1 with one-limb weights for the eligible sets (e = 3 for {1,3,5}, 0
    for {1,2,3}); d = 3 for {2,3,5}."""
    for xs in ELIGIBLE_XS:
        w = _native.lagrange(list(xs), len(xs))
        assert (w.a_limbs, w.has_inv) == (1, 0), xs
        lams = lambdas(xs)
        for i, lam in enumerate(lams):
            assert Fraction(w.a[i][0] * (-1 if (w.neg >> i) & 1 else 1), 1 << w.shift) == lam, xs
    w = _native.lagrange([1, 3, 5], 3)
    assert ([w.a[i][0] for i in range(3)], w.neg, w.shift) == ([15, 10, 3], 0b010, 3)
    assert _native.lagrange([1, 2, 3], 3).shift == 0
    got = [(w.a_limbs, w.has_inv) for w in (_native.lagrange(list(xs), len(xs)) for xs in INELIGIBLE_XS)]
    assert got == [(1, 2), (2, 1), (17, 0)]


def test_routing(tools):
    """Eligible: int64 output alone, one-limb weights, d = 1, sum |a_i| < 2^24;
    the five-limb kernels cover k = 2..5."""
    w = _native.lagrange([1, 3, 5], 3)
    d3 = _native.lagrange([1, 2, 4], 3)
    big = _native.ones_weights(2)
    big.a[0][0], big.a[1][0] = (1 << 24) - 2, 1
    edge = _native.ones_weights(2)
    edge.a[0][0], edge.a[1][0] = (1 << 24) - 1, 1
    wide = _native.ones_weights(2)
    wide.a[0][0], wide.a[1][0] = 0xFFFFFFFF, 0xFFFFFFFF  # (a 64-bit sum would wrap in 32)
    got = ask(tools, [
        call_line(w), call_line(w, ovf=1), call_line(w, fe=1), call_line(w, u64=0, fe=1), call_line(w, fe=1, ovf=1),
        call_line(d3), call_line(w, a_limbs=2), call_line(w, a_limbs=17), call_line(w, has_inv=1),
        call_line(w, has_inv=2), call_line(big), call_line(edge), call_line(wide),
        call_line(_native.ones_weights(1)), call_line(_native.ones_weights(5)), call_line(_native.ones_weights(6)),
        call_line(_native.ones_weights(16)),
    ])
    want = ["R 1 1 1c", "R 0 1 0", "R 0 1 0", "R 0 1 0", "R 0 1 0",
            "R 0 1 0", "R 0 1 0", "R 0 1 0", "R 0 1 0",
            "R 0 1 0", "R 1 1 ffffff", "R 0 1 0", "R 0 1 0",
            "R 1 0 1", "R 1 1 5", "R 1 0 6", "R 1 0 10"]
    assert got == want
    for xs in ELIGIBLE_XS:
        assert ask(tools, [call_line(_native.lagrange(list(xs), len(xs)))])[0].startswith("R 1 1 "), xs
    for xs in INELIGIBLE_XS:
        assert ask(tools, [call_line(_native.lagrange(list(xs), len(xs)))])[0] == "R 0 1 0", xs


@pytest.mark.parametrize("xs", ELIGIBLE_XS)
def test_sharings(tools, xs):
    """Valid sharings of each listed secret (3: the R < q carry case for
    {1,3,5}; the last two are field-sized), three draws of coefficients each."""
    rnd = random.Random(521 + len(xs) + xs[-1])
    secrets = SECRETS + [rnd.getrandbits(64) for _ in range(16)] + [rnd.getrandbits(519) for _ in range(4)]
    rows = [share(rnd, xs, s) for s in secrets for _ in range(3)]
    for s, ys in zip([s for s in secrets for _ in range(3)], rows):
        assert exact(xs, ys) == s
    check_rows(tools, xs, rows)


@pytest.mark.parametrize("xs", ELIGIBLE_XS)
def test_rows_that_are_no_sharing(tools, xs):
    """Random rows; all-ones in planes 3..14; y = 0 and y = p - 1 in the rows
    whose weight is negative (~y is then all ones, and 0) with the others
    random, and the other way round."""
    rnd = random.Random(96 + len(xs) + xs[0])
    w = _native.lagrange(list(xs), len(xs))
    k = len(xs)
    mid = ((1 << 384) - 1) << 96
    rows = [[rnd.randrange(P) for _ in xs] for _ in range(200)]
    rows += [[rnd.randrange(P) | mid for _ in xs] for _ in range(50)]
    assert w.neg != 0
    for edge in (0, P - 1):
        for flip in (False, True):
            for _ in range(10):
                rows.append([edge if bool((w.neg >> i) & 1) != flip else rnd.randrange(P) for i in range(k)])
    # no row is dropped: check_rows computes each one's R and asserts it is outside the sliver
    assert len(rows) == 290
    check_rows(tools, xs, rows)


def test_the_sliver_is_where_the_contract_says(tools):
    """A sharing of p - 5: its R lies within (A + 2) 2^480 of p, outside the
    contract.  Nothing is asserted about the word (the tool must only answer);
    the largest value the contract promises, 2^480 - 1, is on the exact side."""
    rnd = random.Random(5)
    xs = (1, 3, 5)
    w = _native.lagrange(list(xs), 3)
    ys = share(rnd, xs, P - 5)
    assert exact(xs, ys) == P - 5
    assert in_sliver(w, xs, ys)
    got = ask(tools, [call_line(w), elem_line(ys)])
    assert got[1].startswith("W ")
    ok = share(rnd, xs, (1 << 480) - 1)
    assert not in_sliver(w, xs, ok)
    assert ask(tools, [call_line(w), elem_line(ok)])[1] == "W %x" % M64
