"""The robust reconstruct's reference and rows (host and GPU tests): the
DEFINITION in Python integers on share_check_cases' rows — the interpolant of
the shares without the located one, else of all k."""
import math
import random
from fractions import Fraction

import share_check_cases as cases

P = cases.P
# the r >= 2 sets of share_check_cases, then odd divisors up to 59535 and k = 16
CASES = [c for c in cases.CASES if len(c[1]) - c[0] >= 2]
MORE = [(3, (2, 5, 11, 13, 16)), (12, tuple(range(1, 17)))]
# Sets for the divisor shifts and the weight bound (test_share_edges_host.py asserts each property from the
# project's plan): shifts of 10..31; shifts of 24..32 and |A| >= 2^29; c >= 2^31 and xp = 40955^2 at r = 3;
# |A| >= 2^31; k even at r = 2 and at r = 3; k = 3
ROBUST_EDGE = [(2, (1, 2, 5, 17)), (2, (1, 17, 33, 129, 257)), (2, tuple(8191 * i for i in range(1, 6))),
               (3, (360, 361, 362, 363, 364)), (2, (1, 2, 3, 8)), (3, (1, 2, 3, 4, 5, 6)), (1, (1, 2, 3))]


def want(t, xs, ys):
    """(culprit byte, value) the definition gives one element's shares."""
    v = cases.verdict(xs, ys, t)
    pts = [(x, y) for i, (x, y) in enumerate(zip(xs, ys)) if i != v]
    return v, cases.interpolate(pts, 0)


def rows(t, xs):
    """share_check_cases' nine rows, then secrets 0 and p - 1 under a located error."""
    k, out = len(xs), cases.rows(t, xs)
    for secret, i, delta in ((0, 0, 5), (P - 1, k - 1, P - 7)):
        f = [secret] + [(i + 2) * (j + 3) for j in range(t - 1)]  # a polynomial with f(0) = secret
        ys = [sum(c * x ** j for j, c in enumerate(f)) % P for x in xs]
        ys[i] = (ys[i] + delta) % P
        out.append(ys)
    return out


def divisors(xs):
    """The integers a robust reconstruct divides by, from exact rationals: D_all, the least common
    denominator of the Lagrange weights at 0 of all k abscissas, alone (the last entry), and before it
    |w_i| D_all per share i, w_i the parity-check weight lcm_m(P_m) / P_i, P_i = prod_{m != i} |x_i - x_m|."""
    k = len(xs)
    lam = [math.prod(Fraction(xs[j], xs[j] - xs[m]) for j in range(k) if j != m) for m in range(k)]
    d_all = math.lcm(*[f.denominator for f in lam])
    prods = [math.prod(abs(xs[i] - xs[m]) for m in range(k) if m != i) for i in range(k)]
    return [math.lcm(*prods) // p * d_all for p in prods] + [d_all]


def odd_and_shift(v):
    e = (v & -v).bit_length() - 1
    return v >> e, e


def targets(v):
    """The residues at which dividing by v = d 2^e, d odd, takes its special cases: the exact division adds
    m p with m = 0 (a residue divisible by d), the m right after it and m = d - 1 (a residue == p mod d);
    the rotation by e moves low bits all ones, all zero and a lone bit e, and bit 520."""
    d, e = odd_and_shift(v)
    out = [1, P - 1, (1 << e) - 1, 1 << e, P - (1 << e), 1 << 520]
    if d > 1:
        out += [d * 12345, d * 12345 + 1, d * 12345 + P % d]
        assert [-u * pow(P, -1, d) % d for u in out[-3:]] == [0, pow(-P, -1, d), d - 1]
    return list(dict.fromkeys(out))


def edge_rows(t, xs):
    """(rows, verdicts) of share_check_cases.edge_rows, then genuine sharings whose secret puts a chosen
    residue u in front of the final division: f(0) = +-u / v for the divisor v (the sign is the plan's
    negation for even k).  Undamaged, the residue is canon(T') and v is D_all; with share i moved by any
    delta it is canon(N) and v is |w_i| D_all: the delta cancels in N = |w_i| T' - |A_i| S_0."""
    k, rng = len(xs), random.Random(7000 * t + len(xs) + xs[-1])
    div = divisors(xs)
    out, marks = cases.edge_rows(t, xs)

    def crafted(u, v, i=None, delta=0):
        f = [(-1) ** (k - 1) * u * pow(v, -1, P) % P] + [rng.randrange(P) for _ in range(t - 1)]
        assert f[0] * v % P == (u if k % 2 else -u % P)
        ys = [sum(c * x ** j for j, c in enumerate(f)) % P for x in xs]
        if i is not None:
            ys[i] = (ys[i] + delta) % P
        out.append(ys)
        marks.append(cases.CONSISTENT if i is None else i)

    for u in targets(div[k]):
        crafted(u, div[k])
    for i in (0, k - 1):
        for u in targets(div[i]):
            crafted(u, div[i], i, 1)
            crafted(u, div[i], i, 1 + rng.randrange(P - 1))
    for u in (P - 1, 1 << 520):  # canon(T') of an undamaged row, under a located error
        crafted(u, div[k], 0, 1)
        crafted(u, div[k], k - 1, 1 + rng.randrange(P - 1))
    return out, marks
