"""Edge inputs and exact expected values for the GF(2^521 - 1) kernels — a
helper for test_field_edges_host.py and test_gpu_field_edges.py (no tests).

Everything here is plain Python integers: the field arithmetic is exact, so
the reference of every comparison is `%` on big integers and the comparison
is bit for bit.  The inputs are built to reach what uniformly random field
elements do not: a carry out of limb 0 after the Mersenne fold (and past an
all-ones limb), a folded value whose bits 512..520 are all set, a non-zero
multiple of p, the forward-difference bound of the lazy 17-limb form, the
borrow chain of the exact small division and both arms of the 521-bit
rotation (csrc/m521_device.hpp).
"""
from __future__ import annotations

import functools
import random
from fractions import Fraction
from typing import List, Sequence

P = (1 << 521) - 1
M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
TILE = 256
N_LAYOUT = 4 * TILE + 37  # four full tiles and a partial one


# ------------------------------------------------------------------ the pool
@functools.lru_cache(maxsize=None)
def _edge_values() -> tuple:
    vals = [0, 1, 2, P, P - 1, P - 2, 1 << 520, (1 << 520) - 1, (1 << 520) + 1]
    ks = sorted({m + d for m in range(32, 513, 32) for d in (-1, 0, 1)} | {520})
    for k in ks:
        vals += [(1 << k) - 1, 1 << k, (1 << k) + 1, P - (1 << k), P - (1 << k) - 1, P - (1 << k) + 1]

    def limb(j):  # an all-ones limb j (limb 16 holds 9 bits)
        return (0x1FF if j == 16 else M32) << (32 * j)

    vals += [P ^ limb(j) for j in range(17)]  # every limb ones but one
    vals += [limb(j) for j in range(17)]  # one limb ones
    vals += [sum(limb(j) for j in range(ph, 17, 2)) for ph in (0, 1)]  # alternating, both phases
    vals += [sum(limb(i) for i in range(j + 1)) for j in range(17)]  # limbs 0..j ones
    seen, out = set(), []
    for v in vals:
        assert 0 <= v < (1 << 521)
        if v not in seen:
            seen.add(v)
            out.append(v)
    return tuple(out)


def edge_values() -> List[int]:
    """The fixed pool of field inputs in [0, 2^521), p itself included
    (include/dn_shamir.h: inputs must be < 2^521)."""
    return list(_edge_values())


# ------------------------------------------------------------------ expected values
def split_unreduced(c: Sequence[int], x: int) -> int:
    """F = sum_j c_j x^j as an integer (c[0] the secret)."""
    acc = 0
    for cj in reversed(c):
        acc = acc * x + cj
    return acc


def split_expected(c: Sequence[int], x: int) -> int:
    return split_unreduced(c, x) % P


def recon_expected(ys: Sequence[int], a: Sequence[int], neg: int, d: int = 1, shift: int = 0) -> int:
    """(sum_i +-a_i y_i) * d^-1 * 2^-shift mod p (bit i of `neg`: a_i negative)."""
    s = sum((-ai if (neg >> i) & 1 else ai) * y for i, (ai, y) in enumerate(zip(a, ys)))
    return s * pow(d << shift, -1, P) % P


def lagrange_at_zero(xs: Sequence[int]) -> List[int]:
    """lambda_i = prod_{j != i} x_j / (x_j - x_i) mod p."""
    out = []
    for i, xi in enumerate(xs):
        num = den = 1
        for j, xj in enumerate(xs):
            if j != i:
                num *= xj
                den *= xj - xi
        out.append(num * pow(den, -1, P) % P)
    return out


# ------------------------------------------------------------------ predicates on F
def fold_once(F: int) -> int:
    return (F & P) + (F >> 521)


def pred_carry0(F: int) -> bool:
    """The fold's add carries out of limb 0."""
    return (F & M32) + (F >> 521) > M32


def pred_carry_multi(F: int) -> bool:
    """... and the next limb is all ones: the carry goes past limb 1."""
    return pred_carry0(F) and ((F >> 32) & M32) == M32


def pred_top_ones(F: int) -> bool:
    """Bits 512..520 of the folded value are all set (canon() has work)."""
    return (fold_once(F) >> 512) & 0x1FF == 0x1FF


def pred_multiple_of_p(F: int) -> bool:
    return F != 0 and F % P == 0


PREDICATES = {"carry0": pred_carry0, "carry_multi": pred_carry_multi, "top_ones": pred_top_ones,
              "multiple_of_p": pred_multiple_of_p}


def fd_needs_fold(t: int, n: int) -> bool:
    """csrc/dn_internal.hpp fd_needs_fold, the same double arithmetic."""
    s, p = 0.0, 1.0
    for _ in range(t):
        s += p
        p *= float(n + t)
    return s >= 8388608.0


def fd_max_n(t: int) -> int:
    """The largest share count the forward-difference split takes at threshold t."""
    n = t
    assert not fd_needs_fold(t, n)
    while n < 65535 and not fd_needs_fold(t, n + 1):
        n += 1
    return n


def fd_overflow_n(t: int) -> int:
    """The smallest share count whose LAST share, with every coefficient p - 1,
    no longer fits the 17 limbs unreduced (sum_{1<=j<t} c_j n^j >= 2^544): from
    there on a difference table that is never folded is wrong, not merely
    outside its stated bound."""
    n = t
    while (P - 1) * sum(n ** j for j in range(1, t)) < (1 << 544):
        n += 1
    return n


# ------------------------------------------------------------------ descriptors
def make_desc(a: Sequence[int], neg: int, a_limbs: int, shift: int = 0, has_inv: int = 0, d: int = 1):
    """A dn_m521_lagrange_t filled from the header's definitions
    (include/dn_shamir.h, the comment above the struct), not by dn_m521_lagrange."""
    from delta_node.crypto.shamir import _native

    w = _native.Lagrange()
    w.k = len(a)
    w.a_limbs = a_limbs
    w.neg = neg
    w.shift = shift
    w.has_inv = has_inv
    for i, ai in enumerate(a):
        assert 0 <= ai < (1 << (32 * a_limbs)) and (a_limbs < 17 or ai < P)
        for j in range(a_limbs):
            w.a[i][j] = (ai >> (32 * j)) & M32
    if has_inv:
        w.d = d & M32
    if has_inv == 1:
        inv = pow(d, -1, P)
        for j in range(17):
            w.inv[j] = (inv >> (32 * j)) & M32
    elif has_inv == 2:
        assert 3 <= d < 65536 and d & 1
        w.d_inv32 = pow(d, -1, 1 << 32)
        w.p_inv_d = pow(P % d, -1, d)
        w.d_recip = M64 // d
        for j in range(17):
            w.w[j] = pow(2, 32 * j, d)
    else:
        assert d == 1
    return w


def desc_from_xs(xs: Sequence[int]):
    """The small-rational descriptor of abscissas xs: lambda_i = a_i / (d 2^shift)
    with the a_i over the least common denominator (k <= 16, small xs)."""
    lams = []
    for i, xi in enumerate(xs):
        f = Fraction(1)
        for j, xj in enumerate(xs):
            if j != i:
                f *= Fraction(xj, xj - xi)
        lams.append(f)
    L = 1
    for f in lams:
        L = L * f.denominator // _gcd(L, f.denominator)
    a = [abs(f.numerator) * (L // f.denominator) for f in lams]
    neg = sum(1 << i for i, f in enumerate(lams) if f < 0)
    assert max(a) < (1 << 64)
    e = (L & -L).bit_length() - 1
    shift, d = (e, L >> e) if e < 32 else (0, L)
    has_inv = 0 if d == 1 else 2 if (d < 65536 and d & 1) else 1
    return make_desc(a, neg, 2 if max(a) >> 32 else 1, shift, has_inv, d)


def desc_parts(w):
    """(|a_i| as integers, neg, d, shift) of a small-rational descriptor."""
    a = [sum(w.a[i][j] << (32 * j) for j in range(w.a_limbs)) for i in range(w.k)]
    return a, w.neg, (w.d if w.has_inv else 1), w.shift


def _gcd(a: int, b: int) -> int:
    while b:
        a, b = b, a % b
    return a


def desc_fields(w) -> dict:
    """Every field of a descriptor as plain Python values (for comparison)."""
    return {"k": w.k, "a_limbs": w.a_limbs, "neg": w.neg, "shift": w.shift, "has_inv": w.has_inv, "d": w.d,
            "a": [list(row) for row in w.a], "inv": list(w.inv), "d_inv32": w.d_inv32, "p_inv_d": w.p_inv_d,
            "d_recip": w.d_recip, "w": list(w.w), "reserved": w.reserved}


# ------------------------------------------------------------------ layout
# kind of every element: "E" an edge element among edges, "L" the lone edge
# element of an otherwise random quarter, "R" random.
LONE_LANES = (0, 64 + 63, 128 + 31, 192 + 32)  # lane 0, lane 63 and two middle lanes of tile 1's quarters


def layout_kinds(N: int = N_LAYOUT) -> List[str]:
    """Full tiles cycle through: all edges / random with one edge per 64-lane
    quarter / all random / mixed; a partial last tile holds edges.  The
    wave-uniform slow path of the stores thus runs with every lane rare-able
    (tile 0), with one rare lane reducing 63 ordinary ones in place (tile 1),
    not at all (tile 2) and mixed (tile 3)."""
    full = N // TILE
    out = []
    for i in range(N):
        tile, lane = divmod(i, TILE)
        if tile >= full:
            out.append("E")
        elif tile % 4 == 0:
            out.append("E")
        elif tile % 4 == 1:
            out.append("L" if lane in LONE_LANES else "R")
        elif tile % 4 == 2:
            out.append("R")
        else:
            out.append("E" if (lane * 5 + lane // 64) % 3 == 0 else "R")
    return out


def rand_fe(rng: random.Random) -> int:
    return rng.randint(1, P - 1)


def layout_values(N: int = N_LAYOUT, seed: int = 0, phase: int = 0) -> List[int]:
    """Pool values at the layout's edge positions (walking the pool from
    `phase`), seeded random field elements elsewhere."""
    pool, rng = _edge_values(), random.Random(seed)
    out, e = [], 0
    for kind in layout_kinds(N):
        r = rand_fe(rng)
        if kind == "R":
            out.append(r)
        else:
            out.append(pool[(phase + e) % len(pool)])
            e += 1
    return out


# ------------------------------------------------------------------ split cases
def _targets(ei: int, sel: int) -> int:
    """Residue the solved coefficient steers F(x*) to, by class."""
    pool = _edge_values()
    if sel == 0:  # low limbs zero: the fold's carry ripples through 2..15 all-ones limbs
        return 1 << (32 * (2 + (ei // 4) % 14))
    if sel == 1:  # bits 512..520 set
        return (0x1FF << 512) | (pool[ei % len(pool)] & ((1 << 512) - 1) & ~M32) | 0x10
    if sel == 2:  # 0: F is a multiple of p
        return 0
    return ((pool[ei % len(pool)] | 1) << 32) & P  # limb 0 zero, limb 1 odd: the carry stops in limb 1


class SplitCase:
    """Secrets and coefficients of one (t, n, N) split on the layout.

    Random positions hold seeded random secrets and coefficients.  An edge
    position either takes its coefficients from the pool in pairs whose sums
    and small multiples cross limb boundaries (c and p - c, p - c +- 1, all
    p - 1, all p), or takes c_2.. from the pool and has c_1 SOLVED so that
    F(x*) = sum_j c_j x*^j lands on a chosen residue at a target share x*
    (then F's fold carries out of limb 0, or has its top bits set, or F is a
    multiple of p).  Lone edge lanes are always solved, one class each."""

    def __init__(self, t: int, n: int, N: int = N_LAYOUT, fe: bool = False, seed: int = 11):
        self.t, self.n, self.N, self.fe = t, n, N, fe
        pool, rng = _edge_values(), random.Random(seed * 1000003 + 131 * t + n)
        self.kinds = layout_kinds(N)
        u64_edges = [0, 1, M64, 1 << 63, (1 << 63) - 1, M32, 1 << 32, M64 - 1]
        rows, ei, lone = [], 0, 0
        for i, kind in enumerate(self.kinds):
            rsec = rand_fe(rng) if fe else rng.getrandbits(64)
            rco = [rand_fe(rng) for _ in range(t - 1)]
            if kind == "R":
                rows.append([rsec] + rco)
                continue
            sec = pool[(7 * ei + 3) % len(pool)] if fe else u64_edges[ei % len(u64_edges)]
            co = [pool[(13 * ei + 5 * j) % len(pool)] for j in range(t - 1)]
            if kind == "L":
                solve, sel = True, lone % 4
                lone += 1
            else:
                solve, sel = ei % 2 == 0, (ei // 2) % 4
            if t >= 2 and solve:
                # a late share: F(x*) >= 2^521 there, so the fold has a high part to add
                xs = n - (ei // 8) % min(n, 3)
                if xs == 1 and n > 1:
                    xs = n
                for alt in range(8):  # (a secret for which x* divides the target leaves F(x*) = target: next one)
                    sec = pool[(7 * ei + 3 + alt) % len(pool)] if fe else u64_edges[(ei + alt) % len(u64_edges)]
                    rest = split_unreduced([sec, 0] + co[1:], xs)
                    co[0] = (_targets(ei, sel) - rest) * pow(xs, -1, P) % P
                    if sel in (1, 2) or (pred_carry_multi if sel == 0 else pred_carry0)(split_unreduced([sec] + co, xs)):
                        break
                else:
                    # (many coefficients: F >> 521 is wider than a limb and the residue does not fix F's low
                    # limbs)  steer the secret's low 64 bits instead: F(x*) ends in 64 one bits
                    co[0] = pool[(7 * ei) % len(pool)]
                    sec -= sec & M64
                    sec |= (M64 - split_unreduced([sec] + co, xs)) & M64
            elif t >= 2:
                c, m = pool[(17 * ei + 2) % len(pool)], (ei // 2) % 5
                if m == 3:
                    co = [P - 1] * (t - 1)
                elif m == 4:
                    co = [P] * (t - 1)
                else:
                    other = min(P, max(0, P - c + (0, 1, -1)[m]))
                    co = [c if j % 2 == 0 else other for j in range(t - 1)]
            rows.append([sec] + co)
            ei += 1
        self.rows = rows  # per element: [c_0 (the secret), c_1, ..., c_{t-1}]

    def secrets(self) -> List[int]:
        return [r[0] for r in self.rows]

    def coeffs(self, j: int) -> List[int]:
        return [r[j] for r in self.rows]

    def unreduced(self, x: int) -> List[int]:
        return [split_unreduced(r, x) for r in self.rows]

    def expected(self, x: int) -> List[int]:
        return [split_unreduced(r, x) % P for r in self.rows]


@functools.lru_cache(maxsize=8)
def split_case(t: int, n: int, N: int = N_LAYOUT, fe: bool = False) -> SplitCase:
    return SplitCase(t, n, N, fe)


# (t, n) of every int64-secret split the GPU file runs on the layout, and of the
# field-secret ones.  t = 1 has no coefficient: F = the 64-bit secret, nothing folds.
SPLIT_U64_SHAPES = ([(t, n) for t in (1, 2, 3, 4, 6, 7) for n in (t, t + 4)] + [(5, 5), (5, 9), (3, 5)]
                    + [(4, 300), (8, 8), (9, 12), (20, 25)])
SPLIT_HORNER_SHAPES = [(2, 3), (3, 5), (5, 9)]
SPLIT_FE_SHAPES = [(2, 3), (3, 5), (5, 9), (8, 8)]


def predicate_census(case: SplitCase) -> dict:
    """name -> {"count", "full", "partial", "lone"}: over every (element,
    share) of the case, how often the predicate holds, and whether it does in
    a full tile, in the partial tile and at a lone edge lane."""
    full_end = (case.N // TILE) * TILE
    out = {name: {"count": 0, "full": False, "partial": False, "lone": False} for name in PREDICATES}
    for x in range(1, case.n + 1):
        for i, F in enumerate(case.unreduced(x)):
            if F < (1 << 521) - (1 << 512) and (F & M32) + (F >> 521) <= M32:
                continue  # below every predicate (most random-lane shares of x = 1)
            for name, fn in PREDICATES.items():
                if fn(F):
                    c = out[name]
                    c["count"] += 1
                    c["full" if i < full_end else "partial"] = True
                    if case.kinds[i] == "L":
                        c["lone"] = True
    return out


# ------------------------------------------------------------------ steered secrets (fused draw + split)
def steer_secrets(coeff_rows: Sequence[Sequence[int]], n: int) -> List[int]:
    """Per element e with drawn coefficients c_1.. and target share x* = 1 + e mod n:
    the 64-bit secret that makes the low 64 bits of s + sum_j c_j x*^j all ones."""
    out = []
    for e, co in enumerate(coeff_rows):
        xs = 1 + e % n
        out.append((M64 - split_unreduced([0] + list(co), xs)) & M64)
    return out


def steered_multi_share(coeff_rows: Sequence[Sequence[int]], secrets: Sequence[int], n: int) -> float:
    """Share of elements whose F at the target share has a multi-limb carry."""
    hits = sum(pred_carry_multi(split_unreduced([s] + list(co), 1 + e % n))
               for e, (co, s) in enumerate(zip(coeff_rows, secrets)))
    return hits / max(1, len(secrets))


def to_i64(u: int) -> int:
    return u - (1 << 64) if u >> 63 else u


# ------------------------------------------------------------------ reconstruct cases
def rstar_values(d: int, shift: int) -> List[int]:
    """Residues before the division: multiples of d and their neighbours,
    limb boundaries, all-ones low limbs (the borrow chain of the exact division
    through every limb; low `shift` bits all ones for the rotation), p - 1, p - d."""
    vals = [0, 1, d - 1, d, d + 1, 2 * d, 3 * d, 7 * d, 255 * d, 65537 * d, M32, 1 << 32, P - 1, P - d, P - d - 1,
            (1 << max(shift, 1)) - 1, P - (1 << max(shift, 1))]
    vals += [(1 << (32 * j)) - 1 for j in range(1, 17)]
    vals += [((1 << (32 * j)) - 1) * d % P for j in range(1, 17)]
    vals += [((1 << (32 * j))) * d % P for j in range(1, 17)]  # u = r + m p with long zero runs
    return [v % P for v in vals]


class ReconCase:
    """k share vectors on the layout whose last share is solved so that the
    residue before the division is a chosen r* (random positions stay random)."""

    def __init__(self, a: Sequence[int], neg: int, d: int = 1, shift: int = 0, N: int = TILE + 37, seed: int = 5,
                 const_y=None):
        k = len(a)
        self.a, self.neg, self.d, self.shift, self.N, self.k = list(a), neg, d, shift, N, k
        kinds = layout_kinds(N)
        if const_y is not None:  # the accumulator bound: every share the same value
            self.ys = [[const_y] * N for _ in range(k)]
        else:
            ys = [layout_values(N, seed + i, 37 * i + 3 * len(a)) for i in range(k)]
            rs, sgn = rstar_values(d, shift), [(-1 if (neg >> i) & 1 else 1) for i in range(k)]
            if a[k - 1] % P:
                ainv, e = pow(a[k - 1], -1, P), 0
                for i in range(N):
                    if kinds[i] == "R":
                        continue
                    part = sum(sgn[j] * a[j] * ys[j][i] for j in range(k - 1))
                    ys[k - 1][i] = sgn[k - 1] * (rs[e % len(rs)] - part) * ainv % P
                    e += 1
            self.ys = ys

    def expected(self) -> List[int]:
        return [recon_expected([self.ys[j][i] for j in range(self.k)], self.a, self.neg, self.d, self.shift)
                for i in range(self.N)]


def recon_weights(A: int, k: int, seed: int) -> List[int]:
    """|a_i| of a_limbs = A for k shares: the maximum, small and seeded values."""
    rng = random.Random(1009 * A + 31 * k + seed)
    top = P - 1 if A == 17 else (1 << (32 * A)) - 1
    fixed = [top, 1, top - 1, (1 << (32 * A - 1)) if A < 17 else (1 << 520), 2, 3]
    return [fixed[i] if i < len(fixed) and i % 2 == 0 else rng.randint(1, top) for i in range(k)]


def alt_neg(k: int, phase: int = 0) -> int:
    return sum(1 << i for i in range(k) if (i + phase) % 2)


INV2_DIVISORS = (3, 5, 7, 15, 255, 257, 65521, 65535)
INV1_DIVISORS = (65537, (1 << 31) - 1, (1 << 32) - 1, 6)


def recon_cases() -> list:
    """(name, A, INV, k, d, shift, neg) of every crafted-descriptor reconstruct."""
    cases = []
    for A in (1, 2, 17):
        for INV, d in ((0, 1), (1, 65537), (2, 255)):
            cases.append((f"A{A}-inv{INV}", A, INV, 3, d, 0, alt_neg(3)))
    for k in (2, 3, 4, 5, 6, 16):  # every unrolled K and the runtime-k kernel (A = 1)
        for INV, d in ((0, 1), (1, (1 << 31) - 1), (2, 65521)):
            cases.append((f"k{k}-inv{INV}", 1, INV, k, d, 0, alt_neg(k, k)))
    for d in INV2_DIVISORS:
        cases.append((f"inv2-d{d}", 1, 2, 3, d, 0, alt_neg(3, 1)))
        cases.append((f"inv2-d{d}-A2", 2, 2, 4, d, 0, alt_neg(4)))
    for d in INV1_DIVISORS:
        cases.append((f"inv1-d{d}", 1, 1, 3, d, 0, alt_neg(3)))
        cases.append((f"inv1-d{d}-A2", 2, 1, 5, d, 0, alt_neg(5, 1)))
    for e in range(1, 32):
        cases.append((f"shift{e}", 1, 0, 3, 1, e, alt_neg(3, e)))
    for e in (1, 9, 10, 31):
        cases.append((f"shift{e}-inv1", 1, 1, 3, 65537, e, alt_neg(3)))
        cases.append((f"shift{e}-inv2", 1, 2, 3, 257, e, alt_neg(3, 1)))
        cases.append((f"shift{e}-inv2-A2", 2, 2, 2, 15, e, 1))
    return cases


def recon_case_of(spec, N: int = TILE + 37) -> ReconCase:
    _, A, _, k, d, shift, neg = spec
    return ReconCase(recon_weights(A, k, d + shift), neg, d, shift, N)


def recon_desc_of(spec, case: ReconCase):
    _, A, INV, _, d, shift, neg = spec
    return make_desc(case.a, neg, A, shift, INV, d)


def recon_many_specs() -> list:
    """A third of recon_cases() for the segmented kernel: every (A, INV) pair
    once, every K once (2..5 unrolled, 6 and 16 runtime), and the rotation's
    two arms with both divisions."""
    want = {f"A{A}-inv{INV}" for A in (1, 2, 17) for INV in (0, 1, 2)}
    want |= {"k2-inv2", "k3-inv0", "k4-inv1", "k5-inv2", "k6-inv0", "k16-inv1", "k16-inv2"}
    want |= {"shift9", "shift10", "shift31", "shift1-inv1", "shift9-inv2", "shift10-inv1", "shift31-inv2-A2",
             "inv2-d3", "inv2-d65535-A2", "inv1-d6", "inv1-d4294967295-A2"}
    out = [c for c in recon_cases() if c[0] in want]
    assert len(out) == len(want)
    return out


def ragged(values: Sequence, sizes: Sequence[int]) -> list:
    out, o = [], 0
    for s in sizes:
        out.append(values[o:o + s])
        o += s
    assert o == len(values)
    return out
