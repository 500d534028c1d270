"""The share consistency check's reference and rows (host and GPU tests).
The reference is the DEFINITION in Python integers, not the syndrome formula:
consistent when the polynomial through the first t shares reproduces the
others; share i the culprit when the k - 1 shares without i are consistent.
"""
import random

P = (1 << 521) - 1
CONSISTENT, UNEXPLAINED = 0xFF, 0xFE

# (threshold, abscissas): r = 1, 2, 2 on a non-contiguous set, 4, 3
CASES = [(3, (1, 2, 3, 4)), (3, (1, 2, 3, 4, 5)), (3, (1, 3, 4, 7, 9)), (5, tuple(range(1, 10))), (2, (1, 2, 3, 4, 5))]
# Sets the robust planner refuses (test_share_edges_host.py asserts each property from the project's plan):
# k = 2; then r = 1, 2, 3, 4 with a syndrome weight of at least 2^31
EDGE = [(1, (1, 2)), (5, (10, 11, 24, 29, 47, 95)), (4, (9, 37, 46, 57, 79, 88)), (1, (158, 208, 231, 245)),
        (12, (2, 3, 5, 7, 8, 9, 10, 11, 13, 14, 15, 16, 17, 18, 19, 20))]


def interpolate(points, x):
    """The polynomial through `points` at x, mod P."""
    total = 0
    for i, (xi, yi) in enumerate(points):
        num = den = 1
        for m, (xm, _) in enumerate(points):
            if m != i:
                num, den = num * (x - xm) % P, den * (xi - xm) % P
        total += yi * num * pow(den, -1, P)
    return total % P


def consistent(xs, ys, t):
    head = list(zip(xs[:t], ys[:t]))
    return all(interpolate(head, x) == y % P for x, y in zip(xs[t:], ys[t:]))


def verdict(xs, ys, t):
    """The culprit byte the definition gives one element's shares."""
    xs, k = list(xs), len(xs)
    if consistent(xs, ys, t):
        return CONSISTENT
    found = [i for i in range(k) if k - t >= 2 and consistent(xs[:i] + xs[i + 1:], ys[:i] + ys[i + 1:], t)]
    return found[0] if len(found) == 1 else UNEXPLAINED


def rows(t, xs):
    """Nine genuine sharings, six of them then damaged.  Element e of a block is row e % 9: a damaged
    row lies at element 0, at both sides of every wave and tile edge and at the last element of every n."""
    rng, k = random.Random(1000 * t + len(xs) + xs[-1]), len(xs)

    def sharing(head, i=0, delta=0):  # the shares whose first t are `head`, share i then moved by delta
        ys = list(head) + [interpolate(list(zip(xs[:t], head)), x) for x in xs[t:]]
        ys[i] = (ys[i] + delta) % P
        return ys

    def head():
        return [rng.randrange(P) for _ in range(t)]

    two = sharing(head(), 0, 1)
    # two errors: no single share explains them (equal errors in a constant's shares would accuse a third)
    two[1] = (two[1] + (1 if t > 1 else 2)) % P
    return [sharing(head(), 1, 1),          # +1 in limb 0
            sharing(head(), 0, P - 1),      # -1 in the first share
            sharing(head(), 2 % k, 1 << 480),  # +1 in limb 15
            sharing(head(), k - 2, 1 << 512),  # +1 in the 9-bit top alone
            two,
            sharing(([0, P - 1] + head()[2:])[:t]),  # y = 0 and y = p - 1 among the shares (the p - y edge)
            # f = 1 + x (f = 1 at threshold 1): every syndrome is q p, q >= 1, and folds to exactly p
            [(1 + x) % P if t > 1 else 1 for x in xs],
            [(1 << 512) - (1 << 32)] * k,   # middle limbs all ones, consistent
            sharing(head(), k - 1, P - 1)]  # -1 in the last share


def negated(xs):
    """Whether share i's parity-check weight is negative: an odd number of abscissas lie above x_i."""
    return [sum(x > xi for x in xs) % 2 == 1 for xi in xs]


def edge_rows(t, xs):
    """(rows, verdicts) made for the accumulators, not for the damage: Y is y under a positive weight and
    the complement of y within 521 bits under a negated one.  A verdict of None is left to the definition."""
    neg = negated(xs)
    return ([[0 if s else P - 1 for s in neg],  # every c * Y as large as canonical shares make it: Y = p - 1 and ~0 = p
             [P - 1 if s else 0 for s in neg],  # the mirror image: Y = 0 and ~(p - 1) = 1
             [P - 1] * len(xs),                 # f = p - 1
             [P if s else 0 for s in neg],      # the non-canonical p in place of 0: every Y = 0
             [0 if s else P for s in neg]],     # ... under the other sign: every Y = p, the bound of the sums
            [None, None, CONSISTENT, CONSISTENT, CONSISTENT])
