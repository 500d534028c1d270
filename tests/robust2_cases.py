"""The two-error robust reconstruct's elements (host and GPU tests), by construction: genuine sharings
with 0, 1, 2 or 3 shares moved, so the culprit byte is known and the value is the Python Lagrange
interpolant at 0 of the good shares (of all k where three are bad)."""
import functools
import math
import random

P = 2 ** 521 - 1
SETS = [(3, tuple(range(1, 8))), (5, tuple(range(1, 10))), (3, (1, 2, 4, 5, 7, 8, 11))]
N = 300  # one full 256-lane tile and a ragged one


def interpolate(xs, ys):
    return sum(y * math.prod(xj * pow(xj - xm, -1, P) for xj in xs if xj != xm) for xm, y in zip(xs, ys)) % P


def patterns(k):
    """Clean, every single share, EVERY pair i < j, one triple."""
    return [()] + [(i,) for i in range(k)] + [(i, j) for j in range(k) for i in range(j)] + [(0, k // 2, k - 1)]


def byte(bad):
    return [0xFF, bad[0] if bad else 0, 16 + bad[-1] * (bad[-1] - 1) // 2 + bad[0] if bad else 0, 0xFE][len(bad)]


def moved(y, kind, rng):
    """Share y with an error of +1, p - 1, the one that makes it 0, the one that makes it p - 1, or a random one."""
    new = [y + 1, y - 1, 0, P - 1][kind] % P if kind < 4 else y
    return new if new != y else (y + 1 + rng.randrange(P - 1)) % P


@functools.lru_cache(maxsize=None)
def block(t, xs, n=N):
    """(rows, marks, values, secrets) of n elements: element e has pattern e mod the pattern count; its error
    kinds rotate with e so that every pattern meets every kind.  Kind 5 of a pair makes S_0 vanish
    (w_i e_i + w_j e_j = 0: e_i = prod_m (x_i - x_m), e_j = -prod_m (x_j - x_m)); a triple's errors are random."""
    k, pats, rng = len(xs), patterns(len(xs)), random.Random(1000 * t + xs[-1])
    rows, marks, values = [], [], []
    for e in range(n):
        bad, kind = pats[e % len(pats)], (e // len(pats) + e % len(pats)) % 6
        f = [rng.randrange(P) for _ in range(t)]
        ys = [sum(c * x ** j for j, c in enumerate(f)) % P for x in xs]
        for s, i in enumerate(bad):
            if len(bad) == 2 and kind == 5:
                ys[i] = (ys[i] + (-1) ** s * math.prod(xs[i] - xs[m] for m in range(k) if m != i)) % P
            else:
                ys[i] = moved(ys[i], (kind + s) % 5 if len(bad) < 3 else 4, rng)
        good = [l for l in range(k) if len(bad) == 3 or l not in bad]
        rows.append(ys)
        marks.append(byte(bad))
        values.append(interpolate([xs[l] for l in good], [ys[l] for l in good]))
        assert len(bad) == 3 or values[-1] == f[0]
    return rows, marks, values
