"""Edge inputs for the host byte API's big-integer arithmetic
(csrc/host_shamir.cpp) — a helper for test_bigint_edges_host.py and
test_gpu_byte_api.py (no tests, no torch).

`divmod_census` restates the library's `divmod_mag` (Knuth's algorithm D in
base 2^32) digit by digit on Python integers and reports which of its branches
a division takes.  The builders below use it to collect, from a fixed seed,
operands that reach the branches random values over the suite's moduli never
do: a second correction of the quotient estimate, an estimate of 2^32 or more,
and the add-back.  Everything is plain Python integers; the expectation of
every comparison is Python's own `divmod`, `%`, `//` and `pow(k, -1, p)`.
"""
from __future__ import annotations

import functools
import math
import random
from typing import List, Sequence, Tuple

import field_edges as fe

P = (1 << 521) - 1
B = 1 << 32
M32 = B - 1

EVENTS = ("n1", "corr0", "corr1", "corr2", "rh-break", "qh>=B", "addback", "addback-carry", "s=0", "s=31",
          "mlen=0", "q-top-zero", "r=0", "r-short")
RARE = ("corr2", "qh>=B", "addback", "addback-carry")


# ------------------------------------------------------------------ the model
def _limbs(v: int) -> List[int]:
    out = []
    while v:
        out.append(v & M32)
        v >>= 32
    return out


def _value(limbs: Sequence[int]) -> int:
    return sum(d << (32 * i) for i, d in enumerate(limbs))


def divmod_census(a: int, b: int):
    """(q, r, events) of |a| = q |b| + r as `divmod_mag` computes it, a >= 0,
    b > 0.  `events` is the set of branches taken (EVENTS; plus "a<b" for the
    early return).

    "addback-carry" is the add-back whose closing `u[j + n] += c` can be seen:
    the carry c out of the add-back is always 1 and turns the limb the
    subtraction left at 0xffffffff into 0, but a later digit never reads that
    limb again; only the remainder's shift back by s reads u[n], so the store
    matters at the last digit (j = 0) with s > 0 and nowhere else."""
    assert a >= 0 and b > 0
    ev = set()
    am, bm = _limbs(a), _limbs(b)
    if a < b:
        return 0, a, {"a<b"}
    n, mlen = len(bm), len(am) - len(bm)
    if mlen == 0:
        ev.add("mlen=0")
    if n == 1:
        ev.add("n1")
        q, rem = [0] * len(am), 0
        for i in reversed(range(len(am))):
            cur = (rem << 32) | am[i]
            q[i], rem = cur // bm[0], cur % bm[0]
        if q[-1] == 0:
            ev.add("q-top-zero")
        if rem == 0:
            ev.add("r=0")
        return _value(q), rem, ev
    s = 32 - bm[-1].bit_length()
    if s in (0, 31):
        ev.add(f"s={s}")
    v = _limbs(b << s)
    u = _limbs(a << s)
    u += [0] * (len(am) + 1 - len(u))
    assert len(v) == n and len(u) == len(am) + 1
    q = [0] * (mlen + 1)
    for j in reversed(range(mlen + 1)):
        num = (u[j + n] << 32) | u[j + n - 1]
        qh, rh = num // v[n - 1], num % v[n - 1]
        steps, broke = 0, False
        while True:
            big = qh >= B
            if big:
                ev.add("qh>=B")
            if not (big or qh * v[n - 2] > ((rh << 32) | u[j + n - 2])):
                break
            qh -= 1
            rh += v[n - 1]
            steps += 1
            if rh >= B:
                broke = True
                break
        assert steps <= 2
        ev.add(f"corr{steps}")
        if broke:
            ev.add("rh-break")
        borrow = carry = 0
        for i in range(n):
            p = qh * v[i] + carry
            carry = p >> 32
            t = u[i + j] - borrow - (p & M32)
            u[i + j] = t & M32
            borrow = 1 if t < 0 else 0
        t = u[j + n] - borrow - carry
        u[j + n] = t & M32
        if t < 0:
            ev.add("addback")
            qh -= 1
            c = 0
            for i in range(n):
                c += u[i + j] + v[i]
                u[i + j] = c & M32
                c >>= 32
            assert c == 1 and u[j + n] == M32
            u[j + n] = (u[j + n] + c) & M32
            if j == 0 and s > 0:
                ev.add("addback-carry")
        q[j] = qh
    if q[mlen] == 0:
        ev.add("q-top-zero")
    r = _value(u[:n + 1]) >> s
    assert u[n] == 0 and all(d == 0 for d in u[n + 1:])
    if r == 0:
        ev.add("r=0")
    elif len(_limbs(r)) < n:
        ev.add("r-short")
    return _value(q), r, ev


# ------------------------------------------------------------------ operands
STRUCTURED = (0, 1, 2, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF)
TOPS = (1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)
SEED = 521
TEXTBOOK = (0x7FFFFFFF_80000000_00000000_00000000, 0x80000000_00000000_00000001)


def _limb(rng: random.Random) -> int:
    return rng.choice(STRUCTURED) if rng.random() < 0.8 else rng.getrandbits(32)


def _number(rng: random.Random, n: int, top=None) -> int:
    if n == 0:
        return 0
    limbs = [_limb(rng) for _ in range(n)]
    limbs[-1] = top if top is not None else (limbs[-1] or 1)
    return _value(limbs)


def _near_multiples(rng: random.Random, b: int, extra: int) -> List[int]:
    """q b + r for r in {0, 1, b - 1, b - 2}, and each less one and less two."""
    q = _number(rng, extra + 1) if rng.random() < 0.7 else _number(rng, max(extra, 1))
    out = []
    for r in (0, 1, b - 1, b - 2):
        a = q * b + r
        out += [a, a - 1, a - 2]
    return [a for a in out if a >= 0]


def _textbook_relatives() -> List[Tuple[int, int]]:
    """The add-back vector of TAOCP 4.3.1 exercise 21 / Hacker's Delight
    `divmnu` in base 2^32, its neighbours, longer dividends, and both operands
    shifted down by 1..31 bits from one limb higher, so that the same digits
    are computed under every normalising shift s (at s > 0 the add-back at
    the last digit is the one the remainder reads back)."""
    a0, b0 = TEXTBOOK
    base = [(a0, b0), (0x80000000_00000000_00000003, 0x20000000_00000000_00000001),
            (0x80000000_FFFFFFFE_00000000, 0x80000000_0000FFFF),
            (0x7FFFFFFF_00000000_00000000, 0x80000000_00000001),
            (0xFFFFFFFE_00000000_00000000_00000000, 0xFFFFFFFF_FFFFFFFF_00000001)]
    out = []
    for a, b in base:
        for da in (0, 1, 2, -1, -2):
            for db in (0, 1, -1):
                out.append((a + da, b + db))
        out += [(a << 32, b), ((a << 32) | M32, b), (a << 64, b), (a * b0, b), (a * a0 + b - 1, b)]
        for s in range(1, 32):
            out.append(((a << 32) >> s, (b << 32) >> s))
            out.append((((a << 32) >> s) + 1, (b << 32) >> s))
    return out


def _candidates(rng: random.Random):
    """An endless stream of structured (a, b), b of 1..6 limbs."""
    while True:
        for n in (2, 3, 4, 5, 6):
            for top in TOPS:
                for extra in range(6):
                    b = _number(rng, n, top)
                    yield _number(rng, n + extra), b
                    for a in _near_multiples(rng, b, extra):
                        yield a, b
        for n1 in (1, 2, 3, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, rng.getrandbits(32) | 1):
            for _ in range(6):  # the single-limb divisor loop
                yield _number(rng, rng.randrange(1, 7)), n1
                yield n1 * _number(rng, rng.randrange(1, 4)), n1
        for n in (2, 3, 4, 5, 6, 3, 4, 5, 6):  # a small top limb over a full one: the estimate is two too large
            for top in ((0x80000000,), (rng.choice((0, 1)), 1)):  # (normalised: 2^31 over 0xffffffff or ..fe)
                if n > len(top):
                    full = rng.choice((0xFFFFFFFF, 0xFFFFFFFE))
                    b = _value([_limb(rng) for _ in range(n - 1 - len(top))] + [full, *top])
                    q = _value([rng.choice((0xFFFFFFFF, 0xFFFFFFFE, 0x80000001, rng.getrandbits(32) | 1 << 31))
                                for _ in range(rng.randrange(1, 4))])
                    for r in (0, 1, b - 1, b - 2):
                        yield q * b + r, b


N_PAIRS = 5000
MIN_COUNT = 200
MIN_CARRY = 50


@functools.lru_cache(maxsize=None)
def _division() -> tuple:
    rng = random.Random(SEED)
    seen, pairs, events = set(), [], []

    def take(a, b, ev=None):
        if b <= 0 or a < 0 or (a, b) in seen:
            return
        seen.add((a, b))
        pairs.append((a, b))
        events.append(frozenset(ev if ev is not None else divmod_census(a, b)[2]))

    for a, b in _textbook_relatives():
        take(a, b)
    stream = _candidates(rng)
    while len(pairs) < N_PAIRS - MIN_CARRY:
        take(*next(stream))
    # the add-back whose carry store the remainder reads: search the same stream
    need = MIN_CARRY
    while need > 0:
        a, b = next(stream)
        if b > 0 and a >= 0 and (a, b) not in seen:
            ev = divmod_census(a, b)[2]
            if "addback-carry" in ev:
                take(a, b, ev)
                need -= 1
    return tuple(pairs), tuple(events)


def division_pairs() -> List[Tuple[int, int]]:
    """The fixed list of (a, b), a >= 0, b > 0."""
    return list(_division()[0])


def division_events() -> List[frozenset]:
    """divmod_census' events of every pair of division_pairs(), in order."""
    return list(_division()[1])


def event_counts() -> dict:
    counts = {e: 0 for e in EVENTS}
    for ev in _division()[1]:
        for e in ev:
            if e in counts:
                counts[e] += 1
    return counts


def hard_pairs() -> List[Tuple[int, int]]:
    """The pairs that reach a rare branch (RARE)."""
    pairs, events = _division()
    return [p for p, ev in zip(pairs, events) if ev & set(RARE)]


# ------------------------------------------------------------------ Euclid
N_GCD_NOT_ONE = 60


@functools.lru_cache(maxsize=None)
def _euclid() -> tuple:
    good, bad = [], []
    for a, b in hard_pairs():
        for k, p in ((b, a), (a, b)):  # first step 0 then a // b; first step a // b
            if p < 2 or k == 0:
                continue
            dst = good if math.gcd(k, p) == 1 else bad
            dst += [(k, p), (-k, p)]
    return tuple(good), tuple(bad[:: max(1, len(bad) // N_GCD_NOT_ONE)][:N_GCD_NOT_ONE])


def euclid_pairs() -> List[Tuple[int, int]]:
    """(k, p) with gcd(k, p) = 1 for `bn_inverse`: every hard (a, b) as
    (k, p) = (b, a) and (a, b), k of both signs."""
    return list(_euclid()[0])


def euclid_pairs_not_coprime() -> List[Tuple[int, int]]:
    """A smaller set with gcd(k, p) != 1: the reference's AssertionError."""
    return list(_euclid()[1])


# ------------------------------------------------------------------ primes
def is_prime(n: int) -> bool:
    """Miller-Rabin over the first 24 primes as bases, preceded by trial division."""
    small = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89)
    if n < 2:
        return False
    for q in small:
        if n % q == 0:
            return n == q
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for base in small:
        x = pow(base, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


N_PRIME_DIVISORS = 20


@functools.lru_cache(maxsize=None)
def _prime_divisors() -> tuple:
    """Prime moduli with the hard divisors' shape: the first primes at or
    above hard divisors (the divisors themselves are seldom prime), the top
    limbs and most low limbs unchanged."""
    per = N_PRIME_DIVISORS // 5  # of each length 2..6 limbs
    found, seen = {n: [] for n in range(2, 7)}, set()
    for _, b in hard_pairs():
        n = len(_limbs(b))
        if n < 2 or b in seen or len(found[n]) == per:
            continue
        seen.add(b)
        q = b | 1
        while not is_prime(q):
            q += 2
        if q >> (32 * (n - 1)) == b >> (32 * (n - 1)) and q not in found[n]:
            found[n].append(q)
    return tuple(q for n in range(2, 7) for q in found[n])


def prime_divisors() -> List[int]:
    return list(_prime_divisors())


# ------------------------------------------------------------------ inv_small
def inv_small_divisors() -> List[int]:
    """Divisors 0 < d < 2^63 for `inv_small`: m = -p^-1 mod d crosses from
    v[8] into v[9] at 2^55."""
    ds = [1, 2, 3, 1 << 31, (1 << 32) - 1, (1 << 32) + 1, (1 << 55) - 1, (1 << 55) + 1, 1 << 62, (1 << 63) - 25,
          (1 << 63) - 1, 641 * 6700417 * 3]
    assert 641 * 6700417 == (1 << 32) + 1  # (Euler's factors of F5: the divisor above is composite)
    q, found = (1 << 63) - 25, []  # 2^63 - 25 is the largest 63-bit prime
    while len(found) < 4:  # odd 63-bit primes
        q -= 2
        if is_prime(q):
            found.append(q)
    q = (1 << 62) + 1
    while len(found) < 6:
        q += 2
        if is_prime(q):
            found.append(q)
    assert len(set(ds + found)) == len(ds + found)
    return ds + found


# ------------------------------------------------------------------ the 2^63 handover
def predicts_small(xs: Sequence[int]) -> bool:
    """The rule of dn_shamir_resolve_shares_host restated: the 9-limb route is
    taken when every abscissa is a single base-2^32 limb and every partial
    product of num_i = prod (-x_j) and den_i = prod (x_i - x_j), taken in the
    library's order, stays below 2^63 in magnitude."""
    if any(x >= B for x in xs):
        return False
    lim = 1 << 63
    for i in range(len(xs)):
        num = den = 1
        for j in range(len(xs)):
            if i == j:
                continue
            num *= -xs[j]
            den *= xs[i] - xs[j]
            if not (-lim < num < lim and -lim < den < lim):
                return False
    return True


def switch_sets() -> List[Tuple[str, List[int], str]]:
    """(name, abscissas, route) on both sides of the handover; route is
    "m521" (the 9-limb form) or "bn" (the reference's sequence on BN)."""
    out = []
    for scale in (1, 3, 1 << 8, (1 << 16) + 1, (1 << 31) - 1):
        for k in range(2, 26):
            xs = [scale * i for i in range(1, k + 1)]
            out.append((f"scale{scale}-k{k}", xs))
    for x1 in (1, (1 << 63) - 2):
        for d in ((1 << 63) - 2, (1 << 63) - 1, 1 << 63, (1 << 63) + 1):
            out.append((f"pair-x{x1}-d{d}", [x1 + d, x1]))
    # the same handover below 2^32, where the rule's products decide alone
    for x0, x1 in ((M32, 1), (M32, 2), (M32 - 1, M32), (1 << 31, (1 << 31) + 1)):
        out.append((f"pair32-{x0}-{x1}", [x0, x1]))
    for xs in ([M32, M32 - 1, 2], [M32, M32 - 1, 3], [1 << 31, 1 << 31 | 1, 1], [1 << 31, 1 << 31 | 1, 2],
               [0, M32, M32 - 1, M32 - 2], [M32, M32 - 1, M32 - 2, 0]):
        out.append(("triple32-" + "-".join(map(str, xs)), xs))
    return [(name, xs, "m521" if predicts_small(xs) else "bn") for name, xs in out]


# ------------------------------------------------------------------ share records
def int_bytes(v: int) -> bytes:
    return v.to_bytes((v.bit_length() + 7) // 8, "big")


def record(xb: bytes, yb: bytes) -> bytes:
    assert len(xb) < 256
    return bytes([len(xb)]) + xb + yb


def records() -> List[Tuple[str, List[bytes]]]:
    """(name, share records): the shapes `_bytes_to_share` accepts."""
    rng = random.Random(SEED + 1)
    y = [int_bytes(rng.getrandbits(520) | 1 << 519) for _ in range(8)]
    x_of = {0: b"", 1: b"\x05", 8: b"\x80" + bytes(6) + b"\x01", 9: b"\x01" + bytes(7) + b"\x02",
            66: b"\x01" + b"\xff" * 64 + b"\xfe", 255: bytes(range(1, 256))}
    out = [("x-all-lengths", [record(x_of[n], y[i]) for i, n in enumerate(x_of)])]
    for n, xb in x_of.items():
        out.append((f"x-{n}-bytes", [record(xb, y[0]), record(b"\x03", y[1])]))
        out.append((f"x-{n}-bytes-three", [record(b"\x02", y[2]), record(xb, y[0]), record(b"\x03", y[1])]))
    out += [
        ("x-leading-zeros-equal", [record(b"\x07", y[0]), record(b"\x00\x00\x07", y[1])]),
        ("x-leading-zeros-equal-zero", [record(b"", y[0]), record(b"\x00", y[1]), record(b"\x01", y[2])]),
        ("x-leading-zeros-distinct", [record(b"\x07", y[0]), record(b"\x00\x00\x08", y[1])]),
        ("x-leading-zeros-nine-bytes", [record(bytes(8) + b"\x09", y[0]), record(b"\x08", y[1])]),
        ("x-congruent-mod-p", [record(b"\x03", y[0]), record(int_bytes(P + 3), y[1])]),
        ("x-congruent-mod-p-three", [record(b"\x03", y[0]), record(int_bytes(P + 3), y[1]), record(b"\x04", y[2])]),
        ("x-is-p", [record(int_bytes(P), y[0]), record(b"\x01", y[1])]),
        ("x-is-p-and-zero", [record(int_bytes(P), y[0]), record(b"", y[1])]),
        ("empty-record", [b"", record(b"\x01", y[0])]),
        ("empty-record-twice", [b"", b""]),
        ("empty-record-and-zero-x", [b"", record(b"", y[0])]),
        ("empty-record-three", [record(b"\x02", y[1]), b"", record(b"\x01", y[0])]),
        ("len-x-exceeds-record", [b"\x09\x01\x02", record(b"\x01", y[0])]),
        ("len-x-exceeds-record-255", [b"\xff" + y[3], record(b"\x01", y[0])]),
        ("len-x-alone", [b"\x05", record(b"\x01", y[0])]),
    ]
    for n in (0, 1, 65, 66, 67, 150, 300):
        yb = bytes([0x80 | rng.getrandbits(7)]) + bytes(rng.getrandbits(8) for _ in range(n - 1)) if n else b""
        out.append((f"y-{n}-bytes", [record(b"\x01", yb), record(b"\x02", y[0]), record(b"\x04", y[1])]))
        out.append((f"y-{n}-bytes-bn", [record(b"\x01", yb), record(int_bytes(1 << 40), y[0])]))
    out.append(("y-leading-zeros", [record(b"\x01", bytes(5) + y[0]), record(b"\x02", bytes(70) + b"\x01")]))
    for name, v in (("p", P), ("2p", 2 * P), ("p-1", P - 1), ("p+1", P + 1), ("2p+1", 2 * P + 1)):
        out.append((f"y-{name}", [record(b"\x01", int_bytes(v)), record(b"\x02", int_bytes(v))]))
        out.append((f"y-{name}-and-random", [record(b"\x03", int_bytes(v)), record(b"\x02", y[4]),
                                             record(b"\x07", y[5])]))
        out.append((f"y-{name}-bn", [record(int_bytes(1 << 64), int_bytes(v)), record(b"\x02", y[4])]))
    pool = fe.edge_values()
    for i in range(0, len(pool) - 2, 3):
        a, b, c = pool[i:i + 3]
        out.append((f"y-pool-{i}", [record(b"\x01", int_bytes(a)), record(b"\x02", int_bytes(b)),
                                    record(b"\x05", int_bytes(c))]))
    for i in range(0, len(pool) - 1, 7):
        out.append((f"y-pool-bn-{i}", [record(int_bytes((1 << 32) + 1), int_bytes(pool[i])),
                                       record(b"\x02", int_bytes(pool[i + 1]))]))
    return out
