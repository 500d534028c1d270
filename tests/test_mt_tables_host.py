"""Every row of the MT19937 jump tables against its own definition.

The device draw's bit-exactness rests on ~2900 polynomials x^J mod P: three
tables of 190 A / C / B rows (csrc/mt19937_jump.inc, mt19937_jump_short.inc),
four of 64 direct rows (mt19937_jump_direct.inc), the characteristic
polynomial P (mt19937_charpoly.inc) and the 2048 runtime direct rows the build
embeds (lib/mt_rt_rows14.bin).  A damaged row would leave the shares looking
random and only break the equality with the reference at the sizes that read
it; test_mt_levels_host.py shows that hundreds of rows are read by few sizes
or by none.

Here the committed .inc files are parsed as data (the hex words and the
`J =` comments) and checked with GF(2)[x] arithmetic on Python integers
written for this file (squaring by bit spreading, carry-less multiply, table
reduction by P): neither tools/gen_mt_jump.py nor the library's polynomial
code is used.  P is shown to be the generator's polynomial by its degree and
by annihilating a random window; one small x^J is checked against plain
stepping; then every tabulated row must equal x^J mod P for the J its position
defines (square-and-multiply from scratch, row by row), the comment must name
that J, and the embedded rows must follow D_1 = x^(L - 624), D_(s+1) = D_s x^L
with every 32nd computed from scratch as well.

The whole file takes about half a minute of one core (an exponentiation 20 to
40 ms, a multiply-and-reduce 5 ms)."""
import os
import random
import re
import struct

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "delta-node_amd", "csrc")
RT_BLOB = os.path.join(ROOT, "delta-node_amd", "lib", "mt_rt_rows14.bin")

N, M = 624, 397
DEG = 19937
WORDS = 312  # 64-bit words of a row
RT_ROWS = 2048
MASK64 = (1 << 64) - 1


# ------------------------------------------------------------------ the files as data
def parse_inc(name):
    """{macro: [(row name, J, polynomial as int)]} of a generated .inc file."""
    text = open(os.path.join(CSRC, name)).read()
    out = {}
    for m in re.finditer(r"#define (\w+) \{ \\\n(.*?)\n\}\n", text, re.S):
        rows = []
        for r in re.finditer(r"/\* (\w+): J = (\d+) \*/ \{(.*?)\}", m.group(2), re.S):
            words = re.findall(r"0x([0-9a-f]{16})ull", r.group(3))
            assert len(words) == WORDS, (name, m.group(1), r.group(1))
            rows.append((r.group(1), int(r.group(2)), sum(int(w, 16) << (64 * i) for i, w in enumerate(words))))
        out[m.group(1)] = rows
    return out


@pytest.fixture(scope="module")
def tables():
    t = {}
    for name in ("mt19937_jump.inc", "mt19937_jump_short.inc", "mt19937_jump_direct.inc", "mt19937_charpoly.inc"):
        t.update(parse_inc(name))
    assert sorted(t) == ["DN_MT_CHAR_POLY", "DN_MT_JUMP_DIRECT_L10", "DN_MT_JUMP_DIRECT_L12", "DN_MT_JUMP_DIRECT_L14",
                         "DN_MT_JUMP_DIRECT_L8", "DN_MT_JUMP_POLYS", "DN_MT_JUMP_POLYS_L10", "DN_MT_JUMP_POLYS_L12"]
    return t


# ------------------------------------------------------------------ GF(2)[x] on Python integers
SPREAD = [sum(((b >> i) & 1) << (2 * i) for i in range(8)) for b in range(256)]


def square(a: int) -> int:
    """a(x)^2: bit i moves to bit 2 i."""
    raw = a.to_bytes((a.bit_length() + 7) // 8 or 1, "little")
    return int.from_bytes(b"".join(SPREAD[b].to_bytes(2, "little") for b in raw), "little")


def clmul(a: int, b: int) -> int:
    """Carry-less product, b taken a byte at a time."""
    tab = [0] * 256
    for m in range(1, 256):
        low = m & -m
        tab[m] = tab[m ^ low] ^ (a << (low.bit_length() - 1))
    r = 0
    for i, byte in enumerate(b.to_bytes((b.bit_length() + 7) // 8 or 1, "little")):
        if byte:
            r ^= tab[byte] << (8 * i)
    return r


class Field:
    """Arithmetic mod P: the top byte of a value is cleared by one XOR of a
    tabulated multiple of P (top[t] = the multiple q P, deg q < 8, whose bits
    DEG + 7 .. DEG are t)."""

    def __init__(self, P: int):
        assert P.bit_length() - 1 == DEG
        self.P = P
        self.top = [0] * 256
        for q in range(256):
            v = clmul(P, q)
            self.top[v >> DEG] = v
        assert self.top[0] == 0 and all(self.top[t] >> DEG == t for t in range(256))

    def reduce(self, a: int) -> int:
        n = a.bit_length()
        while n > DEG + 8:
            a ^= self.top[a >> (n - 8)] << (n - 8 - DEG)
            n -= 8  # (the top byte is clear now; lower bytes may be zero too)
        while a.bit_length() > DEG:
            a ^= self.P << (a.bit_length() - 1 - DEG)
        return a

    def mul(self, a: int, b: int) -> int:
        return self.reduce(clmul(a, b))

    def xpow(self, J: int) -> int:
        """x^J mod P, square-and-multiply from the top bit of J."""
        r = 1
        for bit in bin(J)[2:]:
            r = self.reduce(square(r))
            if bit == "1":
                r <<= 1
                if r >> DEG:
                    r ^= self.P
        return r


@pytest.fixture(scope="module")
def field(tables):
    (name, J, P), = tables["DN_MT_CHAR_POLY"]
    assert name == "P" and P.bit_length() - 1 == DEG and P & 1
    return Field(P)


# ------------------------------------------------------------------ the generator, one word at a time
def step(win):
    y = (win[0] & 0x80000000) | (win[1] & 0x7FFFFFFF)
    return win[1:] + [win[M] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)]


def apply(g: int, win):
    """g(f) win by Horner, f the one-word transition."""
    r = [0] * N
    for i in range(g.bit_length() - 1, -1, -1):
        r = step(r)
        if (g >> i) & 1:
            r = [a ^ b for a, b in zip(r, win)]
    return r


def same_state(a, b):
    """Equal on the 19937 bits that matter (word 0 counts by its top bit)."""
    return a[1:] == b[1:] and (a[0] ^ b[0]) >> 31 == 0


def test_arithmetic_on_small_cases():
    """square, clmul and reduce against schoolbook bit loops on random values."""
    rnd = random.Random(1)

    def slow_mul(a, b):
        r = 0
        while b:
            if b & 1:
                r ^= a
            a <<= 1
            b >>= 1
        return r

    for bits in (1, 7, 8, 9, 64, 300, 1000):
        a, b = rnd.getrandbits(bits) | 1 << (bits - 1), rnd.getrandbits(bits)
        assert clmul(a, b) == slow_mul(a, b) and square(a) == slow_mul(a, a)
    assert square(0) == 0 and clmul(0, 5) == 0 and clmul(5, 0) == 0


def test_char_poly_annihilates_a_window(field):
    """P has degree 19937, and P(f) W = 0 on the bits that are state: words
    1 .. 623 and the top bit of word 0 (the other 31 bits of word 0 never
    enter the recurrence)."""
    rnd = random.Random(2)
    win = [rnd.getrandbits(32) for _ in range(N)]
    assert len(set(win)) == N
    out = apply(field.P, win)
    assert same_state(out, [0] * N)
    assert not same_state(apply(field.P ^ 2, win), [0] * N)  # (one coefficient off: not annihilated)


def test_small_jump_equals_plain_steps(field):
    """x^J mod P applied to a window is J steps, for a J thirty times the
    degree (a dense polynomial), and x^J is the product of two dense powers
    above the degree."""
    J = 600011
    g = field.xpow(J)
    assert g.bit_length() <= DEG and bin(g).count("1") > DEG // 3
    rnd = random.Random(3)
    win = [rnd.getrandbits(32) for _ in range(N)]
    assert len(set(win)) == N
    b = win
    for _ in range(J):
        b = step(b)
    assert same_state(apply(g, win), b)
    u, v = field.xpow(300007), field.xpow(J - 300007)
    assert min(bin(u).count("1"), bin(v).count("1")) > DEG // 3
    assert field.mul(u, v) == g == field.mul(v, u)


def expected_rows(L: int):
    """[(name, J)] of an A / C / B table for substreams of L words: A_a =
    x^(L - 624 + 64 a L) at row a, C_c = x^(4096 c L) at 63 + c, B_b = x^(b L)
    at 126 + b."""
    return ([(f"A{a}", L - N + 64 * a * L) for a in range(64)] + [(f"C{c}", 4096 * c * L) for c in range(1, 64)] +
            [(f"B{b}", b * L) for b in range(1, 64)])


def expected_direct(L: int):
    """D_s = x^(L - 624 + (s - 1) L) at row s - 1, s = 1 .. 64."""
    return [(f"D{s}", L - N + (s - 1) * L) for s in range(1, 65)]


def bad_rows(field, rows, want):
    """Names of the rows that are not x^J mod P for the J of their position
    (or whose comment names another J)."""
    assert len(rows) == len(want)
    return [name for (name, J, g), (wname, wJ) in zip(rows, want)
            if (name, J) != (wname, wJ) or g != field.xpow(wJ)]


@pytest.mark.parametrize("macro,log2", [("DN_MT_JUMP_POLYS_L10", 10), ("DN_MT_JUMP_POLYS_L12", 12), ("DN_MT_JUMP_POLYS", 14)])
def test_every_table_row_is_its_power_of_x(tables, field, macro, log2):
    assert bad_rows(field, tables[macro], expected_rows(17 << log2)) == []


@pytest.mark.parametrize("log2", [10, 12, 14, 8])
def test_every_direct_row_is_its_power_of_x(tables, field, log2):
    assert bad_rows(field, tables[f"DN_MT_JUMP_DIRECT_L{log2}"], expected_direct(17 << log2)) == []


def test_the_check_sees_one_flipped_bit(tables, field):
    """Not vacuous: one bit flipped in an odd B row of the 2^12 table (a row
    only a last window of one parity reads) is reported, and only that row."""
    rows = list(tables["DN_MT_JUMP_POLYS_L12"])
    want = expected_rows(17 << 12)
    lo, hi = 126 + 35, 126 + 40  # B_35 .. B_39
    assert rows[126 + 37 - 0][0] == "B37"
    name, J, g = rows[126 + 37]
    rows[126 + 37] = (name, J, g ^ (1 << 9001))
    assert bad_rows(field, rows[lo:hi], want[lo:hi]) == ["B37"]
    rows[126 + 37] = (name, J + 1, g)
    assert bad_rows(field, rows[lo:hi], want[lo:hi]) == ["B37"]


def rt_checksum(words):
    """mt_rt_rows_checksum (host_gf2poly.cpp) restated."""
    n = len(words)
    a, c = 0x9E3779B97F4A7C15 ^ n, 0xC2B2AE3D27D4EB4F
    for i, w in enumerate(words):
        a = ((a ^ w) * 0xFF51AFD7ED558CCD) & MASK64
        a ^= a >> 29
        c = ((((c + w) & MASK64) * 0xC4CEB9FE1A85EC53) & MASK64) ^ (c >> 31) ^ i
    return a, c


def test_embedded_runtime_rows(tables, field):
    """lib/mt_rt_rows14.bin (made by the build, embedded in the library): 2048
    rows and two checksum words; the checksum is the restated one; row s is
    D_s = x^(L - 624 + (s - 1) L) for L = 17 * 2^14 — D_1 from scratch, each
    next row the one before times x^L, every 32nd row and the last from
    scratch too — and the first 64 are the tabulated direct rows."""
    assert os.path.exists(RT_BLOB), "delta-node_amd/lib/mt_rt_rows14.bin is missing: run `make -C delta-node_amd` (the build makes and embeds it)"
    raw = open(RT_BLOB, "rb").read()
    assert len(raw) == 8 * (RT_ROWS * WORDS + 2)
    words = struct.unpack(f"<{RT_ROWS * WORDS + 2}Q", raw)
    assert rt_checksum(words[:-2]) == words[-2:]
    assert rt_checksum(words[:-3] + (words[-3] ^ 1,)) != words[-2:]
    rows = [int.from_bytes(raw[8 * WORDS * s:8 * WORDS * (s + 1)], "little") for s in range(RT_ROWS)]
    L = 17 << 14
    xL = field.xpow(L)
    assert xL == tables["DN_MT_JUMP_POLYS"][126 + 1][2]
    g = field.xpow(L - N)
    bad = []
    for s in range(1, RT_ROWS + 1):
        if rows[s - 1] != g:
            bad.append(s)
            g = rows[s - 1]  # (report a damaged row once, not every row after it)
        if s % 32 == 0 or s == RT_ROWS:
            assert g == field.xpow(L - N + (s - 1) * L), s
        g = field.mul(g, xL)
    assert bad == []
    assert rows[:64] == [g for _, _, g in tables["DN_MT_JUMP_DIRECT_L14"]]
