"""Cases and exact references for csrc/m521_device.hpp and
csrc/chacha_device.hpp, operation by operation — a helper for
test_device_ops_host.py and test_gpu_device_ops.py (no tests here).

csrc/opcheck_ops.hpp runs one case of one operation on a fixed-width record
of u32 words; this module builds the records and knows what must come back.
It is plain Python integers (and oracle.c_oracle.chacha_block for the ChaCha
keystream): nothing here calls the library or either checker.  Both checkers
get the same sections and each is compared with the references below, never
with the other.

Every precondition a header states is evaluated on the case before it is
sent (`require`): a case outside the stated domain is a bug of this file.
"""
from __future__ import annotations

import functools
import itertools
import json
import math
import os
import random
import struct
from typing import Callable, List, Optional, Sequence

import field_edges as fe
from field_edges import M32, M64, P

LAZY = 1 << 544  # the lazy form: any integer that fits 17 limbs
CANON_IN = (1 << 521) + (1 << 23)  # canon()'s domain, fold()'s range
TILE_BYTES = 66 * 256
TILE_WORDS = TILE_BYTES // 4
FD_EMIT, FD_MAX_T, MAC_ROWS = 70, 7, 16
W_SET = (0, 1, 63, 64, 255)
MAGIC = 0x504F4E44

# op -> (id, in words, out words): csrc/opcheck_ops.hpp, enum Op / in_words / out_words
_FD_IN, _FD_OUT = FD_MAX_T * 17 + 2 + FD_EMIT, TILE_WORDS + FD_EMIT * 17 + FD_MAX_T * 17
OPS = {name: (i, iw, ow) for i, (name, iw, ow) in enumerate([
    ("add_small", 18, 17), ("fold", 17, 17), ("reduce", 17, 17), ("canon", 17, 17), ("add_fe", 34, 17),
    ("twice", 17, 34), ("mul_small_add", 35, 34), ("mem_buffer", 18, TILE_WORDS + 17),
    ("mem_global", 18, TILE_WORDS + 34), ("store_reduced", 18, TILE_WORDS + 34),
    ("store_reduced_at", 18, TILE_WORDS + 34),
    ("fd2", _FD_IN, _FD_OUT), ("fd3", _FD_IN, _FD_OUT), ("fd4", _FD_IN, _FD_OUT), ("fd5", _FD_IN, _FD_OUT),
    ("fd6", _FD_IN, _FD_OUT), ("fd7", _FD_IN, _FD_OUT),
    ("mac1", 1 + MAC_ROWS * 34, 51), ("mac2", 1 + MAC_ROWS * 34, 51), ("mac17", 1 + MAC_ROWS * 34, 51),
    ("mulmod", 34, 17), ("rotr521", 18, 17), ("mod_small", 5, 1), ("exact_div_small", 39, 17),
    ("chacha_block", 13, 16), ("prng_rejected", 17, 1), ("prng_retry", 30, 17)])}


def require(cond: bool, what: str = "case outside the header's domain"):
    if not cond:
        raise AssertionError(what)


# ------------------------------------------------------------------ records
def fill(nbytes: int) -> bytes:
    """What an out record holds before the operation runs (byte b of the record)."""
    return bytes((b * 37 + 11) & 0xFF for b in range(nbytes))


def feb(v: int) -> bytes:
    return v.to_bytes(68, "little")


def u32(*xs: int) -> bytes:
    return struct.pack(f"<{len(xs)}I", *xs)


def u64(x: int) -> bytes:
    return struct.pack("<Q", x)


def fe_at(rec: bytes, word: int) -> int:
    return int.from_bytes(rec[4 * word:4 * word + 68], "little")


class Section:
    """The cases of one operation: packed in records, and a check of the out
    records.  `expected` (bytes, one whole out record per case) where the
    result is fully determined; else `verify(i, case, out_record)` returns an
    error string or None."""

    def __init__(self, name: str, op: str, cases: list, pack: Callable, expected: Optional[Callable] = None,
                 verify: Optional[Callable] = None, flags: int = 0):
        self.name, self.op, self.cases, self.flags = name, op, cases, flags
        self.op_id, self.iw, self.ow = OPS[op]
        self.verify = verify
        self.records = b"".join(pack(c) for c in cases)
        require(len(self.records) == 4 * self.iw * len(cases), f"{name}: record width")
        self.expected = b"".join(expected(c) for c in cases) if expected else None
        if expected:
            require(len(self.expected) == 4 * self.ow * len(cases), f"{name}: out record width")

    def header(self) -> bytes:
        return u32(MAGIC, self.op_id, len(self.cases), self.iw, self.ow, self.flags)

    def check(self, out: bytes, wave_rare: Optional[Sequence[bool]] = None):
        n, ob = len(self.cases), 4 * self.ow
        assert len(out) == n * ob, f"{self.name}: {len(out)} result bytes for {n} cases"
        if self.expected is not None:
            if out == self.expected:
                return
            bad = [i for i in range(n) if out[i * ob:(i + 1) * ob] != self.expected[i * ob:(i + 1) * ob]]
            i = bad[0]
            raise AssertionError(f"{self.name}: {len(bad)} of {n} cases differ, first case {i}: {self.cases[i]!r}\n"
                                 f" got  {out[i * ob:(i + 1) * ob][:96].hex()}\n"
                                 f" want {self.expected[i * ob:(i + 1) * ob][:96].hex()}")
        errs = []
        for i, c in enumerate(self.cases):
            rec = out[i * ob:(i + 1) * ob]
            e = self.verify(i, c, rec, wave_rare[i]) if wave_rare is not None else self.verify(i, c, rec)
            if e:
                errs.append((i, e))
        assert not errs, f"{self.name}: {len(errs)} of {n} cases fail, first: case {errs[0][0]} " \
                         f"{_short(self.cases[errs[0][0]])}: {errs[0][1]}"


def _short(c) -> str:
    s = repr(c)
    return s if len(s) < 400 else s[:400] + "..."


# ------------------------------------------------------------------ value pools
def limbs(v: int) -> List[int]:
    return [(v >> (32 * j)) & M32 for j in range(17)]


def ripple_len(v: int) -> int:
    """0 when the fold's add does not carry out of limb 0; else the limb the
    carry comes to rest in (1..16): it passed k - 1 all-ones limbs."""
    if not fe.pred_carry0(v):
        return 0
    body = limbs(v & P)
    k = 1
    while k < 16 and body[k] == M32:
        k += 1
    return k


@functools.lru_cache(maxsize=None)
def ripple_values() -> tuple:
    """For every k in 1..16, lazy values whose fold carries out of limb 0 and
    through exactly k limbs; limb 16 at 0x1FF among them (for k = 16 the carry
    then sets bit 521 and canon() subtracts p)."""
    rng, out = random.Random(521), []
    for k in range(1, 17):
        for hi, l0, rest_top in ((5, M32 - 2, 0x0AB), (1, M32, 0x1FF), ((1 << 23) - 1, M32, 0x1FE),
                                 ((1 << 23) - 1, 1 << 31, 0x1FF), (2, M32 - 1, 0)):
            if l0 + hi <= M32:
                continue
            L = [rng.getrandbits(32) for _ in range(17)]
            L[0] = l0
            for j in range(1, k):
                L[j] = M32
            L[16] = rest_top
            if k < 16:
                L[k] = (M32 - 1, 0, 0x7FFFFFFF, 0x80000000, 12345)[len(out) % 5]
            v = sum(x << (32 * j) for j, x in enumerate(L)) + (hi << 521)
            require(v < LAZY and ripple_len(v) == k)
            out.append(v)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def lazy_values() -> tuple:
    """Inputs of reduce / fold / store_reduced: all < 2^544."""
    pool = fe.edge_values()
    vals = list(ripple_values())
    ms = [1, 2, 3, 1 << 22, (1 << 23) - 1, 1 << 23, 4, 5, 7, 255, 256, 65535, 65537, (1 << 22) + 1, (1 << 22) - 1,
          (1 << 23) - 2, 1 << 9, 1 << 16, 0x555555, 0x2AAAAA]
    vals += [m * P for m in ms]
    vals += [LAZY - 1, P - 1, P, P + 1, CANON_IN - 1, 0, 1 << 521, (1 << 521) + 1, CANON_IN, LAZY - (1 << 521)]
    vals += pool
    # pool values under a non-zero high part, and high parts alone
    his = [1, 2, 0x1FF, 1 << 22, (1 << 23) - 1, 0x400001]
    vals += [(his[i % len(his)] << 521) | v for i, v in enumerate(pool)]
    vals += [h << 521 for h in his]
    # bits 512..520 set after the fold only (limb 16 one short, the carry completes it)
    vals += [(1 << 521) | (0x1FE << 512) | ((1 << 512) - 1), (3 << 521) | (0x1FE << 512) | ((1 << 512) - 2)]
    # ordinary lazy values (the fast path of store_reduced): seeded, limb 0 below 2^31 so the fold cannot carry
    rng = random.Random(544)
    vals += [rng.getrandbits(544) & ~(1 << 31) & ~(1 << 520) for _ in range(128)]
    seen, out = set(), []
    for v in vals:
        require(0 <= v < LAZY)
        if v not in seen:
            seen.add(v)
            out.append(v)
    return tuple(out)


def is_rare(v: int) -> bool:
    """store_reduced's own lane needs the slow path: the fold carries out of
    limb 0, or bits 512..520 are all set (without a carry the fold leaves them
    as they are, so this is the header's `top == kTopMask`)."""
    return fe.pred_carry0(v) or fe.pred_top_ones(v)


def census(values: Sequence[int]) -> dict:
    out = {name: sum(1 for v in values if fn(v)) for name, fn in fe.PREDICATES.items()}
    out["ripple"] = {k: sum(1 for v in values if ripple_len(v) == k) for k in range(1, 17)}
    return out


def canon_pool() -> List[int]:
    """Canonical residues (< p) of the edge pool."""
    return [v for v in fe.edge_values() if v < P]


def _subset(vals: Sequence[int], n: int) -> List[int]:
    """n values spread over vals, the first and last among them."""
    if len(vals) <= n:
        return list(vals)
    return [vals[i * (len(vals) - 1) // (n - 1)] for i in range(n)]


# ------------------------------------------------------------------ carry chains
def sec_add_small() -> Section:
    vs = _subset(lazy_values(), 120) + [LAZY - 1, LAZY - 2, (1 << 512) - 1, M32, (1 << 64) - 1]
    cases = [(v, s) for v in vs for s in (0, 1, 2, 0x1FF, (1 << 23) - 1, M32 - 1, M32)]
    return Section("add_small", "add_small", cases, lambda c: feb(c[0]) + u32(c[1]),
                   expected=lambda c: feb((c[0] + c[1]) % LAZY))


def sec_reduce() -> Section:
    return Section("reduce", "reduce", list(lazy_values()), feb, expected=lambda v: feb(v % P))


def sec_canon() -> Section:
    vals = [v for v in lazy_values() if v < CANON_IN]
    vals += [(1 << 521) + k for k in (2, 3, M32 >> 10, (1 << 23) - 2)] + [P - 2, P - 3]
    for v in vals:
        require(v < CANON_IN)
    return Section("canon", "canon", vals, feb, expected=lambda v: feb(v % P))


def sec_fold() -> Section:
    def verify(i, v, rec):
        got = fe_at(rec, 0)
        if got % P != v % P:
            return f"fold gives {got:#x}: not congruent"
        if got >= CANON_IN:
            return f"fold gives {got:#x} >= 2^521 + 2^23"
        if got != fe.fold_once(v):
            return f"fold gives {got:#x}, one fold is {fe.fold_once(v):#x}"
    return Section("fold", "fold", list(lazy_values()), feb, verify=verify)


def _operands() -> List[int]:
    pool = fe.edge_values()
    return pool + _subset(lazy_values(), 60)


def sec_add_fe() -> Section:
    a_s, b_s = _operands(), _subset(fe.edge_values(), 14) + [LAZY - 1 - P, (1 << 543) - 1, 1 << 543]
    cases = [(a, b) for a in a_s for b in b_s if a + b < LAZY]
    return Section("add_fe", "add_fe", cases, lambda c: feb(c[0]) + feb(c[1]), expected=lambda c: feb(c[0] + c[1]))


def sec_twice() -> Section:
    vals = [v for v in _operands() + [(1 << 543) - 1, 1 << 542, (1 << 543) - (1 << 31)] if v < (1 << 543)]
    return Section("twice", "twice", vals, feb, expected=lambda v: feb(2 * v) * 2)


MSA_X = (0, 1, 2, 3, 24, 120, 720, 5040, 65535)


def sec_mul_small_add() -> Section:
    srcs = _subset(fe.edge_values(), 48) + [(1 << 528) - 1, LAZY - 1, (1 << 543) + 12345]
    cs = _subset(fe.edge_values(), 7) + [LAZY - 1, (1 << 543) - 1]
    cases = [(s, x, c) for s in srcs for x in MSA_X for c in cs if s * x + c < LAZY]
    require(all(any(c[1] == x for c in cases) for x in MSA_X))
    return Section("mul_small_add", "mul_small_add", cases, lambda c: feb(c[0]) + u32(c[1]) + feb(c[2]),
                   expected=lambda c: feb(c[0] * c[1] + c[2]) * 2)


# ------------------------------------------------------------------ memory
def tile_with(v: int, w: int, base: bytes) -> bytearray:
    """The pre-filled tile with element w holding the 521-bit v."""
    t = bytearray(base[:TILE_BYTES])
    L = limbs(v)
    for i in range(16):
        t[1024 * i + 4 * w:1024 * i + 4 * w + 4] = struct.pack("<I", L[i])
    t[16384 + 2 * w:16384 + 2 * w + 2] = struct.pack("<H", L[16])
    return t


def _mem_section(op: str, loads: int) -> Section:
    vals = [0, 1, P - 1, P - 2, 1 << 520, (1 << 520) - 1, (1 << 512) - 1, 0x1FF << 512] + _subset(canon_pool(), 8)
    cases = [(v, w) for v in vals for w in W_SET]
    base = fill(4 * OPS[op][2])

    def expected(c):
        v, w = c
        require(v < P and w < 256)
        return bytes(tile_with(v, w, base)) + feb(v) * loads
    return Section(op, op, cases, lambda c: feb(c[0]) + u32(c[1]), expected=expected)


def sec_mem_buffer() -> Section:
    return _mem_section("mem_buffer", 1)


def sec_mem_global() -> Section:
    return _mem_section("mem_global", 2)


@functools.lru_cache(maxsize=None)
def store_reduced_layout() -> tuple:
    """(D, w) per lane, ordered by 64-lane waves: two waves with no rare lane;
    waves whose only rare lane is lane 0, lane 63, lane 29; two all-rare waves;
    then the remaining values as they come (mixed)."""
    vals = list(lazy_values())
    rare = [v for v in vals if is_rare(v)]
    calm = [v for v in vals if not is_rare(v)]
    require(len(rare) >= 3 + 128 and len(calm) >= 5 * 64)
    order, ri, ci = [], 0, 0

    def take(src, idx, k):
        return src[idx:idx + k], idx + k
    for kind in ("calm", "calm", 0, 63, 29, "rare", "rare"):
        if kind == "calm":
            blk, ci = take(calm, ci, 64)
        elif kind == "rare":
            blk, ri = take(rare, ri, 64)
        else:
            blk, ci = take(calm, ci, 63)
            one, ri = take(rare, ri, 1)
            blk = blk[:kind] + one + blk[kind:]
        order += blk
    placed = set(order)
    order += [v for v in vals if v not in placed]
    return tuple((v, W_SET[i % len(W_SET)] if i % 7 else (i * 11) % 256) for i, v in enumerate(order))


def wave_census(lay: Sequence[tuple]) -> dict:
    """How many 64-lane waves of the layout are of each kind."""
    out = {"none": 0, "all": 0, "only0": 0, "only63": 0, "only_mid": 0, "mixed": 0}
    for o in range(0, len(lay), 64):
        r = [is_rare(v) for v, _ in lay[o:o + 64]]
        if len(r) < 64:
            out["mixed"] += 1
        elif not any(r):
            out["none"] += 1
        elif all(r):
            out["all"] += 1
        elif sum(r) == 1:
            out["only0" if r[0] else "only63" if r[63] else "only_mid"] += 1
        else:
            out["mixed"] += 1
    return out


def wave_rare_of(lay: Sequence[tuple]) -> List[bool]:
    """Per lane: does any lane of its 64-lane wave need the slow path."""
    out = []
    for o in range(0, len(lay), 64):
        blk = lay[o:o + 64]
        out += [any(is_rare(v) for v, _ in blk)] * len(blk)
    return out


def sec_store_reduced(op: str = "store_reduced", flags: int = 0) -> Section:
    base = fill(4 * OPS[op][2])

    def verify(i, c, rec, wave_rare=None):
        D, w = c
        if wave_rare is None:  # one lane at a time: the lane itself, or the forced ballot
            wave_rare = is_rare(D) or bool(flags & 1)
        if rec[:TILE_BYTES] != bytes(tile_with(D % P, w, base)):
            got = tile_with(0, w, rec)  # (element w blanked: does the rest still hold the pattern)
            where = "element w" if bytes(got) == bytes(tile_with(0, w, base)) else "bytes outside element w"
            return f"tile differs from the pattern with D mod p at element {w} ({where})"
        after, back = fe_at(rec, TILE_WORDS), fe_at(rec, TILE_WORDS + 17)
        if back != D % P:
            return f"load after the store gives {back:#x}"
        if after % P != D % P or after > D:
            return f"D afterwards {after:#x}: not congruent, or larger"
        want = D % P if wave_rare else D
        if after != want:
            return f"D afterwards {after:#x}, want {want:#x} ({'slow' if wave_rare else 'fast'} path)"
    return Section(op + ("+ballot" if flags & 1 else ""), op, list(store_reduced_layout()),
                   lambda c: feb(c[0]) + u32(c[1]), verify=verify, flags=flags)


# ------------------------------------------------------------------ forward differences
def fd_xs(n: int) -> List[int]:
    """The abscissas whose share a case emits: the first 3, the last 3 and 64
    spread between (all of 1..n when n is small), ascending, 0-padded."""
    xs = {1, 2, 3, n - 2, n - 1, n} | {4 + i * (n - 7) // 63 for i in range(64)}
    xs = sorted(x for x in xs if 1 <= x <= n)
    require(len(xs) <= FD_EMIT)
    return xs + [0] * (FD_EMIT - len(xs))


def fd_rows(T: int) -> List[List[int]]:
    pool, rng = fe.edge_values(), random.Random(7000 + T)
    rows = [[P] * T, [P - 1] * T, [M64] + [P] * (T - 1), [M64] + [P - 1] * (T - 1), [0] + [P] * (T - 1)]
    rows += [[pool[(31 * r + 7 * j) % len(pool)] for j in range(T)] for r in range(5)]
    rows += [[rng.getrandbits(64)] + [rng.randint(1, P - 1) for _ in range(T - 1)] for _ in range(2)]
    return rows


def forward_difference(c: Sequence[int], k: int, x: int) -> int:
    """Delta^k f (x) of f = sum c_j X^j, as an integer."""
    return sum((-1) ** (k - i) * math.comb(k, i) * fe.split_unreduced(c, x + i) for i in range(k + 1))


def sec_fd(T: int) -> Section:
    n = fe.fd_max_n(T)
    cases = [(row, n, W_SET[i % len(W_SET)], fd_xs(n)) for i, row in enumerate(fd_rows(T))]
    base = fill(4 * _FD_OUT)

    def pack(c):
        row, n_, w, xs = c
        require(all(0 <= v < (1 << 521) for v in row) and not fe.fd_needs_fold(T, n_))
        require(fe.split_unreduced(row, n_ + 1) < LAZY, "difference table leaves the lazy bound")
        return b"".join(feb(v) for v in row) + bytes(68 * (FD_MAX_T - T)) + u32(n_, w) + u32(*xs)

    def verify(i, c, rec):
        row, n_, w, xs = c
        for e, x in enumerate(xs):
            got = fe_at(rec, TILE_WORDS + 17 * e)
            if x and got != fe.split_expected(row, x):
                return f"share at x = {x}: {got:#x}, want {fe.split_expected(row, x):#x}"
            if not x and rec[4 * (TILE_WORDS + 17 * e):4 * (TILE_WORDS + 17 * e) + 68] != \
                    base[4 * (TILE_WORDS + 17 * e):4 * (TILE_WORDS + 17 * e) + 68]:
                return f"unused share slot {e} written"
        if rec[:TILE_BYTES] != bytes(tile_with(fe.split_expected(row, n_), w, base)):
            return "tile: not the pattern with the last share at element w"
        for k in range(T):
            got, want = fe_at(rec, TILE_WORDS + 17 * (FD_EMIT + k)), forward_difference(row, k, n_ + 1)
            require(0 <= want < LAZY)
            if k == 0 and (got % P != want % P or got > want):
                return f"D[0] = {got:#x}: not congruent to f(n + 1)"
            if k and got != want:
                return f"D[{k}] = {got:#x}, the exact difference is {want:#x}"
    return Section(f"fd{T}", f"fd{T}", cases, pack, verify=verify)


# ------------------------------------------------------------------ wide accumulators
def mac_bound(A: int) -> int:
    return 1046 if A == 17 else 521 + 32 * A + 4


def sec_mac(A: int) -> Section:
    top_a, top_y = ((1 << 521) - 1 if A == 17 else (1 << (32 * A)) - 1), (1 << 521) - 1
    pool, rng = fe.edge_values(), random.Random(900 + A)
    cases = [[(top_a, top_y)] * 16, [(top_a, top_y) if i % 2 == 0 else (0, 0) for i in range(16)],
             [(top_a, 0) if i % 2 == 0 else (1, top_y) for i in range(16)],
             [(top_a, top_y) if i % 2 else (1, 1) for i in range(16)], [(0, top_y)] * 16, [(top_a, top_y)]]
    for k in (1, 2, 3, 5, 16):
        for r in range(6):
            cases.append([(pool[(17 * r + 5 * i + k) % len(pool)] & top_a if (i + r) % 3 else rng.randint(0, top_a),
                           pool[(29 * r + 11 * i + 3 * k) % len(pool)]) for i in range(k)])

    def pack(rows):
        S = sum(a * y for a, y in rows)
        require(len(rows) <= MAC_ROWS and all(a <= top_a and y < (1 << 521) for a, y in rows))
        require(S < (1 << mac_bound(A)), "sum beyond the kernels' value bound")
        body = b"".join(feb(a) + feb(y) for a, y in rows)
        return u32(len(rows)) + body + bytes(136 * (MAC_ROWS - len(rows)))

    def expected(rows):
        S = sum(a * y for a, y in rows)
        return S.to_bytes(136, "little") + feb(S % P)
    require(sum(a * y for a, y in cases[0]).bit_length() == mac_bound(A))  # the bound is met, not just respected
    return Section(f"mac{A}", f"mac{A}", cases, pack, expected=expected)


def sec_mulmod() -> Section:
    pool = canon_pool()
    require(P - 1 in pool)
    cases = list(itertools.product(pool, pool))
    return Section("mulmod", "mulmod", cases, lambda c: feb(c[0]) + feb(c[1]),
                   expected=lambda c: feb(c[0] * c[1] % P))


# ------------------------------------------------------------------ rotation
def sec_rotr() -> Section:
    vals = [1 << k for k in range(521)] + [P - 1, 0] + [v for v in canon_pool() if v.bit_count() != 1]
    cases = [(v, e) for e in range(1, 32) for v in vals]
    inv = {e: pow(1 << e, -1, P) for e in range(1, 32)}
    return Section("rotr521", "rotr521", cases, lambda c: feb(c[0]) + u32(c[1]),
                   expected=lambda c: feb(c[0] * inv[c[1]] % P))


# ------------------------------------------------------------------ small divisors
MOD_D = (1, 2, 3, 65535, 65537, 1 << 31, (1 << 32) - 1)
MOD_RANDOM_D = 300  # the random sample of divisors


def sec_mod_small() -> Section:
    rng = random.Random(64)
    ds = list(MOD_D) + [rng.getrandbits(rng.randint(2, 32)) | 1 for _ in range(MOD_RANDOM_D // 2)] + \
        [max(2, rng.getrandbits(rng.randint(2, 32))) for _ in range(MOD_RANDOM_D // 2)]
    cases = []
    for d in ds:
        require(1 <= d < (1 << 32))
        qmax = M64 // d
        xs = {0, d - 1, d, d + 1, 1 << 63, (1 << 63) - 1, M64 - d + 1, M64, M64 - 1, M32, 1 << 32, qmax * d,
              qmax * d - 1, min(M64, qmax * d + d - 1)}
        for q in (1, 2, 3, qmax // 2, qmax - 1, rng.randint(1, qmax), rng.randint(1, qmax)):
            if q >= 1:
                xs |= {q * d - 1, q * d, min(M64, q * d + d - 1)}
        xs |= {rng.getrandbits(64) for _ in range(4)}
        cases += [(x, d) for x in sorted(xs) if 0 <= x <= M64]
    return Section("mod_small", "mod_small", cases, lambda c: u64(c[0]) + u32(c[1]) + u64(M64 // c[1]),
                   expected=lambda c: u32(c[0] % c[1]))


@functools.lru_cache(maxsize=None)
def descriptor_divisors() -> tuple:
    """Every small odd d (3 <= d < 2^16) the library's small-rational
    descriptors can hold for abscissa sets within 1..16: the odd part of the
    least common denominator of the Lagrange weights at 0 (field_edges.desc_from_xs)."""
    out = set()
    for k in range(2, 17):
        for xs in itertools.combinations(range(1, 17), k):
            L = 1
            for xi in xs:
                num = den = 1
                for xj in xs:
                    if xj != xi:
                        num *= xj
                        den *= xj - xi
                dd = abs(den) // math.gcd(num, abs(den))
                L = L * dd // math.gcd(L, dd)
            d = L // (L & -L)
            if 3 <= d < 65536:
                out.add(d)
    return tuple(sorted(out))


DIV_RANDOM_R = 256  # random residues per descriptor divisor


def _div_params(d: int) -> bytes:
    """make_desc's has_inv = 2 fields, from the definitions in include/dn_shamir.h."""
    require(3 <= d < 65536 and d & 1 == 1)
    return u32(d, pow(d, -1, 1 << 32), pow(P % d, -1, d)) + u64(M64 // d) + \
        b"".join(u32(pow(2, 32 * j, d)) for j in range(17))


def sec_exact_div(which: str) -> Section:
    rng = random.Random(3 if which == "sweep" else 5)
    cases = []
    if which == "sweep":  # every odd d, eight residues each
        for d in range(3, 65536, 2):
            rs = (0, 1, d, P - d, P - 1, rng.randrange(P // d) * d, rng.randrange(P), rng.randrange(P))
            cases += [(r, d) for r in rs]
    else:
        for d in descriptor_divisors():
            cases += [(rng.randrange(P), d) for _ in range(DIV_RANDOM_R)]
    params, dinv = {}, {}

    def pack(c):
        r, d = c
        require(0 <= r < P)
        if d not in params:
            params[d], dinv[d] = _div_params(d), pow(d, -1, P)
        return feb(r) + params[d]
    return Section(f"exact_div_small-{which}", "exact_div_small", cases, pack,
                   expected=lambda c: feb(c[0] * dinv[c[1]] % P))


# ------------------------------------------------------------------ ChaCha
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _key_rec(key: bytes, nonce: int, rounds: int, ctr: int) -> bytes:
    require(len(key) == 32 and rounds in (8, 12, 20) and 0 <= ctr <= M64 and 0 <= nonce <= M64)
    return key + u64(nonce) + u32(rounds) + u64(ctr)


def _block(key: bytes, ctr: int, nonce: int, rounds: int) -> List[int]:
    from oracle import c_oracle
    return [int(x) for x in c_oracle.chacha_block(key, ctr, nonce, rounds)]


def kat_cases() -> list:
    with open(os.path.join(ROOT, "tests", "golden", "chacha_kat.json")) as f:
        kat = json.load(f)["cases"]
    out = []
    for c in kat:
        for b in range(len(c["words"]) // 16):
            out.append((bytes.fromhex(c["key"]), c["nonce"], 20, (c["counter"] + b) & M64, c["words"][16 * b:16 * b + 16]))
    return out


CHACHA_KEYS = (bytes(range(32)), bytes(32), bytes((3 + 7 * i) & 0xFF for i in range(32)))


def sec_chacha() -> Section:
    cases = kat_cases()
    n_kat = len(cases)
    for key in CHACHA_KEYS:
        for rounds in (8, 12, 20):
            for ctr in (1 << 32, M64, (1 << 63) + 1, (1 << 62) + (1 << 32) - 1, 0xDEADBEEF00000000, M32, 0):
                nonce = 0x0123456789ABCDEF ^ ctr
                cases.append((key, nonce, rounds, ctr, _block(key, ctr, nonce, rounds)))
    require(all(any(c[2] == r and c[3] >> 32 for c in cases[n_kat:]) for r in (8, 12, 20)))
    return Section("chacha_block", "chacha_block", cases, lambda c: _key_rec(c[0], c[1], c[2], c[3]),
                   expected=lambda c: u32(*c[4]))


def sec_prng_rejected() -> Section:
    cases = []
    for v in (P - 2, P - 1, P):
        cases.append(v)
        cases += [v - (1 << (32 * j)) for j in range(1, 16)]
        cases.append(v - (1 << 512))  # limb 16 at 0x1FE
    cases += [0, 1, P - 3, (1 << 520) - 1, P - 2 - (1 << 1), P ^ M32]
    for v in cases:
        require(0 <= v < (1 << 521))
    require({P - 2, P - 1, P} <= set(cases))
    return Section("prng_rejected", "prng_rejected", cases, feb, expected=lambda v: u32(1 if v >= P - 1 else 0))


RETRY_I = (0, 1, 15, 16, (1 << 32) - 1, 1 << 32, 1 << 57, (1 << 58) - 1, 1 << 58, M64)


def retry_draw(key: bytes, nonce: int, rounds: int, i: int) -> int:
    """The first redraw of coefficient i, from the rule in chacha_device.hpp's
    head comment and prng_retry: before the + 1."""
    c = ((1 << 63) + (i << 6)) & M64
    lo = _block(key, c, nonce, rounds)
    top = _block(key, (c + 1) & M64, nonce, rounds)[0] & 0x1FF
    return sum(x << (32 * j) for j, x in enumerate(lo)) | (top << 512)


def sec_prng_retry() -> Section:
    cases = []
    for kn, key in enumerate(CHACHA_KEYS):
        for rounds in (8, 20):
            for i in RETRY_I:
                nonce = (0x9E3779B97F4A7C15 * (kn + 1)) & M64
                draw = retry_draw(key, nonce, rounds, i)
                require(draw < P - 1, "the first redraw is itself rejected")
                cases.append((key, nonce, rounds, i, draw))
    return Section("prng_retry", "prng_retry", cases,
                   lambda c: _key_rec(c[0], c[1], c[2], c[3]) + feb(LAZY - 1), expected=lambda c: feb(c[4] + 1))


# ------------------------------------------------------------------ the whole list
_BUILDERS = {"add_small": sec_add_small, "fold": sec_fold, "reduce": sec_reduce, "canon": sec_canon,
             "add_fe": sec_add_fe, "twice": sec_twice, "mul_small_add": sec_mul_small_add,
             "mem_buffer": sec_mem_buffer, "mem_global": sec_mem_global,
             "store_reduced": lambda: sec_store_reduced("store_reduced"),
             "store_reduced_at": lambda: sec_store_reduced("store_reduced_at"),
             **{f"fd{T}": functools.partial(sec_fd, T) for T in range(2, 8)},
             **{f"mac{A}": functools.partial(sec_mac, A) for A in (1, 2, 17)},
             "mulmod": sec_mulmod, "rotr521": sec_rotr, "mod_small": sec_mod_small,
             "exact_div_small-sweep": lambda: sec_exact_div("sweep"),
             "exact_div_small-descriptors": lambda: sec_exact_div("descriptors"),
             "chacha_block": sec_chacha, "prng_rejected": sec_prng_rejected, "prng_retry": sec_prng_retry}


def section_names() -> List[str]:
    return list(_BUILDERS)


@functools.lru_cache(maxsize=None)
def section(name: str) -> Section:
    """One section both checkers run, built once (the host checker adds
    store_reduced with the forced ballot)."""
    sec = _BUILDERS[name]()
    require(sec.name == name)
    return sec


def sections() -> tuple:
    return tuple(section(name) for name in _BUILDERS)
