"""Edge inputs and exact expected values for the MiMC7 BN254 kernels — a
helper for test_mimc7_field_host.py and test_gpu_mimc7_edges.py (no tests).

Every reference here is oracle/py_mimc7.py (Python integers), so every
comparison is bit for bit.  The inputs are built to reach what uniformly
random field elements and N(0,1) floats do not (csrc/mimc7_field.hpp): the
limb boundaries of the 29-bit Montgomery form and of the 32-bit memory form,
all-ones limbs, round sums r + k + c_i that land exactly on 0 and on q, every
(limb, bit) placement of the double -> field conversion, its q - a branch
(|v 10^p| in (q/2, 2^253)), the truncation crossing at 2^53 and the values it
must refuse.
"""
from __future__ import annotations

import functools
import math
import random
from typing import List, Sequence

import numpy as np

from oracle import py_mimc7 as om

Q = om.Q
HALF_Q = Q // 2
R = 1 << 261  # the Montgomery radix of the 9 x 29-bit form
M29 = (1 << 29) - 1
LIMIT = 1 << 253  # the device conversion handles |v 10^p| below this


# ------------------------------------------------------------------ field pool
def limb_ones(j: int) -> int:
    """An all-ones 29-bit limb at position j."""
    return M29 << (29 * j)


@functools.lru_cache(maxsize=None)
def _field_pool() -> tuple:
    vals = [0, 1, 2, Q - 1, Q - 2, HALF_Q, HALF_Q + 1, R % Q, R * R % Q, Q - R % Q]
    ks = sorted({w * m + d for w in (29, 32) for m in range(1, 10) for d in (-1, 0, 1)})
    for k in ks:
        if k < 254:
            vals += [(1 << k) - 1, 1 << k, (1 << k) + 1, Q - (1 << k), Q - (1 << k) - 1]
    vals += [limb_ones(j) for j in range(9)]
    for c in om.CTS:
        vals.append(c)
        if c:
            vals.append(Q - c)
    rng = random.Random(254)
    vals += [rng.randrange(Q) for _ in range(20)]
    seen, out = set(), []
    for v in vals:
        if 0 <= v < Q and v not in seen:
            seen.add(v)
            out.append(v)
    return tuple(out)


def field_pool() -> List[int]:
    """Distinct integers in [0, q), in a fixed order."""
    return list(_field_pool())


def merkle_partners() -> List[int]:
    """16 fixed picks from the pool: the second leaf of every level-0 pair."""
    picks = [0, 1, 2, Q - 1, Q - 2, HALF_Q, HALF_Q + 1, R % Q, Q - R % Q, limb_ones(0), limb_ones(4), limb_ones(7),
             (1 << 232) - 1, 1 << 224, om.CTS[1], Q - om.CTS[1]]
    pool = set(_field_pool())
    assert len(set(picks)) == 16 and all(p in pool for p in picks)
    return picks


def raw_pool() -> List[int]:
    """The pool plus operands of the lazy form beyond q: anything in [0, 3q)."""
    top = 3 * Q - 1
    low_ones = (top >> 232 << 232) - 1  # the largest value below 3q whose limbs 0..7 are all ones
    assert low_ones < 3 * Q and low_ones & ((1 << 232) - 1) == (1 << 232) - 1
    return field_pool() + [Q, 2 * Q - 1, 2 * Q, 3 * Q - 1, low_ones]


# ------------------------------------------------------------------ float pools
def product(v: float, scale: float) -> float:
    """The reference's float multiply (mimc7.py:41): v * 10^p in double."""
    return float(v) * float(scale)  # (a Python float is an IEEE double; overflow gives inf, silently)


def _steps(x: float, n: int = 3) -> List[float]:
    out, lo, hi = [x], x, x
    for _ in range(n):
        lo, hi = math.nextafter(lo, -math.inf), math.nextafter(hi, math.inf)
        out += [lo, hi]
    return out


@functools.lru_cache(maxsize=None)
def _float_pool(scale: float) -> tuple:
    ys = []
    for e in range(-3, 254):
        ms = [0.5, 0.5 + 2.0 ** -53, 1.0 - 2.0 ** -53, math.pi / 4]
        if e == 253:
            ms += [0.76, 0.8, 0.9]  # above q / 2: the q - a branch
        for m in ms:
            ys += [math.ldexp(m, e), -math.ldexp(m, e)]
    ys += [2.0 ** 53 - 1, 2.0 ** 53, 2.0 ** 53 + 2, 2.0 ** 52 + 0.5, 0.99999999, 1.0, 1.5, -0.5]
    vs = [y / scale for y in ys]
    vs += _steps(HALF_Q / scale) + _steps((HALF_Q + 1) / scale)
    vs += [0.0, -0.0, 5e-324, -5e-324]
    vs += _steps(1.0 / scale, 1)  # 1e-8 (1 +- ulp) at scale 1e8: a = 0 or 1
    out = tuple(vs)
    # what the GPU tests rely on, checked on the oracle's side alone
    prods = [product(v, scale) for v in out]
    assert all(abs(p) < LIMIT for p in prods), "a pool member is outside the device conversion's range"
    exps = {math.frexp(abs(p))[1] for p in prods}
    assert all(e in exps for e in range(1, 254)), sorted(set(range(1, 254)) - exps)
    assert sum(1 for p in prods if p > 0 and int(p) > HALF_Q) >= 8
    return out


def float_pool(scale: float) -> List[float]:
    """Doubles v whose product v * scale reaches every (limb, bit) placement of
    the device float_to_field, both signs, the q - a branch and the 2^53 crossing."""
    return list(_float_pool(float(scale)))


@functools.lru_cache(maxsize=None)
def _bad_floats(scale: float) -> tuple:
    v = LIMIT / scale
    while product(v, scale) >= LIMIT:
        v = math.nextafter(v, 0.0)
    while product(v, scale) < LIMIT:
        v = math.nextafter(v, math.inf)
    below = math.nextafter(v, 0.0)
    assert product(v, scale) >= LIMIT > product(below, scale) and math.isfinite(product(v, scale))
    return (math.nan, math.inf, -math.inf, 1.7e308, v, -v), below


def bad_floats(scale: float) -> List[float]:
    """Values the device conversion must refuse at this scale: NaN, +-inf, a
    product that overflows, and the smallest v with |v * scale| >= 2^253 (+-)."""
    return list(_bad_floats(float(scale))[0])


def good_neighbour(scale: float) -> float:
    """The double just below the smallest refused one: must be accepted."""
    return _bad_floats(float(scale))[1]


# ------------------------------------------------------------------ expected values
def expected_hash(x: int, key: int) -> int:
    return om.mimc7_hash(x, key)


def expected_hash_arr(xs: Sequence[int], key: int = 2) -> int:
    return om.mimc7_hash_arr(list(xs), key)


def expected_merkle(block: Sequence[int]) -> int:
    return om.merkle(list(block), 2)


def expected_field(v: float, precision: int) -> int:
    return om.float2int(float(v), precision) % Q


def expected_row_hashes(data) -> List[int]:
    return om.data_row_hashes(data)


# ------------------------------------------------------------------ limbs
def limbs_of(vals: Sequence[int], width: int = 8) -> np.ndarray:
    """uint32 [len(vals), width], little-endian limbs."""
    return np.frombuffer(b"".join(int(v).to_bytes(4 * width, "little") for v in vals), dtype="<u4").reshape(-1, width)


def ints_of(limbs: np.ndarray) -> List[int]:
    a = np.ascontiguousarray(limbs, dtype="<u4")
    return [int.from_bytes(row.tobytes(), "little") for row in a]
