"""Edge inputs and exact expected values for the masking path — the PCG64 /
Lemire mask kernels (csrc/mask_pcg64.hip), fix / unfix_precision and the int64
member sum (csrc/sum_i64.hip).  A helper for test_mask_edges_host.py,
test_gpu_mask_edges.py and test_gpu_agg_edges.py (no tests, no torch).

Every expectation comes from numpy itself (a Generator over a PCG64 whose
`.state` is set, `PCG64.advance`), from oracle/py_mask.py or from Python
integers, never from the library under test, and every comparison is bit for
bit.  The inputs reach what random seeds do not: a PCG64 state whose k-th raw
draw Lemire's test rejects (odds 2^-47 per draw in make_mask's range), ranges
at both ends of the 64-bit Lemire path, products x 10^p on and beside +-2^63
and beside an integer, int64 -> float64 ties.
"""
from __future__ import annotations

import functools
import random
from typing import List, Sequence, Tuple

import numpy as np

from oracle import py_mask as pm

M64, M128 = pm.M64, pm.M128
PCG_MULT = pm.PCG_MULT
PCG_MULT_INV = pow(PCG_MULT, -1, 1 << 128)
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
MERS_EXCL = (1 << 47) - 1  # make_mask: integers(0, 2**47 - 1) draws below 2^47 - 1
MERS_THRESHOLD = 1 << 17   # (2^64 - excl) % excl

# ------------------------------------------------------------------ size tables
TILE, SMALL_TILE, CHUNK = 4096, 512, 512
TILE_NS = [1, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 3 * 4096 + 5]  # lane, chunk and tile edges
LOOP_N = 70001                       # a capped grid's waves step through many tiles
GEN_COUNTS = [1, 2, 3, 16, 17]       # lone, pair, pair + odd, a full launch, two launches
CRAFT_N = 5000
CRAFT_KS = [0, 63, 64, 511, 512, 4095, 4096, 4999]
CRAFT_K_PAST = 5050                  # past the array, inside its last tile (4096- and 512-element tiles alike)
CRAFT_MS = [0, 1, MERS_THRESHOLD - 1, MERS_THRESHOLD]  # the last one is the first accepted low word
DEFAULT_GRID_WAVES = 8192 * 4        # bounded_acc_kernel: at most 8192 workgroups of 4 waves
BIG_MASK_N = (1 << 27) + 3 * TILE + 5        # > 8192 * 4 tiles: the default kernel's tile loop runs twice
SUM_NS = [1, 2, 3, 127, 128, 129, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8193]  # 64-, 512-, 2048-pair edges
SUM_KS = [1, 2, 15, 16, 17, 31, 32]
BIG_SUM_N = (1 << 25) + 4097         # > 8192 workgroups of 2048 pairs: i64_sum_kernel's stride loop runs twice
SPARSE_SEED = bytes(range(32))
SPARSE_LOW = -(1 << 62)
SPARSE_EXCLS = [(1 << 63) - (1 << 52), (1 << 63) - (1 << 49)]  # thresholds 2^53 and 2^50


def threshold(excl: int) -> int:
    """Lemire's rejection bound for draws below `excl`: (2^64 - excl) mod excl."""
    return (M64 - (excl - 1)) % excl


# ------------------------------------------------------------------ crafted PCG64 states
def crafted_x(m: int, excl: int) -> int:
    """A 64-bit x with x * excl = m (mod 2^64).  excl = 2^t o with o odd needs
    2^t | m; the answer is unique mod 2^(64 - t) and the top t bits are zero."""
    t = (excl & -excl).bit_length() - 1
    assert m % (1 << t) == 0 and 0 <= m <= M64
    mod = 1 << (64 - t)
    x = ((m >> t) * pow(excl >> t, -1, mod)) % mod
    assert (x * excl) & M64 == m
    return x


def _state_with_output(x: int) -> int:
    """A post-step state whose XSL-RR output is x: high word 1 (rotation 0), hi ^ lo = x."""
    return (1 << 64) | (x ^ 1)


def rewind(state: int, inc: int, steps: int) -> int:
    a_inv = PCG_MULT_INV
    for _ in range(steps):
        state = ((state - inc) * a_inv) & M128
    return state


def crafted_state(m: int, k: int, inc: int, excl: int = MERS_EXCL) -> Tuple[int, int]:
    """(state, inc) of a PCG64 whose raw draw k is the x with x * excl = m (mod
    2^64): Lemire's low word is m, so the draw is rejected iff m < threshold."""
    assert inc & 1
    return rewind(_state_with_output(crafted_x(m, excl)), inc, k + 1), inc


def crafted_pair_state(m1: int, m2: int, k: int, excl: int) -> Tuple[int, int]:
    """(state, inc) whose raw draws k and k + 1 have the low words m1 and m2.
    The increment is what maps the first crafted state onto the second, so the
    two x must differ in parity for it to be odd (as every PCG64 increment is)."""
    s1 = _state_with_output(crafted_x(m1, excl))
    s2 = _state_with_output(crafted_x(m2, excl))
    inc = (s2 - s1 * PCG_MULT) & M128
    assert inc & 1, "pick low words whose x differ in parity"
    return rewind(s1, inc, k + 1), inc


def some_inc(i: int) -> int:
    """A fixed odd 128-bit increment per index."""
    return random.Random(0xC0FFEE + i).getrandbits(128) | 1


# ------------------------------------------------------------------ references
def numpy_generator(state: int, inc: int) -> np.random.Generator:
    bg = np.random.PCG64(0)
    bg.state = {"bit_generator": "PCG64", "state": {"state": state, "inc": inc}, "has_uint32": 0, "uinteger": 0}
    return np.random.Generator(bg)


def numpy_integers(state: int, inc: int, low: int, high: int, n: int) -> np.ndarray:
    """Generator(PCG64 at (state, inc)).integers(low, high, n, int64): the reference draw."""
    return numpy_generator(state, inc).integers(low, high, size=n, dtype=np.int64)


def numpy_advanced(state: int, inc: int, delta: int) -> Tuple[int, int]:
    bg = np.random.PCG64(0)
    bg.state = {"bit_generator": "PCG64", "state": {"state": state, "inc": inc}, "has_uint32": 0, "uinteger": 0}
    st = bg.advance(delta).state["state"]
    return st["state"], st["inc"]


def numpy_seeded(seed) -> Tuple[int, int]:
    st = np.random.PCG64(np.random.SeedSequence(seed if isinstance(seed, int) else list(seed))).state["state"]
    return st["state"], st["inc"]


def raw_rejects(state: int, inc: int, excl: int, raw_end: int, raw_begin: int = 0) -> List[int]:
    """Raw draw indices in [raw_begin, raw_end) that Lemire's test rejects."""
    thr = threshold(excl)
    out = []
    for r in range(raw_end):
        state, x = pm.pcg64_next(state, inc)
        if r >= raw_begin and ((x * excl) & M64) < thr:
            out.append(r)
    return out


def bounded_from_state(state: int, inc: int, n: int, low: int, high: int) -> Tuple[List[int], List[int]]:
    """pm.bounded_int64 from a given state: (values, rejected raw indices)."""
    excl = high - low
    assert excl - 1 > pm.M32 and excl - 1 < M64
    thr = threshold(excl)
    out, rejects, raw = [], [], 0
    while len(out) < n:
        state, x = pm.pcg64_next(state, inc)
        m = x * excl
        if (m & M64) < thr:
            rejects.append(raw)
        else:
            out.append(low + (m >> 64))
        raw += 1
    return out, rejects


@functools.lru_cache(maxsize=None)
def sparse_rejects(excl: int, n: int) -> Tuple[int, ...]:
    """Rejected raws among those the first n elements of SPARSE_SEED's stream need."""
    st, inc = pm.pcg64_init(SPARSE_SEED)
    return tuple(bounded_from_state(st, inc, n, SPARSE_LOW, SPARSE_LOW + excl)[1])


def wrap_i64(v: int) -> int:
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def wrapping_sum(base, terms: Sequence[Tuple[np.ndarray, int]]) -> np.ndarray:
    """base + sum_j sign_j * draws_j as int64 with wrap-around (uint64 arithmetic)."""
    n = len(terms[0][0]) if terms else len(base)
    acc = np.zeros(n, dtype=np.uint64) if base is None else np.asarray(base, dtype=np.int64).view(np.uint64).copy()
    for arr, sign in terms:
        u = np.asarray(arr, dtype=np.int64).view(np.uint64)
        acc = acc + u if sign > 0 else acc - u
    return acc.view(np.int64)


def extremes_base(n: int) -> np.ndarray:
    """int64 extremes and neighbours, cycled to n elements: sums with it wrap."""
    pat = np.array([INT64_MAX, INT64_MIN, -1, 0, 1, INT64_MAX - 1, INT64_MIN + 1, 1 << 62, -(1 << 62)],
                   dtype=np.int64)
    return np.resize(pat, n)


# ------------------------------------------------------------------ fix_precision
def fix_expect(x, p: int) -> np.ndarray:
    """int64(float64(x) * 10^p) as the reference computes it on x86: numpy's
    float64 multiply, then C truncation; NaN and anything outside [-2^63, 2^63)
    give INT64_MIN.  Stated in Python integers, independent of the host's cast."""
    with np.errstate(all="ignore"):
        y = np.asarray(x).astype(np.float64) * np.float64(10 ** p)
    out = [int(v) if -9223372036854775808.0 <= v < 9223372036854775808.0 else INT64_MIN for v in y.reshape(-1).tolist()]
    return np.array(out, dtype=np.int64).reshape(y.shape)


def _ulps(x: float, k: int) -> float:
    v = np.float64(x)
    for _ in range(abs(k)):
        v = np.nextafter(v, np.float64(np.inf if k > 0 else -np.inf))
    return float(v)


@functools.lru_cache(maxsize=None)
def _fix_inputs(p: int) -> np.ndarray:
    vals = [0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308,
            0.29, -0.29, 1.15, 2.675, 0.1 + 0.2, 1.0 - 2.0 ** -53]
    rng = random.Random(1000 + p)
    scale = np.float64(10 ** p)
    for _ in range(200):  # x 10^p beside an integer: truncation shows a wrongly rounded product
        j = rng.choice((-1, 1)) * rng.getrandbits(rng.randrange(1, 63))
        x = float(np.float64(j) / scale)
        vals += [x, _ulps(x, 1), _ulps(x, -1)]
    x0 = float(np.float64(2.0 ** 63) / scale)  # x0 10^p on or beside 2^63
    for sgn in (1.0, -1.0):
        vals += [sgn * _ulps(x0, d) for d in (0, 1, -1, 2, -2)]
    vals += [float("inf"), float("-inf"), float("nan"), 1.7976931348623157e308, -1.7976931348623157e308]
    a = np.array(vals, dtype=np.float64)
    a.setflags(write=False)
    return a


def fix_cases(p: int) -> Tuple[np.ndarray, np.ndarray]:
    """(float64 inputs, expected int64) for fix_precision(., p)."""
    x = _fix_inputs(p)
    return x, fix_expect(x, p)


# ------------------------------------------------------------------ unfix_precision
@functools.lru_cache(maxsize=None)
def _unfix_inputs() -> np.ndarray:
    vals = [0, 1, -1]
    for v in ((1 << 53), (1 << 53) + 1, (1 << 53) + 3):
        vals += [v, -v]
    # float64 spacing is 1024 just below 2^63: 2^63 - 512 is a tie, 2^63 - 513 just under it
    vals += [INT64_MAX, INT64_MIN, (1 << 63) - 512, (1 << 63) - 513, -(1 << 63) + 512, -(1 << 63) + 513]
    rng = np.random.default_rng(53)
    a = np.concatenate([np.array(vals, dtype=np.int64),
                        rng.integers(INT64_MIN, INT64_MAX, size=10000, dtype=np.int64, endpoint=True)])
    a.setflags(write=False)
    return a


def unfix_cases() -> np.ndarray:
    return _unfix_inputs()


def unfix_expect(v, p: int) -> np.ndarray:
    """float64(v) / 10^p, both correctly rounded (numpy's int64 -> float64 and division)."""
    return np.asarray(v).astype(np.float64) / np.float64(10 ** p)


def bits(a: np.ndarray) -> np.ndarray:
    """float64 values as their bit patterns (so that -0.0 != 0.0 and NaN == NaN)."""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
