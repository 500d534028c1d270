"""random.Random states whose 521-bit draws carry chosen values — a helper for
test_mt_edges_host.py and test_gpu_mt_edges.py (no tests, pure Python: no
device, no native library).

The reference draws every coefficient as randint(1, p - 1) = 1 +
getrandbits(521), redrawn while the raw value is >= p - 1
(delta_node/crypto/shamir/shamir.py:59-61).  On random states the redraw has
odds of ~2^-520 per draw, so neither the device's rejection predicate
(csrc/mt19937_device.hip: emit_group, emit_prepare), nor the host redraw
(csrc/host_m521.cpp: ge_p_minus_1), nor the carry chain of the + 1 at its
edges is ever met by a seeded generator.  MT19937's word recurrence runs
backwards, so a state can be built whose D-th draw has any 17 words wanted:

  x[k + 624] = x[k + 397] ^ (y >> 1) ^ (y odd ? A : 0),
  y = (x[k] & 2^31) | (x[k + 1] & (2^31 - 1))

A's top bit is set and y >> 1's is clear, so t = x[k + 624] ^ x[k + 397] gives
y's low bit (t's top bit) and then y itself: x[k]'s top bit and x[k + 1]'s low
31 bits.  craft_state writes the chosen words, untempered, at the end of a
624-word window of seeded words and steps that window back to the caller's
array; CPython alone then checks the state (an assertion, in craft_state) and
computes every expected value (`draw`, `reference`).
"""
from __future__ import annotations

import random
from typing import Dict, List, Sequence, Tuple, Union

P = (1 << 521) - 1
ONES = (1 << 521) - 1  # the largest raw draw (= p)
M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
WORDS = 17  # MT19937 words per getrandbits(521)
N, M = 624, 397
A, UP, LO = 0x9908B0DF, 0x80000000, 0x7FFFFFFF
MAX_CLUSTER = 36  # draws: 612 words fit in one 624-word window

Draw = Union[int, Tuple[int, int]]  # a raw 521-bit value, or (value, low 23 bits of its 17th word)


# ------------------------------------------------------------------ the generator, backwards
def temper(y: int) -> int:
    y ^= y >> 11
    y ^= (y << 7) & 0x9D2C5680
    y ^= (y << 15) & 0xEFC60000
    y ^= y >> 18
    return y & M32


def untemper(y: int) -> int:
    """The raw state word x with temper(x) == y."""
    y ^= y >> 18
    y ^= (y << 15) & 0xEFC60000
    x = y
    for _ in range(4):  # 7 bits more per round
        x = y ^ ((x << 7) & 0x9D2C5680)
    y = x & M32
    x = y
    for _ in range(2):  # 11 bits more per round
        x = y ^ (x >> 11)
    return x & M32


def step_back(win: List[int], steps: int) -> List[int]:
    """The window `steps` words earlier in the stream: x[k .. k + 624) from
    x[k + steps .. k + steps + 624).  Each step recovers the top bit of the
    word entering at the front and the low 31 bits of the word behind it (whose
    low 31 bits no later word depends on); the low 31 bits of the final front
    word are free and stay 0."""
    buf = [0] * steps + list(win)
    for k in range(steps - 1, -1, -1):
        t = buf[k + N] ^ buf[k + M]
        if t & UP:
            y = (((t ^ A) << 1) | 1) & M32
        else:
            y = (t << 1) & M32
        buf[k] = y & UP
        buf[k + 1] = (buf[k + 1] & UP) | (y & LO)
    return buf[:N]


def draw_words(value: int, low23: int) -> List[int]:
    """The 17 tempered words getrandbits(521) assembles `value` from: 16
    little-endian words, then one whose top 9 bits are bits 512 .. 520 and whose
    low 23 bits (dropped by the >> 23) are `low23`."""
    assert 0 <= value < 1 << 521 and 0 <= low23 < 1 << 23
    return [(value >> (32 * i)) & M32 for i in range(16)] + [((value >> 512) << 23) | low23]


def _split(d: Draw, low23: int) -> Tuple[int, int]:
    return (d[0], d[1]) if isinstance(d, tuple) else (d, low23)


def craft_state(draws: Union[Dict[int, Draw], Sequence[Draw]], first_draw: int, index: int, seed,
                low23: int = 0x7FFFFF) -> tuple:
    """A random.Random.setstate argument with MT index `index` (1 .. 624) whose
    521-bit draws, counted from the caller's position, carry chosen raw values.

    draws       a list: the values of draws first_draw, first_draw + 1, ...; or
                a dict {draw number: value} (numbers >= first_draw, the
                uncrafted draws between them seeded).  A value is an int or
                (int, low 23 bits of its 17th word); `low23` serves the ints
    Everything not crafted comes from `seed`.  The crafted draws lie within
    MAX_CLUSTER consecutive draws.  The cluster may lie inside the caller's own
    array (no stepping back), straddle a 624-word regeneration, or lie any
    number of regenerations later.  The state is checked by CPython before it
    is returned."""
    assert 1 <= index <= N
    if not isinstance(draws, dict):
        draws = {first_draw + i: d for i, d in enumerate(draws)}
    assert draws and min(draws) >= first_draw >= 0
    last = max(draws)
    assert last - first_draw < MAX_CLUSTER, "the cluster must fit one 624-word window"
    # stream position of output word w (from the caller's position): index + w,
    # position 0 .. 623 being the caller's array
    end = index + WORDS * (last + 1)  # one past the cluster's last word
    q = max(0, end - N)  # the window [q, q + 624) holds the whole cluster at its end
    src = random.Random(seed)
    win = [src.getrandbits(32) for _ in range(N)]
    for d, v in draws.items():
        value, lo = _split(v, low23)
        for i, w in enumerate(draw_words(value, lo)):
            win[index + WORDS * d + i - q] = untemper(w)
    arr = step_back(win, q)
    state = (3, tuple(arr) + (index,), None)
    check_state(state, draws, low23)
    return state


def check_state(state: tuple, draws: Dict[int, Draw], low23: int) -> None:
    """CPython, forward from `state`: getrandbits(521) number d returns the
    chosen value and the 17 words are the chosen words, for every crafted d."""
    by521, by32 = random.Random(), random.Random()
    by521.setstate(state)
    by32.setstate(state)
    d0 = 0
    for d in sorted(draws):
        value, lo = _split(draws[d], low23)
        if d > d0:
            by32.getrandbits(32 * WORDS * (d - d0))  # whole words: 17 per draw skipped
            for _ in range(d - d0):
                by521.getrandbits(521)
        got = by521.getrandbits(521)
        assert got == value, f"crafted draw {d}: getrandbits(521) gives {got:#x}, wanted {value:#x}"
        words = [by32.getrandbits(32) for _ in range(WORDS)]
        assert words == draw_words(value, lo), f"crafted draw {d}: words {words}"
        d0 = d + 1


# ------------------------------------------------------------------ values
# raw draws the reference redraws: raw >= p - 1
REJECTED = [ONES, ONES - 1]

# raw draws the reference accepts, at the edges of the rejection test (one bit
# short of a rejected value in every limb class the predicate looks at), of the
# + 1 carry chain and of the 17th word's >> 23
ACCEPTED_EDGES: List[Draw] = [
    ONES - 2,                    # the largest accepted draw: coefficient p - 1
    ONES ^ (1 << (32 * 1 + 7)),  # all ones but one bit of limb 1
    ONES ^ (1 << (32 * 8 + 31)),  # ... of limb 8
    ONES ^ (1 << (32 * 15)),     # ... of limb 15
    ONES ^ (1 << 512),           # limb 16 = 0x1FE: (0x1FE << 512) | (2^512 - 1), coefficient 0x1FF << 512
    ONES ^ (1 << 520),           # limb 16 = 0x0FF
    ONES ^ 2,                    # limb 0 = 0xFFFFFFFD
    ONES ^ (1 << 31),            # limb 0 = 0x7FFFFFFF
    (1 << 512) - 1,              # the carry runs through sixteen limbs into limb 16
    0,                           # coefficient 1
    M32,                         # the carry stops in limb 1
    ((1 << 511) | 5, 0x7FFFFF),  # 17th word 0x007FFFFF: top 9 bits zero, every dropped bit set
    ((0x1FF << 512) | 0xDEADBEEF, 0),  # 17th word 0xFF800000
    (ONES ^ (1 << 300), 0),      # all ones but one bit of limb 9, dropped bits clear
]
assert len(ACCEPTED_EDGES) + 1 <= MAX_CLUSTER


def raw(d: Draw) -> int:
    return d[0] if isinstance(d, tuple) else d


assert all(raw(v) >= P - 1 for v in REJECTED) and all(raw(v) < P - 1 for v in ACCEPTED_EDGES)


# ------------------------------------------------------------------ the reference
def draw(state: tuple, n: int, tm1: int):
    """The reference's draws of n elements: randint(1, P - 1) per coefficient,
    element-major, on a random.Random set to `state`.  Returns (cols, final
    state, redrawn): cols[j][e] coefficient j + 1 of element e; redrawn is True
    when the draws consumed more than 17 * tm1 * n words."""
    rng = random.Random()
    rng.setstate(state)
    cols = [[0] * n for _ in range(tm1)]
    for e in range(n):
        for j in range(tm1):
            cols[j][e] = rng.randint(1, P - 1)
    final = rng.getstate()
    return cols, final, final != skip_state(state, WORDS * tm1 * n)


def skip_state(state: tuple, words: int) -> tuple:
    """`state` advanced by `words` 32-bit outputs (CPython's own generator)."""
    rng = random.Random()
    rng.setstate(state)
    if words:
        rng.getrandbits(32 * words)
    return rng.getstate()


def shares_of(cols: Sequence[Sequence[int]], secrets: Sequence[int], n_shares: int) -> List[List[int]]:
    """rows[x - 1][e] = secret_e + sum_j cols[j - 1][e] x^j mod P, the secret
    an int64 read as make_shares reads its 8 bytes (two's complement, unsigned)."""
    rows = []
    for x in range(1, n_shares + 1):
        row = []
        for e, s in enumerate(secrets):
            acc = 0
            for col in reversed(cols):
                acc = (acc + col[e]) * x % P
            row.append((acc + (int(s) & M64)) % P)
        rows.append(row)
    return rows


def reference(state: tuple, n: int, t: int, n_shares: int, secrets: Sequence[int]):
    """n sequential make_shares calls in plain Python: (share rows, final getstate())."""
    assert len(secrets) == n
    cols, final, _ = draw(state, n, t - 1)
    return shares_of(cols, secrets, n_shares), final


def secrets_for(n: int, seed: int = 0) -> List[int]:
    """n int64 secrets: the extremes first, then seeded values."""
    rng = random.Random(f"mt-edges-secrets-{seed}")
    edge = [0, -1, 1, (1 << 63) - 1, -(1 << 63)]
    return (edge + [rng.getrandbits(64) - (1 << 63) for _ in range(max(0, n - len(edge)))])[:n]


# ------------------------------------------------------------------ where the kernels change path
def geometry(n_elem: int, tm1: int, fused: bool):
    """(ncoef, draws per substream D, substreams S, draws per emission group G,
    backward substreams) of the device draw of n_elem * tm1 coefficients, from
    the constants the sources state: csrc/mt19937_device.hip's header comment,
    its "cutting the word stream into S substreams" sentence and its "generation
    kernel" item (substreams of 2^k whole draws; k = 14 from 2^24 coefficients,
    12 from 2^21, else 10); in csrc/mt_plan.hpp the comment over mt_sub_len (2^8
    draws up to 65 * 2^8 = 16640 coefficients), the one over mt_sub_forward
    (backward: s even, not 0, not the last) and the first comment inside
    mt_levels (2^8-draw substreams run forward only); and the comment over
    mt_gen_kernel in csrc/mt19937_device.hip (groups of 64 draws, or of 64
    elements = 64 (t - 1) draws in the fused draw + split)."""
    ncoef = n_elem * tm1
    if ncoef <= 65 << 8:
        D, back = 1 << 8, False
    else:
        D, back = (1 << 14 if ncoef >= 1 << 24 else 1 << 12 if ncoef >= 1 << 21 else 1 << 10), True
    S = (ncoef + D - 1) // D
    G = 64 * tm1 if fused else 64
    backward = [s for s in range(S) if back and s and s % 2 == 0 and s + 1 < S]
    return ncoef, D, S, G, backward


# MT index the caller's generator has in each position family (624: the array
# is used up, the first word regenerates it; else substream 0 starts inside it)
FAMILY_INDEX = {"first": 624, "first_333": 333, "first_623": 623, "group_edge": 333, "group_wrap": 624,
                "sub_edge": 624, "fwd_to_back": 100, "back_to_fwd": 624, "back_top": 333, "back_bottom": 624,
                "last": 333, "after": 624, "slots": 623}


def positions(n_elem: int, tm1: int, fused: bool = True) -> Dict[str, List[int]]:
    """Draw numbers, per family, at which the device draw of n_elem * tm1
    coefficients changes path (families a shape lacks are left out):

    first*       draw 0 (index 624; 333 and 623: substream 0 starts mid-array)
    group_edge   lane 63 of group 0 into lane 0 of group 1 (ring half 0 -> 1)
    group_wrap   lane 63 of group 1 into lane 0 of group 2 (ring half 1 -> 0)
    sub_edge     the last draw of substream 0 into the first of substream 1
    fwd_to_back  ... of substream 1 (forward) into substream 2 (backward)
    back_to_fwd  ... of substream 2 (backward) into substream 3 (forward)
    back_top     the top group of backward substream 2 (emitted first): its
                 first draw, after the last draw of the group below
    back_bottom  group 0 of substream 2 (emitted last): its last draw, before
                 the first draw of group 1
    last         the vector's last group: its first draw and the last draw
    after        draw ncoef, the first one after the vector
    slots        the tm1 coefficient slots of one element inside a group"""
    ncoef, D, S, G, backward = geometry(n_elem, tm1, fused)
    pos = {"first": [0], "first_333": [0], "first_623": [0]}

    def pair(b):  # draws b - 1 and b, both in the vector
        return [b - 1, b] if 0 < b < ncoef else None

    pos["group_edge"] = pair(G) if G < D else None
    pos["group_wrap"] = pair(2 * G) if 2 * G < D else None
    pos["sub_edge"] = pair(D) if S >= 2 else None
    if 2 in backward:
        pos["fwd_to_back"] = pair(2 * D)
        pos["back_to_fwd"] = pair(3 * D)
        pos["back_top"] = pair(3 * D - G)
        pos["back_bottom"] = pair(2 * D + G)
    k_last = (S - 1) * D  # the last substream's first draw
    g_last = k_last + (ncoef - 1 - k_last) // G * G
    pos["last"] = sorted({g_last, ncoef - 1})
    pos["after"] = [ncoef]
    e = min(70, n_elem - 1)  # lane 6 of group 1 where the vector has one
    pos["slots"] = [e * tm1 + j for j in range(tm1)]
    return {k: v for k, v in pos.items() if v}


def accepted_cluster(family: str, spots: Sequence[int], ncoef: int):
    """(first_draw, values): the ACCEPTED_EDGES cluster laid over a family's
    spots — around the last spot (seven draws before it, six after), up to the
    vector's last draw for `last`, and for `after` up to the last draw with a
    rejected value behind it at draw ncoef (never consumed)."""
    k = len(ACCEPTED_EDGES)
    if family == "after":
        return ncoef - k, list(ACCEPTED_EDGES) + [REJECTED[1]]
    if family == "last":
        return max(0, ncoef - k), list(ACCEPTED_EDGES)
    return max(0, min(spots[-1] - k // 2, ncoef - k)), list(ACCEPTED_EDGES)
