"""Tensor lists that put segment boundaries where the list kernels change
path, the substream geometry they are placed in, and an exact reference — a
helper for test_list_edges_host.py and test_gpu_list_edges.py (no tests,
importable without a device).

The fused draw + split of a list (csrc/mt19937_device.hip: emit_split_seg,
emit_pieces, the seg_find / seg_step cursor of csrc/seg_plan.hpp) runs inside
the draw's substream structure: a draw of more than 65 * 2^8 coefficients is
cut into substreams of 2^10 draws (2^12 from 2^21 coefficients, 2^14 from
2^24), and the even substreams 2 .. S - 2 run BACKWARD — their groups of 64
elements are emitted top-down and the segment cursor steps down.  The lists
here are built per threshold t so that their edges fall into chosen
substreams of that geometry; test_list_edges_host.py asserts that they do.

The reference is Python integers: the generator replayed as the reference
implementation draws (t - 1 randint(1, p - 1) per element), the polynomial
evaluated at x = 1 .. n mod p, Lagrange at zero as a linear combination.  The
field arithmetic itself is field_edges'.
"""
from __future__ import annotations

import functools
import random
from typing import List, Sequence, Set, Tuple

import field_edges as fe

P = fe.P
M64 = fe.M64
GROUP = 64  # elements per emission group (lane = element)
TILE = fe.TILE
FILL = 4097  # the filler tensor: sixteen tiles and one element
THRESHOLDS = (2, 3, 5)


# ------------------------------------------------------------------ geometry
def substream_plan(n_total: int, t: int) -> Tuple[int, int, Set[int]]:
    """(draws per substream, S, the set of backward substreams) of the draw of
    n_total * (t - 1) coefficients.  Mirrors csrc/mt_plan.hpp:
    mt_sub_len (2^8 draws up to 65 * 2^8 coefficients, else 2^10, 2^12 from
    2^21, 2^14 from 2^24), mt_subs (S), mt_levels (back = 0 at 2^8 draws, else
    1) and mt_sub_forward (backward: s even, not 0, not the last)."""
    tm1 = t - 1
    ncoef = n_total * tm1
    if ncoef <= 65 << 8:
        draws, back = 1 << 8, 0
    else:
        draws, back = (1 << 14 if ncoef >= 1 << 24 else 1 << 12 if ncoef >= 1 << 21 else 1 << 10), 1
    S = (ncoef + draws - 1) // draws
    backward = {s for s in range(S) if back and s != 0 and s % 2 == 0 and s + 1 < S}
    return draws, S, backward


def elems_per_substream(t: int, draws: int = 1 << 10) -> int:
    """E: a substream's draws / (t - 1) — 1024, 512, 256 at t = 2, 3, 5 in the 2^10 regime."""
    assert draws % (t - 1) == 0
    return draws // (t - 1)


def seg_begins(sizes: Sequence[int]) -> List[int]:
    """e_begin of every non-empty tensor, then the sentinel n_total (the kernel's table)."""
    out, e = [], 0
    for n in sizes:
        if n:
            out.append(e)
            e += n
    return out + [e]


def seg_of(begins: Sequence[int], e: int) -> int:
    """seg_find: the last k with begins[k] <= e (e < n_total)."""
    lo, hi = 0, len(begins) - 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if begins[mid] <= e:
            lo = mid
        else:
            hi = mid
    return lo


def group_segments(begins: Sequence[int], ebase: int) -> List[int]:
    """The table entries that intersect the group [ebase, min(ebase + 64, n_total))."""
    n_total = begins[-1]
    gend = min(ebase + GROUP, n_total)
    k = seg_of(begins, ebase)
    out = []
    while begins[k] < gend:
        out.append(k)
        k += 1
    return out


def single_tile(begins: Sequence[int], k: int, ebase: int) -> bool:
    """seg_single_tile of csrc/seg_plan.hpp for the group at ebase with the cursor on k."""
    n_total = begins[-1]
    return begins[k] % GROUP == 0 and (begins[k + 1] - ebase >= GROUP or begins[k + 1] == n_total)


def substream_groups(n_total: int, t: int, s: int) -> List[int]:
    """ebase of every group of substream s, in element order."""
    draws, S, _ = substream_plan(n_total, t)
    E = elems_per_substream(t, draws)
    return list(range(s * E, min((s + 1) * E, n_total), GROUP))


def piece_spans_two_tiles(begins: Sequence[int], k: int, ebase: int) -> bool:
    """seg_piece of segment k in the group at ebase: the last lane's word
    w0 + lane - lane_lo lies past tile0 (> 255)."""
    n_total = begins[-1]
    gend = min(ebase + GROUP, n_total)
    lo, hi = max(begins[k], ebase), min(begins[k + 1], gend)
    w0 = (lo - begins[k]) % TILE
    return w0 + (hi - lo - 1) > TILE - 1


# ------------------------------------------------------------------ list builders
def _fill_to_regime(sizes: List[int], t: int, tail: int = 0) -> None:
    """4097-element tensors until the list (with `tail` more elements to come)
    is past the 2^8 regime: 16640 < n_total * (t - 1)."""
    while (sum(sizes) + tail) * (t - 1) <= 16640 + 64 * (t - 1):
        sizes.append(FILL)


def _checked(sizes: List[int], t: int) -> List[int]:
    n_total = sum(sizes)
    assert 16640 < n_total * (t - 1) < 1 << 21, (n_total, t)
    draws, S, backward = substream_plan(n_total, t)
    assert draws == 1 << 10 and S >= 8 and {2, 4} <= backward
    return sizes


@functools.lru_cache(maxsize=None)
def _ones(t: int) -> tuple:
    E = elems_per_substream(t)
    sizes = [2 * E - 70]
    for i in range(1, E + 140 + 1):  # substream 2 and 70 elements either side: one-element tensors
        sizes.append(1)
        if i % 7 == 0:
            sizes.append(0)
        if i == E // 2 + 1:  # (not a multiple of 7: exactly two empties in a row)
            sizes += [0, 0]
    assert (E // 2 + 1) % 7 != 0
    tail = [1, 0, 1, 2, 1]
    _fill_to_regime(sizes, t, sum(tail))
    if (sum(sizes) + sum(tail)) % GROUP < 5:  # the tail's five elements in the last, partial group
        sizes.append(37)
    sizes += tail
    assert 5 <= sum(sizes) % GROUP <= 63
    return tuple(_checked(sizes, t))


@functools.lru_cache(maxsize=None)
def _bounds(t: int) -> tuple:
    E = elems_per_substream(t)
    sizes = [2 * E - 1, 1, 1]  # cuts at 2E - 1, 2E, 2E + 1
    for _ in (3, 4, 5):  # ... and at kE - 1, kE, kE + 1
        sizes += [E - 2, 1, 1]
    tail = [300, 1, 63, 7]
    _fill_to_regime(sizes, t, sum(tail))
    return tuple(_checked(sizes + tail, t))


@functools.lru_cache(maxsize=None)
def _sixtyfours(t: int) -> tuple:
    E = elems_per_substream(t)
    sizes = [2 * E]
    for i in range(3 * E // GROUP):  # substreams 2, 3 and 4: one 64-element tensor per group
        if i:
            sizes.append(0)
        sizes.append(GROUP)
    sizes.append(192)
    _fill_to_regime(sizes, t)
    if sum(sizes) % GROUP:
        sizes.append(GROUP - sum(sizes) % GROUP)
    assert sum(sizes) % GROUP == 0
    return tuple(_checked(sizes, t))


@functools.lru_cache(maxsize=None)
def _straddle(t: int) -> tuple:
    E = elems_per_substream(t)
    sizes = [3]
    while sum(sizes) < 6 * E:  # through substreams 0 .. 5
        sizes += [256, 257, 511, 513, 1000]
    _fill_to_regime(sizes, t)
    return tuple(_checked(sizes, t))


@functools.lru_cache(maxsize=None)
def _empty_ends(t: int) -> tuple:
    E = elems_per_substream(t)
    return tuple(_checked([0, 0, 9 * E + 37, 0, 0, 8 * E + 101, 0], t))


@functools.lru_cache(maxsize=None)
def _single(t: int) -> tuple:
    return tuple(_checked([17 * elems_per_substream(t) + 77], t))


BUILDERS = {"ONES": _ones, "BOUNDS": _bounds, "SIXTYFOURS": _sixtyfours, "STRADDLE": _straddle,
            "EMPTY_ENDS": _empty_ends, "SINGLE": _single}
MAIN_LISTS = ("ONES", "BOUNDS", "SIXTYFOURS", "STRADDLE")


def build(name: str, t: int) -> List[int]:
    return list(BUILDERS[name](t))


def big_list() -> List[int]:
    """t = 5, n_total = 2^19 + 77: 2^21 + 308 coefficients, the 2^12-draw
    length (E = 1024), with the ONES structure over substream 2 and the BOUNDS
    cuts at 4E and 5E."""
    E, n_total = 1024, (1 << 19) + 77
    sizes = list(_ones(2)[:_ones(2).index(FILL)])  # (t = 2 has E = 1024 too) up to 3E + 70
    assert sum(sizes) == 3 * E + 70
    sizes += [E - 71, 1, 1, E - 2, 1, 1]  # cuts at 4E - 1, 4E, 4E + 1, 5E - 1, 5E, 5E + 1
    while sum(sizes) + FILL + 5 <= n_total:
        sizes.append(FILL)
    sizes += [n_total - sum(sizes) - 5, 1, 0, 1, 2, 1]
    assert sum(sizes) == n_total and min(sizes) >= 0
    assert substream_plan(n_total, 5) == (1 << 12, 513, set(range(2, 512, 2)))
    return sizes


# ------------------------------------------------------------------ the reference
def replayed(seed: int, pre: int = 0) -> random.Random:
    """A generator seeded as the caller's, `pre` 32-bit words drawn from it."""
    r = random.Random(seed)
    if pre:
        r.getrandbits(32 * pre)
    return r


def draw_rows(r: random.Random, n_total: int, tm1: int) -> List[List[int]]:
    """Per element its t - 1 coefficients, drawn as the reference draws them."""
    return [[r.randint(1, P - 1) for _ in range(tm1)] for _ in range(n_total)]


def to_field(secret: int) -> int:
    """An int64 secret as make_shares_vec maps it: its two's-complement 64 bits."""
    return secret & M64


def split_reference(secrets: Sequence[int], sizes: Sequence[int], t: int, n: int, r: random.Random):
    """shares[x - 1][k] = share x of tensor k's elements, for the list `sizes`
    of int64 `secrets` (concatenated), drawing from r (which advances)."""
    assert len(secrets) == sum(sizes)
    rows = draw_rows(r, len(secrets), t - 1)
    polys = [[to_field(int(s))] + co for s, co in zip(secrets, rows)]
    out = []
    for x in range(1, n + 1):
        flat = [fe.split_expected(c, x) for c in polys]
        out.append(fe.ragged(flat, sizes))
    return out


def lagrange_reference(ys: Sequence[Sequence[int]], xs: Sequence[int]) -> List[int]:
    """sum_i lambda_i y_i mod p per element, for ANY y values (a linear map:
    the rows need not be shares of one polynomial)."""
    lam = fe.lagrange_at_zero(xs)
    return [sum(l * y for l, y in zip(lam, col)) % P for col in zip(*ys)]
