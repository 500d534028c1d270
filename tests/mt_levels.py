"""A plain-Python model of the device MT19937 draw's jump-level builder.

The draw's host planner, csrc/mt_plan.hpp (included by
csrc/mt19937_device.hip), turns a coefficient count into a substream length, a
substream count S and up to three jump levels; S alone decides the kind of
level, how many parts P every jump is cut into, the word ranges of the parts,
the workgroup width W (mt_jump_kernel<8> or <16>), the group size `per`, which
rows of which table are read and which window the final state is stepped from.
This module restates that arithmetic (mt_sub_len, mt_subs, mt_sub_forward,
mt_window_needed, the runtime-direct condition of mt_levels, build_levels,
push_level's P / per / W and part_cuts) for the product defaults, so that

  * test_mt_levels_host.py can pin it to the real builder (the host compile
    tools/mt_levels_check.cpp, `dump` mode), and
  * test_gpu_mt_levels.py can enumerate every distinct level shape and draw at
    each of them.

No tests here.  Job `poly` indices are the builder's: rows of the three A/C/B
tables first (table ki at ki * 190: A_a at a, C_c at 63 + c, B_b at 126 + b),
then the direct rows D_s of the four lengths (570 + 64 ki + s - 1), then the
runtime direct rows (826 + s - 1).
"""
import functools
from collections import namedtuple

LEN_LOG2 = (10, 12, 14, 8)  # draws per substream, by table index ki
TAB_LENS = 3                # lengths with A / C / B rows
RADIX = 64
POLY_WORDS = 312
ROW_A, ROW_C, ROW_B, JUMP_ROWS = 0, 63, 126, 190
DIRECT_ROWS = 64
RT_ROWS = 2048
DIRECT_BASE = TAB_LENS * JUMP_ROWS
RT_BASE = DIRECT_BASE + len(LEN_LOG2) * DIRECT_ROWS
MAX_PARTS = 32
PART_ROWS = 4096
JUMP_WAVES = 16
MT_N = 624
HEAD_BYTES = 2816
MAX_SUBS = 262145 - 1  # mt_jump_max_subs() - 1: three radix-64 digits of s - 1
MAX_COEFFS = MAX_SUBS << 14  # the largest supported draw

Level = namedtuple("Level", "name n P W per wgs grp cuts polys prow")
Plan = namedtuple("Plan", "ncoef ki draws S back rt kind levels part_rows sig")


def sub_len(ncoef: int) -> int:
    if ncoef <= (DIRECT_ROWS + 1) << 8:
        return 3
    return 2 if ncoef >= 1 << 24 else 1 if ncoef >= 1 << 21 else 0


def sub_draws(ki: int) -> int:
    return 1 << LEN_LOG2[ki]


def subs(ncoef: int) -> int:
    d = sub_draws(sub_len(ncoef))
    return (ncoef + d - 1) // d


def default_back(ki: int) -> int:
    return 0 if ki == 3 else 1


def sub_forward(s: int, S: int, back: int) -> bool:
    s &= 0xFFFFFFFF  # (uint32_t: window 1's predecessor is substream 0, never -1)
    return (not back) or s == 0 or bool(s & 1) or s + 1 >= S


def window_needed(s: int, S: int, back: int) -> bool:
    return sub_forward(s, S, back) or not sub_forward(s - 1, S, back)


def rt_level(S: int, ki: int, back: int, rt_rows: bool = True) -> bool:
    """mt_levels' condition for the one direct level through the runtime rows."""
    return rt_rows and ki == 2 and back == 1 and DIRECT_ROWS < S - 1 <= RT_ROWS


@functools.lru_cache(maxsize=None)
def part_cuts(P: int, W: int):
    r = 0.014 if W >= 16 else 0.053
    runs_total = (POLY_WORDS + 10) // 11
    T = 11
    while True:
        cut = [0]
        while cut[-1] < POLY_WORDS and len(cut) <= P:
            lo = cut[-1]
            runs = int((T - r * lo) / 11.0)
            if runs < 1:
                break
            cut.append(min(POLY_WORDS, lo + 11 * runs))
        if cut[-1] >= POLY_WORDS and len(cut) - 1 <= P:
            return tuple(cut)
        if T > 11 * runs_total + 1000:
            raise AssertionError("part_cuts: no split found")  # (the builder's unreachable branch)
        T += 1


def push_level(name, lens, polys, prow0, p_force=0, w_force=0):
    """One level from the jump counts of its sources (`lens`: (jumps, sources
    with that many) pairs) and the set of rows they read.  None for a level
    without jumps."""
    lens = [(k, c) for k, c in lens if k and c]
    n = sum(k * c for k, c in lens)
    if n == 0:
        return None
    most = max(k for k, _ in lens)
    P = max(1, min(MAX_PARTS, PART_ROWS // n))
    if p_force > 0:
        P = min(p_force, MAX_PARTS)
    per = min(JUMP_WAVES, max(2, (n * P + 255) // 256))
    W = 16 if min(per, most) > 8 else 8
    if w_force > 0:
        W = per = w_force
    groups = sum((k + per - 1) // per * c for k, c in lens)
    grp = min(per, most)
    if P == 1:
        return Level(name, n, 1, W, per, groups, grp, (0, POLY_WORDS), frozenset(polys), (0, 0))
    cuts = part_cuts(P, W)
    P = len(cuts) - 1
    return Level(name, n, P, W, per, groups * P, grp, cuts, frozenset(polys), (prow0, prow0 + n * P))


def build_levels(S: int, ki: int, back: int, rt: bool):
    """[level A-or-direct, level C, level B], None where a level has no jumps.
    back is 0 or 1 (the tuning build's probe value 2 is not modelled)."""
    if S < 2:
        return [None, None, None]
    last = S - 2
    prow0 = S + 1
    if rt or last < DIRECT_ROWS:
        base = RT_BASE if rt else DIRECT_BASE + ki * DIRECT_ROWS
        polys = [base + s - 1 for s in range(1, S) if window_needed(s, S, back)]
        return [push_level("rt" if rt else "direct", [(len(polys), 1)], polys, prow0), None, None]
    t0 = ki * JUMP_ROWS
    R = RADIX
    na = min(R, last // R + 1)
    lvA = push_level("A", [(na, 1)], range(t0 + ROW_A, t0 + ROW_A + na), prow0)
    # C: per source W(1 + 64 a) the digits c = 1 .. with 4096 c + 64 a <= last
    lens = [min(R - 1, (last - R * a) // (R * R)) for a in range(na)]
    lvC = push_level("C", [(k, 1) for k in lens], range(t0 + ROW_C + 1, t0 + ROW_C + 1 + max(lens)), prow0)
    # B: per source W(1 + base) the digits b = 1 .. 63 with base + b <= last
    # whose window is needed: all of them, or with backward generation the
    # even ones (odd windows) and the last window's
    def digits(base):
        return [b for b in range(1, min(R - 1, last - base) + 1) if window_needed(1 + base + b, S, back)]

    tail = last // R * R  # the block of the last window; the blocks before it are alike
    first, end = digits(0), digits(tail)
    lens = [(len(first), tail // R), (len(end), 1)]
    bs = set(end) | (set(first) if tail else set())
    lvB = push_level("B", lens, [t0 + ROW_B + b for b in bs], prow0)
    return [lvA, lvC, lvB]


def j0_parts() -> int:
    """Parts of the speculation's one jump to the next call's W_idx (mt_levels'
    j0: P forced to 32, four-wave workgroups): its part rows count too."""
    return len(part_cuts(MAX_PARTS, 4)) - 1


def final_sig(ncoef: int, idx: int, ki: int, S: int) -> int:
    """`sig` of mt_final_plan (csrc/mt_plan.hpp): the window CPython's final array is stepped from
    (-1: the draw ends inside the caller's array).  It is always the last
    window, S - 1 (test_mt_levels_host.py), which every draw jumps to."""
    words, h = 17 * ncoef, MT_N - idx
    if words <= h:
        return -1
    q = (words - h + MT_N - 1) // MT_N
    return min((MT_N * q + MT_N - 1 - idx) // (17 * sub_draws(ki)), S - 1)


@functools.lru_cache(maxsize=None)
def plan_for(S: int, ki: int, back: int = None, rt_rows: bool = True):
    """(back, rt, kind, levels, part_rows) of mt_levels(S, ki)."""
    if back is None:
        back = default_back(ki)
    rt = rt_level(S, ki, back, rt_rows)
    lv = build_levels(S, ki, back, rt)
    kind = "none" if S < 2 else "rt" if rt else "direct" if S - 2 < DIRECT_ROWS else "radix"
    rows = [l.prow[1] - (S + 1) for l in lv if l is not None and l.P > 1]
    if S >= 2:
        rows.append(j0_parts())
    return back, rt, kind, lv, max(rows, default=0)


def supported(S: int, ki: int) -> bool:
    """Substream counts the builder has rows for at this length."""
    return S <= (DIRECT_ROWS + 1 if ki >= TAB_LENS else MAX_SUBS)


def plan(ncoef: int, idx: int = 624, back: int = None, rt_rows: bool = True) -> Plan:
    ki = sub_len(ncoef)
    S = subs(ncoef)
    b, rt, kind, lv, part_rows = plan_for(S, ki, back, rt_rows)
    return Plan(ncoef, ki, sub_draws(ki), S, b, rt, kind, lv, part_rows, final_sig(ncoef, idx, ki, S))


def scratch_bytes(ncoef: int, back: int = None, rt_rows: bool = True) -> int:
    """dn_mt19937_device_scratch_bytes for a draw of ncoef coefficients."""
    if not ncoef:
        return HEAD_BYTES + MT_N * 4
    p = plan(ncoef, back=back, rt_rows=rt_rows)
    return HEAD_BYTES + (1 + p.S + 1 + p.part_rows) * MT_N * 4


def shape_of(ki: int, kind: str, levels) -> tuple:
    """What decides the launch sequence: (draws per substream, kind, per level
    (name, P, W, group)), group the jobs of the level's largest workgroup.
    push_level's `per` is that group size unless no source has so many jumps
    (one jump, or the few C digits of one A window); then `per` changes
    nothing in the jobs, the builder's output cannot show it, and it does not
    count as a different shape."""
    return (sub_draws(ki), kind, tuple((l.name, l.P, l.W, l.grp) for l in levels if l is not None))


def describe(ki: int, S: int, kind: str, levels) -> str:
    lv = "; ".join(f"{l.name}: n={l.n} P={l.P} W={l.W} per={l.per} group={l.grp}" for l in levels if l is not None)
    return f"2^{LEN_LOG2[ki]}-draw substreams, S={S}, {kind}" + (f" [{lv}]" if lv else "")


def s_range(lo: int, hi: int):
    """(ki, S_lo, S_hi) for each substream length with coefficient counts in
    [lo, hi]: S is monotonic in the count within one length."""
    out = []
    bounds = [(3, 1, (DIRECT_ROWS + 1) << 8), (0, ((DIRECT_ROWS + 1) << 8) + 1, (1 << 21) - 1),
              (1, 1 << 21, (1 << 24) - 1), (2, 1 << 24, MAX_SUBS << 14)]
    for ki, a, b in bounds:
        a, b = max(a, lo), min(b, hi)
        if a <= b:
            out.append((ki, subs(a), subs(b)))
    return out


@functools.lru_cache(maxsize=None)
def shapes(lo: int, hi: int, back: int = None, rt_rows: bool = True):
    """{shape: (ki, smallest S that has it)} over coefficient counts lo..hi,
    in order of substream length, then S."""
    out = {}
    for ki, s_lo, s_hi in s_range(lo, hi):
        for S in range(s_lo, s_hi + 1):
            _, _, kind, lv, _ = plan_for(S, ki, back, rt_rows)
            out.setdefault(shape_of(ki, kind, lv), (ki, S))
    return out


def covering_subs(lo: int, hi: int):
    """[(ki, S)] that between them read every row some draw of lo..hi
    coefficients reads: every S of a length with at most 8192 of them; of a
    longer range the first 4200 and the last 128.  (Beyond 66 substreams the A
    and C rows read only grow with S, the even B rows are all read, and the odd
    B row read is that of the last window, (S - 2) mod 64: 128 consecutive
    counts at the top have every residue and the largest A and C digits.)"""
    out = []
    for ki, s_lo, s_hi in s_range(lo, hi):
        if s_hi - s_lo < 8192:
            out += [(ki, S) for S in range(s_lo, s_hi + 1)]
        else:
            out += [(ki, S) for S in range(s_lo, s_lo + 4200)] + [(ki, S) for S in range(s_hi - 127, s_hi + 1)]
    return out


def rows_used(lo: int, hi: int, back: int = None, rt_rows: bool = True):
    """(used, unused): the job poly indices some draw of lo..hi coefficients
    reads, and the rest of the tables (RT_BASE + RT_ROWS indices in all)."""
    used = set()
    for ki, S in covering_subs(lo, hi):
        for l in plan_for(S, ki, back, rt_rows)[3]:
            if l is not None:
                used |= l.polys
    return used, set(range(RT_BASE + RT_ROWS)) - used


def row_name(poly: int) -> str:
    if poly >= RT_BASE:
        return f"runtime D_{poly - RT_BASE + 1}"
    if poly >= DIRECT_BASE:
        ki, s = divmod(poly - DIRECT_BASE, DIRECT_ROWS)
        return f"2^{LEN_LOG2[ki]} direct D_{s + 1}"
    ki, r = divmod(poly, JUMP_ROWS)
    name = f"A_{r}" if r < ROW_C + 1 else f"C_{r - ROW_C}" if r <= ROW_B else f"B_{r - ROW_B}"
    return f"2^{LEN_LOG2[ki]} {name}"


def coeffs_for(S: int, ki: int, full: bool) -> int:
    """Coefficient count with S substreams of length ki: the last substream
    holding one draw, or full."""
    return S * sub_draws(ki) if full else (S - 1) * sub_draws(ki) + 1
