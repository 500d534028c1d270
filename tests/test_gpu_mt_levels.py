"""The device MT19937 draw at every jump-level shape.

The substream count S alone decides how the draw's host planner
(csrc/mt_plan.hpp) builds a draw's jump levels: the kind (none, one
tabulated direct level, the runtime direct level, radix levels A / C / B), the
parts P every jump is cut into and their word ranges, the workgroup width W
(mt_jump_kernel<8> or <16>), the group size `per`, what mt_combine_kernel XORs
together, which table rows are read and which window the final state comes
from.  tests/mt_levels.py models that builder (test_mt_levels_host.py pins the
model to the real one) and lists the distinct shapes (length, kind, and per
level the parts, the waves and the largest workgroup's jobs): 60 below 2^21
coefficients (190 over every supported size).  The sizes the rest of the suite
draws at, coefficient draw or fused, reach 28 of the 190 and 20 of the 60
(from the model):

  * test_gpu_parity.py — no levels (1 substream); the direct level in groups
    of 1, 2, 4 and 8 (2^8-draw substreams: 2 .. 17, 33, 65 of them) and of 2, 3, 5
    (2^10: 17, 33, 65); A + B with B of 23 parts in 8-wave groups of 4, 5, 6
    and 8 (66, 79, 98, 128 .. 130 substreams), of 29 parts in 16 waves (157)
    and of 8 and 4 parts (1025, 2048); at the 2^12 length B of 16, 10, 8 and 2
    parts (512, 769, 1025, 4096 substreams); the runtime direct level of 8 and
    7 parts (1024, 1025); A + C + B at 16384 substreams (slow);
  * test_gpu_spec.py — loops on the direct level (4, 20, 21, 41 substreams), on
    A + B with B of 23, 29, 19, 14 and 16 parts (79 .. 586 substreams) and on
    the runtime level of 8 parts; DN_MT_PARTS_B = 4, 8 on the runtime level;
  * test_gpu_mt_edges.py, test_gpu_list_edges.py — the direct level in groups
    of 2 (2 .. 5 and 17 substreams).

Part counts 5 .. 7, 9, 11 .. 13, 15, 22, 25 and 28, most 16-wave group sizes
below 16, level A in groups of 3 or 4 and the direct level in groups of 6 and
7 ran nowhere, and nothing drew with 2049 or 2050 substreams or without the
runtime rows.  Here every shape below 2^21 coefficients is drawn at its
smallest S (a), some of them in loops, where the levels also run on the
speculation's side stream (b), the shapes that need larger draws (c), the
fallback without runtime rows and the whole B / A tables through DN_MT_BACK=0
(d), and the fused consumers once (e).

The code under test is dn_mt19937_draw_coeffs_device (the levels do not
depend on the consumer); the reference is _native.mt_draw_coeffs, the
sequential host draw that test_host.py and mt_edges pin to CPython.  Every
comparison is byte for byte over the whole block (outputs pre-zeroed: the draw
leaves the tile padding alone) plus getstate() equality; a failure names the
shape."""
import random

import pytest
import torch

import mt_levels as ml
from delta_node.crypto import shamir
from delta_node.crypto.shamir import _native, field
from golden.fixtures import secrets_int64

pytestmark = pytest.mark.gpu

STARTS = (624, 333, 623)  # CPython's index at the call: a fresh seed, mid-array, the last word


def dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _native.lib()


def rng_at(seed, start: int) -> random.Random:
    rng = random.Random(seed)  # (index 624)
    if start != 624:
        rng.getrandbits(32 * start)  # one regeneration, then `start` words taken
    assert rng.getstate()[1][-1] == start
    return rng


def what_of(ncoef: int, tm1: int, start=None, **kw) -> str:
    p = ml.plan(ncoef, **kw)
    return f"{ml.describe(p.ki, p.S, p.kind, p.levels)}; {ncoef} coefficients, t-1={tm1}, index {start}"


def draw_equals_host(a: random.Random, b: random.Random, n: int, tm1: int, what: str):
    """One device draw from `b` against the host draw from `a` (equal states
    before, equal states after)."""
    want = torch.from_numpy(_native.mt_draw_coeffs(a, n, tm1)).to(dev())
    got = torch.zeros((tm1, field.vec_bytes(n)), dtype=torch.uint8, device=dev())
    assert _native.mt_draw_coeffs_device(b, n, tm1, got) is True, f"{what}: the device draw asked for a host redo"
    if not torch.equal(got, want):
        bad = (got != want).any(dim=0).nonzero()
        raise AssertionError(f"{what}: {len(bad)} byte columns differ, first at {int(bad[0])} of {got.shape[1]}")
    assert a.getstate() == b.getstate(), f"{what}: final state"


def one_draw(n: int, tm1: int, start: int, what: str = None):
    a = rng_at(n * 31 + tm1 + start, start)
    b = random.Random()
    b.setstate(a.getstate())
    draw_equals_host(a, b, n, tm1, what or what_of(n * tm1, tm1, start))


# ------------------------------------------------------------------ (a) every shape below 2^21 coefficients
SHAPES = list(ml.shapes(1, (1 << 21) - 1).items())  # [(shape, (ki, smallest S))]


def shape_sizes(i: int):
    """[(n, tm1)] of shape i: the last substream holding one element's draws,
    and full.  t - 1 = 2 for every fourth shape (the element-major order).
    (17 substreams of 2^10 draws: that length begins at 65 * 2^8 + 1
    coefficients, which test_gpu_parity.py draws, as it does the next element
    count at t - 1 = 2; the one after here.)"""
    _, (ki, S) = SHAPES[i]
    tm1 = 2 if i % 4 == 2 else 1
    d = ml.sub_draws(ki)
    few = (S - 1) * d + tm1
    if ml.sub_len(few) != ki:
        few = (ml.DIRECT_ROWS + 1 << 8) + 2 * tm1
    return [(few // tm1, tm1), (S * d // tm1, tm1)]


# (n, t - 1) the product library's coefficient draw already runs at elsewhere
# in the suite (test_gpu_parity.py, test_gpu_spec.py, test_gpu_mt_edges.py)
DRAWN_ELSEWHERE = {(1, 2), (1000, 2), (40000, 2), (40000, 4), (100003, 1), (1 << 20, 2), ((1 << 20) + 77, 3),
                   ((1 << 20) - 3, 2), ((1 << 23) - 5, 2), (1 << 23, 2), (1 << 26, 4), ((1 << 24) + 1, 1),
                   ((1 << 23) + 1, 2), (8320, 2), (8321, 2), (4160, 4), (16640, 1), (16641, 1), (33280, 2), (33281, 2),
                   (1 << 16, 2), (2561, 2), (2048 * 5 + 1, 1), (400, 2), (5 * 1024 + 18, 1), ((1 << 20) + 1, 2),
                   ((1 << 23) + 7, 2), (300, 3), (5548, 3), ((1 << 20) + 5, 2)}


def test_every_shape_has_its_case():
    """60 shapes, each at a size that has it (both fills), none at a size the
    suite already draws at."""
    assert len(SHAPES) == 60
    for i, (shape, (ki, S)) in enumerate(SHAPES):
        for n, tm1 in shape_sizes(i):
            p = ml.plan(n * tm1)
            assert (p.ki, p.S) == (ki, S) and ml.shape_of(p.ki, p.kind, p.levels) == shape, (i, n, tm1)
            assert (n, tm1) not in DRAWN_ELSEWHERE, (i, n, tm1)
    for n, tm1 in LARGER + [(n, tm1) for n, tm1, _ in BOUNDARY]:
        assert (n, tm1) not in DRAWN_ELSEWHERE


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=lambda i: "S%d-of-2^%d" % (SHAPES[i][1][1], ml.LEN_LOG2[SHAPES[i][1][0]]))
def test_draw_at_every_level_shape(i):
    """The shape's smallest S, the last substream with one element's draws and
    full, each from MT index 624, 333 and 623: the host draw's block and state."""
    for n, tm1 in shape_sizes(i):
        for start in STARTS:
            one_draw(n, tm1, start)


# ------------------------------------------------------------------ (b) loops
PRODUCT_SPEC_MIN, PRODUCT_BESIDE_MIN = 1 << 23, 1 << 16


def speculates(ncoef: int, spec_min: int, beside_min: int) -> bool:
    """mt_device_run's decision for a coefficient draw that continues the
    previous one: the next call's levels beside the generation where they fit
    (the runtime level always; else the generation's 8964-byte rings of
    ceil(S / 256) substreams and one 84968-byte jump workgroup within a CU's
    160 KB, for substreams of 2^12 draws or at most 256 substreams), or after
    it from spec_min coefficients."""
    p = ml.plan(ncoef)
    if p.S < 2 or ncoef < min(spec_min, beside_min):
        return False
    fit = (p.S + 255) // 256 * 8964 + 84968 <= 160 * 1024
    beside = ncoef >= beside_min and (p.rt or (fit and (p.draws >= 4096 or p.S <= 256)))
    return beside or ncoef >= spec_min


def loop_of_three(ki: int, S: int, tm1: int, spec_min: int, beside_min: int):
    """Three consecutive draws of S full substreams on one generator against
    three host draws.  The first call finds nothing to continue; the second
    continues it and speculates where mt_device_run's rule says so; the third
    then uses the speculated windows: one hit, two launches — or none at all."""
    n = S * ml.sub_draws(ki) // tm1
    what = what_of(n * tm1, tm1, 333)
    a = rng_at(S * 7 + ki, 333)
    b = random.Random()
    b.setstate(a.getstate())
    s0 = _native.mt_spec_stats()
    for i in range(3):
        draw_equals_host(a, b, n, tm1, f"{what}, call {i}")
    s1 = _native.mt_spec_stats()
    want = (1, 2) if speculates(n * tm1, spec_min, beside_min) else (0, 0)
    assert (s1["hits"] - s0["hits"], s1["launched"] - s0["launched"]) == want, (what, s0, s1)
    assert bool(s1["armed"]) is (want == (1, 2)), what


# (ki, S): one shape per kind and workgroup width, and level B at the part
# counts a request for 32, 16, 8 and 4 parts gives (23 or 29, 16, 8, 4)
LOOP_PRODUCT = [(0, 117), (0, 135), (0, 445), (0, 993), (0, 1983)]  # >= 2^16 coefficients
LOOP_TUNING = [(3, 2), (3, 58), (0, 17)]                            # below: the direct level, 23 parts


@pytest.mark.parametrize("ki,S", LOOP_PRODUCT)
def test_loop_at_a_level_shape(ki, S):
    """The product library: A + B with B in 8-wave and in 16-wave workgroups
    (117, 135 substreams: beside the generation), and B of 16, 8 and 4 parts
    (445, 993, 1983 substreams of 2^10 draws: more than 256, so the product
    does not speculate and every call jumps for itself)."""
    assert ml.coeffs_for(S, ki, True) >= PRODUCT_BESIDE_MIN
    loop_of_three(ki, S, 2 if S == 135 else 1, PRODUCT_SPEC_MIN, PRODUCT_BESIDE_MIN)


@pytest.mark.parametrize("ki,S", LOOP_TUNING)
def test_loop_at_a_direct_level_shape_below_the_thresholds(ki, S, monkeypatch):
    """The tuning library with DN_MT_BESIDE_MIN=0: the direct level of 2, 58
    and 17 substreams beside the generation."""
    assert ml.coeffs_for(S, ki, True) < PRODUCT_BESIDE_MIN
    monkeypatch.setenv("DN_MT_BESIDE_MIN", "0")
    with _native.library(_native.TUNING_LIB):
        loop_of_three(ki, S, 1, PRODUCT_SPEC_MIN, 0)


@pytest.mark.parametrize("ki,S", [(0, 445), (0, 993), (0, 1983)])
def test_loop_speculating_after_the_generation(ki, S, monkeypatch):
    """The tuning library with DN_MT_SPEC_MIN=0: level B of 16, 8 and 4 parts
    on the side stream after the generation, and the third call on its windows."""
    monkeypatch.setenv("DN_MT_SPEC_MIN", "0")
    with _native.library(_native.TUNING_LIB):
        loop_of_three(ki, S, 1, 0, PRODUCT_BESIDE_MIN)


def test_loop_at_the_runtime_level_with_four_parts():
    """1639 substreams of 2^14 draws (26.9 million coefficients): the runtime
    direct level of 4 parts, groups of 13, speculated beside the generation."""
    assert ml.plan(1639 << 14).kind == "rt" and ml.plan(1639 << 14).levels[0].P == 4
    loop_of_three(2, 1639, 2, PRODUCT_SPEC_MIN, PRODUCT_BESIDE_MIN)


# ------------------------------------------------------------------ (c) shapes that need larger draws
def larger(ki: int, S: int, tm1: int):
    return ((S - 1) * ml.sub_draws(ki) + tm1) // tm1, tm1


# 2^12-draw substreams: the smallest S with 3 and with 2 parts in level B, and
# the largest draw of that length (4096 substreams: A_63); the runtime direct
# level at the part counts 6, 5 and 4 (1024 and 1025 substreams, 8 and 7
# parts: test_gpu_parity.py)
LARGER = [larger(1, 2117, 1), larger(1, 2821, 2), (((1 << 24) - 2) // 2, 2), larger(2, 1171, 1), larger(2, 1365, 2),
          larger(2, 1639, 1)]


@pytest.mark.parametrize("n,tm1", LARGER)
def test_draw_at_the_larger_level_shapes(n, tm1):
    p = ml.plan(n * tm1)
    want = {2117: ("radix", 3), 2821: ("radix", 2), 4096: ("radix", 2), 1171: ("rt", 6), 1365: ("rt", 5), 1639: ("rt", 4)}
    assert (p.kind, [l for l in p.levels if l][-1].P) == want[p.S], p
    if p.S == 4096:
        assert p.ki == 1 and ml.JUMP_ROWS + 63 in p.levels[0].polys  # A_63 of the 2^12 table
    one_draw(n, tm1, 333)


# the last runtime row and the first radix-level draw of the 2^14 table
BOUNDARY = [(((2049 - 1) << 13) + 1, 2, "rt"), (((2050 - 1) << 13) + 1, 2, "radix")]


@pytest.mark.slow
@pytest.mark.parametrize("n,tm1,kind", BOUNDARY)
def test_draw_on_either_side_of_the_last_runtime_row(n, tm1, kind):
    """S - 1 <= 2048: 2049 substreams take the runtime direct level (3 parts,
    its last row D_2048), 2050 levels A and B of the 2^14 table (33.6 million
    coefficients, a 2.2 GB block each)."""
    p = ml.plan(n * tm1)
    assert (p.S, p.kind) == (2049 if kind == "rt" else 2050, kind)
    if kind == "rt":
        assert ml.RT_BASE + ml.RT_ROWS - 1 in p.levels[0].polys
    one_draw(n, tm1, 623)


# ------------------------------------------------------------------ (d) the fallback and whole tables
def test_fallback_without_the_runtime_rows(monkeypatch):
    """The tuning library with DN_MT_RT=0, as on a host without carry-less
    multiply or with a damaged embedded table: 2^24 + 1 coefficients (1025
    substreams) through levels A and B of the 2^14 table."""
    n = (1 << 24) + 1
    p = ml.plan(n, rt_rows=False)
    assert (p.S, p.kind, [l.name for l in p.levels if l]) == (1025, "radix", ["A", "B"])
    monkeypatch.setenv("DN_MT_RT", "0")
    with _native.library(_native.TUNING_LIB):
        one_draw(n, 1, 333, what_of(n, 1, 333, rt_rows=False) + ", DN_MT_RT=0")


@pytest.mark.parametrize("n,tm1,log2,a_rows", [((1 << 21) - 3, 1, 10, 32), ((1 << 24) - 5, 1, 12, 64)])
def test_every_window_jumped_to_reads_the_whole_tables(n, tm1, log2, a_rows, monkeypatch):
    """The tuning library with DN_MT_BACK=0 (forward generation only: every
    window is jumped to) at the largest draws of the 2^10 and 2^12 lengths: one
    draw reads B_1 .. B_63, odd rows included, and A_0 .. A_31 / A_63."""
    p = ml.plan(n * tm1, back=0)
    t0 = p.ki * ml.JUMP_ROWS
    assert ml.LEN_LOG2[p.ki] == log2 and p.back == 0 and p.kind == "radix"
    assert p.levels[0].polys == frozenset(range(t0, t0 + a_rows)) and p.levels[1] is None
    assert p.levels[2].polys == frozenset(range(t0 + ml.ROW_B + 1, t0 + ml.ROW_B + 64))
    assert p.levels[2].n == p.S - 1 - a_rows  # every window but the A windows
    monkeypatch.setenv("DN_MT_BACK", "0")
    with _native.library(_native.TUNING_LIB):
        one_draw(n, tm1, 333, what_of(n * tm1, tm1, 333, back=0) + ", DN_MT_BACK=0")


# ------------------------------------------------------------------ (e) the fused consumers
@pytest.mark.parametrize("ki,S", [(3, 18), (0, 69), (0, 135)], ids=["direct", "radix-8-waves", "radix-16-waves"])
@pytest.mark.parametrize("t,n_shares", [(2, 3), (3, 5), (5, 9)])
def test_make_shares_vec_at_three_level_shapes(t, n_shares, ki, S):
    """make_shares_vec (the fused draw + split) at the smallest element count
    whose draw has S substreams, against the host draw + split."""
    N = -(-ml.coeffs_for(S, ki, False) // (t - 1))
    p = ml.plan(N * (t - 1))
    assert (p.ki, p.S) == (ki, S)
    what = what_of(N * (t - 1), t - 1, 333)
    sec = torch.from_numpy(secrets_int64(S + t, N)).to(dev())
    a, b = shamir.SecretShare(t), shamir.SecretShare(t)
    a.random.seed(S * 11 + t)
    a.random.getrandbits(32 * 333)
    b.random.setstate(a.random.getstate())
    got = a.make_shares_vec(sec, n_shares, out=torch.zeros((n_shares, field.vec_bytes(N)), dtype=torch.uint8, device=dev()))
    assert a.last_draw_rejected is False, what
    co = torch.from_numpy(_native.mt_draw_coeffs(b.random, N, t - 1)).to(dev())
    want = torch.zeros_like(got)
    _native.split_u64(sec, co, want, N, t, n_shares)
    assert torch.equal(got, want), what
    assert a.random.getstate() == b.random.getstate(), what
