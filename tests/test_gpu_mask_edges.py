"""The mask PRG, fix / unfix_precision kernels (csrc/mask_pcg64.hip) at their
edges, bit for bit against numpy: Lemire rejections placed by crafted PCG64
states (tests/mask_edges.py), sparse rejections and the exact replay, both ends
of the 64-bit Lemire range, the segment API, the default kernel's tile loop,
and the float64 <-> int64 conversions at every precision.

`build` selects the kernel under test: the product library, or the tuning
build with DN_MASK_SMALL=1 (512-element tiles) or DN_MASK_BLOCKS=1 / 3 (the
default kernel on 1 or 3 workgroups, so that its 4 or 12 waves step through
many tiles at small n).
"""
import collections
import functools
import random

import numpy as np
import pytest
import torch

import mask_edges as me
from delta_node import utils
from delta_node.crypto.shamir import _native
from delta_node.utils import _mask_native as mn
from delta_node.utils.mask import bounded_sum
from oracle import py_mask as pm

pytestmark = pytest.mark.gpu
SENT = 0x5A5A5A5A5A5A5A5A
MERS = (0, 2**47 - 1)
BUILDS = {"product": {}, "small": {"DN_MASK_SMALL": "1"}, "blocks1": {"DN_MASK_BLOCKS": "1"},
          "blocks3": {"DN_MASK_BLOCKS": "3"}}
LOOPED = ["product", "blocks1", "blocks3"]
ALL_BUILDS = ["product", "small", "blocks1", "blocks3"]


Build = collections.namedtuple("Build", "name tile")


class Crafted:
    """A sentinel seed: bounded_sum's mn.pcg64 returns this state as it is."""

    def __init__(self, state_inc):
        self.state, self.inc = state_inc


@pytest.fixture
def build(request, monkeypatch):
    """Bind the kernel variant; the value names it and gives the number of
    elements a wave draws (and tests) per tile."""
    name = getattr(request, "param", "product")
    real = mn.pcg64

    def pcg64(seed):
        if isinstance(seed, Crafted):
            return mn.PCG64(seed.state >> 64, seed.state & me.M64, seed.inc >> 64, seed.inc & me.M64)
        return real(seed)

    monkeypatch.setattr(mn, "pcg64", pcg64)
    b = Build(name, me.SMALL_TILE if name == "small" else me.TILE)
    if name == "product":
        yield b
        return
    for k, v in BUILDS[name].items():
        monkeypatch.setenv(k, v)
    with _native.library(_native.TUNING_LIB):
        yield b


def seed_bytes(i: int) -> bytes:
    r = random.Random(7000 + i)
    return bytes(r.getrandbits(8) for _ in range(32))


@functools.lru_cache(maxsize=None)
def _ref_cached(seed: bytes, low: int, high: int, n: int) -> np.ndarray:
    a = np.random.default_rng(list(seed)).integers(low, high, size=n, dtype=np.int64)
    a.setflags(write=False)
    return a


def ref_draw(seed, low: int, high: int, n: int) -> np.ndarray:
    """numpy's draw for a seed or a crafted state (a prefix of a longer draw is the shorter draw)."""
    if isinstance(seed, Crafted):
        return me.numpy_integers(seed.state, seed.inc, low, high, n)
    return _ref_cached(seed, low, high, n)


def ref_sum(terms, low, high, n, base=None) -> np.ndarray:
    return me.wrapping_sum(base, [(ref_draw(s, low, high, n), sg) for s, sg in terms])


def dev_i64(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


def flags_of(terms, n, low, high) -> list:
    """The reject flags of one direct accumulate launch, in the caller's order."""
    gens = [mn.pcg64(s) for s, _ in terms]
    flags = torch.zeros(len(gens), dtype=torch.int32, device="cuda")
    out = torch.empty(n, dtype=torch.int64, device="cuda")
    mn.accumulate(gens, [sg for _, sg in terms], out, n, low, high - 1 - low, rejects=flags)
    return flags.cpu().tolist()


# ------------------------------------------------------------------ B1: Mersenne path
@pytest.mark.parametrize("build", ["product", "small"], indirect=True)
@pytest.mark.parametrize("m", me.CRAFT_MS)
def test_mersenne_rejection_at_crafted_raw(m, build):
    """make_mask's range with a raw draw whose Lemire low word is m: rejected
    for m < 2^17, accepted at 2^17.  The sum equals numpy's from the same state
    wherever the generator sits in the launch, and the reject flag is set at the
    caller's index of that generator."""
    n = me.CRAFT_N
    a, b = seed_bytes(1), seed_bytes(2)
    seen = build.tile * ((n + build.tile - 1) // build.tile)  # the raw draws the kernel tests
    for i, k in enumerate(me.CRAFT_KS + [me.CRAFT_K_PAST]):
        c = Crafted(me.crafted_state(m, k, me.some_inc(i)))
        rej = me.raw_rejects(c.state, c.inc, me.MERS_EXCL, seen)
        assert rej == ([k] if m < me.MERS_THRESHOLD else []), "the case is what it claims"
        placements = [([(c, 1)], 0), ([(a, 1), (c, 1)], 1), ([(a, 1), (b, 1), (c, 1)], 2),
                      ([(c, -1), (a, 1), (b, 1)], 0)]
        for terms, at in placements:
            got = bounded_sum(terms, n, *MERS).cpu().numpy()
            assert np.array_equal(got, ref_sum(terms, *MERS, n)), (m, k, len(terms), at)
            flags = flags_of(terms, n, *MERS)
            if any(r < n for r in rej):
                assert flags[at] != 0, (m, k, len(terms))
            elif not rej:
                assert flags[at] == 0, (m, k, len(terms))
            # else: a rejected raw past the array but inside its last tile; the
            # kernel may or may not flag it (it does test those draws), and the
            # replay it then takes must leave numpy's values, checked above
            assert not any(f for j, f in enumerate(flags) if j != at), (m, k, len(terms))


# ------------------------------------------------------------------ B2: sparse rejections
@pytest.mark.parametrize("build", ALL_BUILDS, indirect=True)
@pytest.mark.parametrize("excl", me.SPARSE_EXCLS)
def test_sparse_rejections_replay(excl, build):
    """A few scattered rejections (the realistic regime of _replay_exact), with
    array ends placed on them, a rejection at raw 0 and two adjacent ones."""
    low, high = me.SPARSE_LOW, me.SPARSE_LOW + excl
    seed, s2 = me.SPARSE_SEED, seed_bytes(3)
    ns = []
    for n in (20000, 100003):
        rej = me.sparse_rejects(excl, n)
        assert 3 <= len(rej) <= 64, "sparse, and the replay stays a handful of launches"
        ns.append(n)
    rej = me.sparse_rejects(excl, 100003)
    for j in (0, 1, len(rej) - 1):
        ns += [rej[j] - j, rej[j] - j + 1]  # ends just before rejected raw r_j / first element after it
    for n in ns:
        got = bounded_sum([(seed, 1)], n, low, high).cpu().numpy()
        assert np.array_equal(got, ref_draw(seed, low, high, 100003)[:n]), n
    for n in (ns[0], ns[2], ns[3]):
        base = me.extremes_base(n)
        for terms in ([(seed, 1), (s2, -1)], [(s2, -1), (seed, 1)], [(seed, -1), (s2, 1)]):
            got = bounded_sum(terms, n, low, high, base_i64=dev_i64(base)).cpu().numpy()
            want = me.wrapping_sum(base, [(ref_draw(s, low, high, 100003)[:n], sg) for s, sg in terms])
            assert np.array_equal(got, want), (n, terms[0][1])
    step = excl & -excl  # the low words x excl can take are its multiples; 0 and step are below the threshold
    c0 = Crafted(me.crafted_state(step, 0, me.some_inc(20), excl))
    assert np.array_equal(bounded_sum([(c0, 1)], 1, low, high).cpu().numpy(), ref_draw(c0, low, high, 1))
    assert flags_of([(c0, 1)], 1, low, high)[0] != 0
    cp = Crafted(me.crafted_pair_state(0, step, 4095, excl))
    for n in (4095, 4096, 4097, 5000):
        terms = [(s2, 1), (cp, -1)]
        got = bounded_sum(terms, n, low, high).cpu().numpy()
        assert np.array_equal(got, ref_sum(terms, low, high, n)), n


# ------------------------------------------------------------------ B3: the reject list
def test_list_rejects_direct():
    dev = torch.device("cuda")
    g = mn.pcg64(me.SPARSE_SEED)
    st, inc = pm.pcg64_init(me.SPARSE_SEED)
    excl = me.SPARSE_EXCLS[0]
    for b, e in [(37, 100040), (513, 4096), (4095, 4097), (0, 45), (44, 45), (45, 46)]:
        want = me.raw_rejects(st, inc, excl, e, b)
        cnt, got = mn.list_rejects(g, excl - 1, b, e, 256, dev)
        assert (cnt, got) == (len(want), want), (b, e)
    want = me.raw_rejects(st, inc, excl, 100040, 37)
    cnt, got = mn.list_rejects(g, excl - 1, 37, 100040, 8, dev)
    assert cnt == len(want) > 8, "the count is complete past the capacity"
    assert len(got) == len(set(got)) == 8 and set(got) <= set(want)
    # a quarter of the draws rejected
    low, high = -3 * 2**61, 3 * 2**61
    want = me.raw_rejects(st, inc, high - low, 513 + 3001, 513)
    cnt, got = mn.list_rejects(g, high - low - 1, 513, 513 + 3001, 4096, dev)
    assert len(want) > 500 and (cnt, got) == (len(want), want)
    assert mn.list_rejects(g, excl - 1, 100, 100, 8, dev) == (0, [])


# ------------------------------------------------------------------ B4: ranges
RANGES = {"rng=2^32,low=0": (0, 2**32 + 1), "rng=2^32,low=min": (-2**63, -2**63 + 2**32 + 1),
          "rng=2^64-2": (-2**63, 2**63 - 1), "excl=2^40": (-5, 2**40 - 5), "excl=2^63": (-2**62, 2**62)}
SIGNS = [1, -1, 1, -1, -1, 1, -1, 1, -1, -1, 1, -1, 1, -1, -1, 1, -1]  # 7 of the first 16 add: odd on both sides


@pytest.mark.parametrize("build", LOOPED, indirect=True)
@pytest.mark.parametrize("name", list(RANGES))
def test_ranges_general_path(name, build):
    low, high = RANGES[name]
    sizes = me.TILE_NS + ([me.LOOP_N] if build.name.startswith("blocks") else [])
    nmax = max(sizes)
    seeds = [seed_bytes(100 + i) for i in range(17)]
    base = me.extremes_base(nmax)
    dbase = dev_i64(base)
    for gcount in me.GEN_COUNTS:
        terms = list(zip(seeds[:gcount], SIGNS[:gcount]))
        for n in sizes:
            got = bounded_sum(terms, n, low, high, base_i64=dbase[:n]).cpu().numpy()
            want = me.wrapping_sum(base[:n], [(ref_draw(s, low, high, nmax)[:n], sg) for s, sg in terms])
            assert np.array_equal(got, want), (name, gcount, n)
    if me.threshold(high - low) == 0:  # a power-of-two range rejects nothing
        assert not any(flags_of(list(zip(seeds[:16], SIGNS[:16])), nmax, low, high))


@pytest.mark.parametrize("build", LOOPED, indirect=True)
def test_block_cap_sets_the_waves_that_draw(build):
    """The looped builds do loop: every wave that saw a rejected draw adds one to
    its generator's flag, so where a quarter of the draws are rejected the flag
    counts the waves that drew — one per tile in the product build, 4 per
    workgroup under DN_MASK_BLOCKS."""
    n = me.LOOP_N
    tiles = (n + me.TILE - 1) // me.TILE
    waves = {"product": tiles, "blocks1": 4, "blocks3": 12}[build.name]
    assert flags_of([(me.SPARSE_SEED, 1), (seed_bytes(3), -1)], n, -3 * 2**61, 3 * 2**61) == [waves, waves]


def test_refusals_leave_out_untouched():
    out = torch.full((64,), SENT, dtype=torch.int64, device="cuda")
    g = mn.pcg64(1)
    zeros = torch.zeros(64, dtype=torch.float64, device="cuda")
    with pytest.raises(NotImplementedError):
        bounded_sum([(1, 1)], 64, 0, 2**32, out=out)  # rng = 2^32 - 1: numpy's 32-bit path
    with pytest.raises(NotImplementedError):
        bounded_sum([(1, 1)], 64, -2**63, 2**63, out=out)  # rng = 2^64 - 1: numpy draws raw words
    with pytest.raises(NotImplementedError):
        mn.list_rejects(g, 2**32 - 1, 0, 64, 8, torch.device("cuda"))
    for p in (23, -1):
        with pytest.raises(ValueError):
            bounded_sum([], 64, *MERS, base_f64=zeros, precision=p, out=out)
        with pytest.raises(ValueError):
            utils.fix_precision(np.zeros(4), p)
        with pytest.raises(ValueError):
            utils.unfix_precision(np.zeros(4, dtype=np.int64), p)
    with pytest.raises(ValueError):
        bounded_sum([(1, 0)], 64, *MERS, out=out)
    with pytest.raises(ValueError):
        mn.accumulate([g], [0], out, 64, 0, 2**47 - 2)
    with pytest.raises(NotImplementedError):
        mn.accumulate([g] * 17, [1] * 17, out, 64, 0, 2**47 - 2)
    # nothing to do: n = 0, an empty segment
    assert bounded_sum([(1, 1)], 0, *MERS).shape == (0,)
    mn.accumulate([g], [1], out, 0, 0, 2**47 - 2)
    mn.accumulate([g], [1], out, 64, 0, 2**47 - 2, elem_begin=10, elem_end=10)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
    e = utils.fix_precision(np.zeros((0, 3)), 8)
    assert e.shape == (0, 3) and e.dtype == np.int64
    e = utils.unfix_precision(np.zeros((0, 3), dtype=np.int64), 8)
    assert e.shape == (0, 3) and e.dtype == np.float64


# ------------------------------------------------------------------ B5: segment API
@pytest.mark.parametrize("build", ALL_BUILDS, indirect=True)
def test_segment_api_edges(build):
    """Elements [b, e) of generator g draw raw e + off_g; the base is indexed by
    the absolute element; nothing outside [b, e) is written."""
    n, pad = 9000, 64
    seeds, signs, offs = [seed_bytes(200 + i) for i in range(3)], [1, -1, 1], [0, 5, 37]
    gens = [mn.pcg64(s) for s in seeds]
    base = me.extremes_base(n)
    x = np.random.default_rng(5).standard_normal(n) * 1e6
    x[[0, 1234, 4096, 8000, 8999]] = [np.nan, 0.29, -0.29, 9.3e15, -np.inf]
    fixed = me.fix_expect(x, 3)
    dbase, dx = dev_i64(base), torch.from_numpy(x).cuda()
    # make_mask's range (a crafted-free stream rejects nothing: shifting by a raw
    # offset is numpy's stream shifted) and a power-of-two range on the general path
    for low, high in (MERS, RANGES["excl=2^63"]):
        refs = [ref_draw(s, low, high, n + pad) for s in seeds]
        for b, e in [(1234, 8001), (4096, 8192), (511, 513), (0, 1), (8999, 9000), (4095, 4097), (1, 9000)]:
            for kind in ("i64", "f64", None):
                out = torch.full((n,), SENT, dtype=torch.int64, device="cuda")
                kw = {"i64": dict(base_i64=dbase), "f64": dict(base_f64=dx, precision=3), None: {}}[kind]
                mn.accumulate(gens, signs, out, n, low, high - 1 - low, raw_offsets=offs, elem_begin=b, elem_end=e,
                              **kw)
                o = out.cpu().numpy()
                bb = {"i64": base, "f64": fixed, None: np.zeros(n, dtype=np.int64)}[kind][b:e]
                want = me.wrapping_sum(bb, [(r[b + off:e + off], sg) for r, sg, off in zip(refs, signs, offs)])
                assert np.array_equal(o[b:e], want), (low, b, e, kind)
                assert (o[:b] == SENT).all() and (o[e:] == SENT).all(), (low, b, e, kind)


# ------------------------------------------------------------------ B6: the default kernel's tile loop
def test_default_kernel_tile_loop_product_build():
    """n > 8192 * 4 * 4096: the product kernel's waves take a second tile (a new
    jump, the per-lane LDS states overwritten).  Checked against the same sum
    from segments of at most 2^27 elements (one tile per wave, the path the 2^24
    digests pin), and windows of it against numpy after PCG64.advance."""
    n = me.BIG_MASK_N
    seeds, signs = [seed_bytes(300), seed_bytes(301)], [1, -1]
    gens = [mn.pcg64(s) for s in seeds]
    flags = torch.zeros(2, dtype=torch.int32, device="cuda")
    out = torch.empty(n, dtype=torch.int64, device="cuda")
    mn.accumulate(gens, signs, out, n, 0, 2**47 - 2, rejects=flags)
    assert flags.cpu().tolist() == [0, 0]  # no rejection: element e is raw e, so advance() finds a window
    seg = torch.empty(n, dtype=torch.int64, device="cuda")
    for b in range(0, n, 1 << 27):
        mn.accumulate(gens, signs, seg, n, 0, 2**47 - 2, elem_begin=b, elem_end=min(n, b + (1 << 27)))
    assert torch.equal(out, seg)
    del seg
    second = me.DEFAULT_GRID_WAVES * me.TILE
    assert second + me.TILE < n
    for start, cnt in [(0, 4096), (second, 4096), (second - 100, 200), (n - 4096, 4096)]:
        terms = []
        for s in seeds:
            st, inc = me.numpy_advanced(*me.numpy_seeded(s), start)
            terms.append(me.numpy_integers(st, inc, *MERS, cnt))
        want = me.wrapping_sum(None, list(zip(terms, signs)))
        assert np.array_equal(out[start:start + cnt].cpu().numpy(), want), start
    del out
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ B7: fix_precision
@pytest.mark.parametrize("p", range(23))
def test_fix_precision_edges(p):
    x, want = me.fix_cases(p)
    got = utils.fix_precision(x.copy(), p)  # (the shared inputs are read-only)
    assert got.dtype == np.int64
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(float(x[i]).hex(), int(got[i]), int(want[i])) for i in bad[:5]]


@pytest.mark.parametrize("p", [0, 3, 8])
def test_fix_precision_input_types(p):
    """Every input type widens to float64 first, as the reference's astype does."""
    fl = [0.0, -0.0, 0.29, -0.29, 1.15, 2.675, 0.1, 1 / 3, 65504.0, -65504.0, 6e-8, 1e-40, 3.3895314e38, 1e30, -1e30,
          9.2233e10, 9.2233e15, 9.3e18, float("inf"), float("-inf"), float("nan"), 123456.789, -0.999999]
    ints = [0, 1, -1, 2**31 - 1, -2**31, 2**53 + 1, -(2**53) - 1, 2**53 + 3, me.INT64_MAX, me.INT64_MIN, 2**63 - 513,
            2**63 - 512, 922337203685, 9223372036854775, -9223372036854775, 92233720368547758]
    with np.errstate(all="ignore"):
        cases = [torch.tensor(fl, dtype=torch.float64).to(dt) for dt in (torch.float16, torch.bfloat16, torch.float32,
                                                                         torch.float64)]
    cases.append(torch.tensor([v for v in ints if -2**31 <= v < 2**31], dtype=torch.int32))
    cases.append(torch.tensor(ints, dtype=torch.int64))
    for t in cases:
        if t.dtype == torch.bfloat16:
            wide = t.to(torch.float64).numpy()  # bfloat16 -> float64 is exact
        else:
            wide = t.numpy().astype(np.float64)
        want = me.fix_expect(wide, p)
        got = utils.fix_precision(t, p)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.int64
        assert np.array_equal(got.cpu().numpy(), want), (t.dtype, p)
        if t.dtype != torch.bfloat16:
            got = utils.fix_precision(t.numpy().reshape(-1, 1), p)
            assert isinstance(got, np.ndarray) and np.array_equal(got, want.reshape(-1, 1)), (t.dtype, p)


def test_masked_sum_base_at_fix_edges():
    x, fixed = me.fix_cases(8)
    terms = [(seed_bytes(400), 1), (seed_bytes(401), -1)]
    got = utils.masked_sum(torch.from_numpy(x.copy()), terms, precision=8).cpu().numpy()
    want = me.wrapping_sum(fixed, [(pm.make_mask_numpy(s, x.shape), sg) for s, sg in terms])
    assert np.array_equal(got, want)


# ------------------------------------------------------------------ B8: unfix_precision
@pytest.mark.parametrize("p", range(23))
def test_unfix_precision_edges(p):
    v = me.unfix_cases()
    got = utils.unfix_precision(v.copy(), p)  # (the shared inputs are read-only)
    want = me.unfix_expect(v, p)
    assert got.dtype == np.float64
    bad = np.nonzero(me.bits(got) != me.bits(want))[0]
    assert bad.size == 0, [(int(v[i]), float(got[i]).hex(), float(want[i]).hex()) for i in bad[:5]]


@pytest.mark.parametrize("p", [0, 1, 3, 8, 22])
def test_unfix_precision_float_inputs(p):
    """Float inputs take the torch branch: the same correctly rounded float64
    division, not a multiplication by the reciprocal."""
    rng = np.random.default_rng(p)
    x = np.concatenate([rng.standard_normal(4000) * 1e9, np.arange(1.0, 200.0), [0.0, -0.0, 5e-324, 1e308, np.inf]])
    want = x / np.float64(10**p)
    if p:
        with np.errstate(all="ignore"):
            recip = x * (np.float64(1.0) / np.float64(10**p))
        assert (me.bits(recip) != me.bits(want)).any(), "the inputs tell a reciprocal multiply from a division"
    got = utils.unfix_precision(x, p)
    assert np.array_equal(me.bits(got), me.bits(want))
    x32 = x[:4000].astype(np.float32)
    got = utils.unfix_precision(torch.from_numpy(x32), p)
    assert isinstance(got, torch.Tensor)
    assert np.array_equal(me.bits(got.cpu().numpy()), me.bits(x32.astype(np.float64) / np.float64(10**p)))


def test_unmasked_values_ragged_tail():
    shape = (37, 129)  # 4773 elements: one full tile and a ragged one
    masked = np.random.default_rng(8).integers(me.INT64_MIN, me.INT64_MAX, size=shape, dtype=np.int64, endpoint=True)
    terms = [(seed_bytes(500), -1), (seed_bytes(501), 1), (seed_bytes(502), -1)]
    for p in (0, 8, 22):
        got = utils.unmasked_values(torch.from_numpy(masked), terms, p).cpu().numpy()
        ints = me.wrapping_sum(masked.reshape(-1), [(pm.make_mask_numpy(s, masked.size), sg) for s, sg in terms])
        want = me.unfix_expect(ints, p).reshape(shape)
        assert got.shape == shape and np.array_equal(me.bits(got), me.bits(want)), p
