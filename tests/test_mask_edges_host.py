"""Pin the builders of tests/mask_edges.py to numpy, and the host half of the
mask C-ABI (dn_pcg64_seed, dn_pcg64_advance) to numpy's SeedSequence and
PCG64.advance.  CPU only; bit-exact."""
import os

import numpy as np
import pytest

import mask_edges as me
from delta_node.utils import _mask_native as mn
from golden.fixtures import HERE
from oracle import py_mask as pm

Z = np.load(os.path.join(HERE, "mask.npz"), allow_pickle=False)
SEEDS = [b"", b"\x00", b"\x00\x00", 0, 2**32, 2**128 + 1, bytes(range(7, 47))]


# ------------------------------------------------------------------ builders
@pytest.mark.parametrize("m", me.CRAFT_MS)
def test_crafted_state_rejects_exactly_raw_k(m):
    """numpy rejects exactly raw draw k of a crafted state for low words below
    2^17 and nothing at 2^17, the threshold of make_mask's range."""
    n = me.CRAFT_N
    for i, k in enumerate(me.CRAFT_KS + [me.CRAFT_K_PAST]):
        st, inc = me.crafted_state(m, k, me.some_inc(i))
        raw = me.numpy_generator(st, inc).bit_generator.random_raw(k + 1)
        assert (int(raw[k]) * me.MERS_EXCL) & me.M64 == m
        vals, rej = me.bounded_from_state(st, inc, n, 0, me.MERS_EXCL)
        assert rej == ([k] if m < me.MERS_THRESHOLD and k < n else []), (m, k)
        ref = me.numpy_integers(st, inc, 0, me.MERS_EXCL, n)
        assert np.array_equal(np.array(vals, dtype=np.int64), ref), (m, k)
        # the rejection shifts numpy's stream by one raw from element k on
        plain = (raw.astype(object) * me.MERS_EXCL) >> 64
        if rej:
            assert [int(v) for v in ref[:k]] == list(plain[:k])
        assert me.raw_rejects(st, inc, me.MERS_EXCL, 8192) == ([k] if m < me.MERS_THRESHOLD else []), (m, k)


def test_threshold_values():
    assert me.threshold(me.MERS_EXCL) == me.MERS_THRESHOLD
    assert me.threshold(2**32 + 1) == 1 and me.threshold(2**64 - 1) == 1
    assert me.threshold(2**40) == 0 and me.threshold(2**63) == 0
    assert [me.threshold(e) for e in me.SPARSE_EXCLS] == [2**53, 2**50]


@pytest.mark.parametrize("excl", me.SPARSE_EXCLS)
def test_crafted_general_and_adjacent_pair(excl):
    """The general recipe (even excl) and two adjacent rejected raws at a tile edge."""
    thr = me.threshold(excl)
    step = excl & -excl
    low = me.SPARSE_LOW
    st, inc = me.crafted_state(step, 0, me.some_inc(1), excl)
    vals, rej = me.bounded_from_state(st, inc, 1, low, low + excl)
    assert rej[0] == 0 and step < thr
    assert np.array_equal(np.array(vals, dtype=np.int64), me.numpy_integers(st, inc, low, low + excl, 1))
    st, inc = me.crafted_pair_state(0, step, 4095, excl)
    vals, rej = me.bounded_from_state(st, inc, 5000, low, low + excl)
    assert 4095 in rej and 4096 in rej
    assert np.array_equal(np.array(vals, dtype=np.int64), me.numpy_integers(st, inc, low, low + excl, 5000))


def test_sparse_rejection_cases_are_sparse():
    """The recorded counts of the sparse-rejection cases (seed bytes(range(32)), low = -2^62)."""
    r = me.sparse_rejects(me.SPARSE_EXCLS[0], 20000)
    assert len(r) == 15 and r[:3] == (44, 3888, 4244)
    assert len(me.sparse_rejects(me.SPARSE_EXCLS[0], 100003)) == 58
    assert len(me.sparse_rejects(me.SPARSE_EXCLS[1], 20000)) == 3
    assert len(me.sparse_rejects(me.SPARSE_EXCLS[1], 100003)) == 5
    st, inc = pm.pcg64_init(me.SPARSE_SEED)
    for excl in me.SPARSE_EXCLS:
        vals, _ = me.bounded_from_state(st, inc, 20000, me.SPARSE_LOW, me.SPARSE_LOW + excl)
        ref = np.random.default_rng(list(me.SPARSE_SEED)).integers(me.SPARSE_LOW, me.SPARSE_LOW + excl, size=20000,
                                                                   dtype=np.int64)
        assert np.array_equal(np.array(vals, dtype=np.int64), ref)
        assert np.array_equal(ref, me.numpy_integers(st, inc, me.SPARSE_LOW, me.SPARSE_LOW + excl, 20000))


def test_fix_unfix_expectations_match_reference_fixture():
    assert np.array_equal(me.fix_expect(Z["fix_in"], 8), Z["fix8"])
    assert np.array_equal(me.bits(me.unfix_expect(Z["unfix_in"], 8)), me.bits(Z["unfix8"]))
    for p in (0, 8, 22):
        x, want = me.fix_cases(p)
        assert len(x) == len(want) == 12 + 600 + 10 + 5
        assert (want == me.INT64_MIN).sum() >= 5  # NaN, the infinities, +-DBL_MAX at least
        x0 = float(np.float64(2.0**63) / np.float64(10**p))
        assert me.fix_expect(np.array([-x0]), p)[0] == me.INT64_MIN  # -2^63 is in range: its own value
    v = me.unfix_cases()
    assert v.dtype == np.int64 and len(v) == 3 + 6 + 6 + 10000
    # the tie rounds to even (2^63), the value under it rounds down
    assert float(np.int64(2**63 - 512)) == 2.0**63 and float(np.int64(2**63 - 513)) == 2.0**63 - 1024


def test_wrapping_sum_is_integer_arithmetic():
    a = np.array([me.INT64_MAX, me.INT64_MIN, 5], dtype=np.int64)
    b = np.array([1, -1, 7], dtype=np.int64)
    got = me.wrapping_sum(a, [(b, 1), (a, -1), (b, 1)])
    assert got.tolist() == [me.wrap_i64(int(x) + 2 * int(y) - int(x)) for x, y in zip(a, b)]


# ------------------------------------------------------------------ host C-ABI
@pytest.mark.parametrize("seed", SEEDS, ids=[repr(s)[:24] for s in SEEDS])
def test_native_seeding_matches_numpy(seed):
    g = mn.pcg64(seed)
    assert (g.state, g.inc) == me.numpy_seeded(seed)
    assert (g.state, g.inc) == pm.pcg64_init(seed)


@pytest.mark.parametrize("seed", [b"", 2**128 + 1, bytes(range(7, 47))], ids=["empty", "int", "40B"])
def test_native_advance_matches_numpy(seed):
    g = mn.pcg64(seed)
    for delta in (0, 1, 63, 64, 4096, 2**32, 2**63, 2**64 - 1):
        h = mn.advance(g, delta)
        assert (h.state, h.inc) == me.numpy_advanced(g.state, g.inc, delta), delta
        assert (g.state, g.inc) == me.numpy_seeded(seed)  # the argument is left alone
    # a few steps are the LCG itself
    st = g.state
    for _ in range(5):
        st, _x = pm.pcg64_next(st, g.inc)
    assert mn.advance(g, 5).state == st


def test_native_advance_composes():
    g = mn.pcg64(12345)
    for a, b in [(0, 0), (1, 63), (4095, 1), (2**32, 2**32), (2**63, 2**63 - 1), (2**64 - 1, 0), (12345, 2**40 + 7)]:
        assert a + b < 2**64
        two = mn.advance(mn.advance(g, a), b)
        one = mn.advance(g, a + b)
        assert (two.state, two.inc) == (one.state, one.inc), (a, b)
