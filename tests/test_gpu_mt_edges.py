"""The device MT19937 draw at real rejected draws and crafted coefficient words.

The draw's claim is bit-exactness with N sequential reference calls on one
random.Random, redraws (raw value >= p - 1, odds ~2^-520 each) included.  The
device flags such a draw (csrc/mt19937_device.hip: the predicate in emit_group
and emit_prepare, mt_flag) and the caller redoes the call on the host; on
seeded generators neither the predicate, nor the flag's way back and its reset,
nor the + 1 carry chain at its edges is ever exercised.  tests/mt_edges.py
builds generator states whose chosen draws carry chosen words, places them
where the kernels change path (mt_edges.positions), and CPython's own randint
gives every expected value (mt_edges.reference), never the host C draw.

Every comparison is byte for byte over the whole block (outputs are zeroed:
the kernels leave the last tile's padding alone) plus getstate() equality.
A case with a rejected value must come back False from the primitive with the
generator untouched; a case with only accepted edge values (or a rejected
value behind the call) must come back True — a predicate that fires too often
gives exact results through the host fallback and shows only there.
test_mt_edges_host.py checks the helper and the host side without a device."""
import functools
import random

import numpy as np
import pytest
import torch

import mt_edges as me
from delta_node.crypto import shamir
from delta_node.crypto.shamir import _native, field

pytestmark = pytest.mark.gpu

# (t, n, N): the smallest shapes of each regime (test_mt_edges_host.py:
# test_positions_follow_the_substream_geometry) — 2^8-draw substreams, forward
# only, and 2^10-draw substreams with the even ones backward
FUSED_SHAPES = [(3, 5, 300), (2, 3, 300), (5, 9, 200), (3, 5, 8321), (5, 9, 4161), (2, 3, 16641)]
# the coefficient draw (T = 0), t - 1 = 3: (tm1, N)
COEF_SHAPES = [(3, 300), (3, 5548)]

FUSED_CASES = [(t, n, N, fam) for t, n, N in FUSED_SHAPES for fam in me.positions(N, t - 1, True)]
COEF_CASES = [(tm1, N, fam) for tm1, N in COEF_SHAPES for fam in me.positions(N, tm1, False)]


def dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _native.lib()


@functools.lru_cache(maxsize=None)
def secrets(N: int):
    host = me.secrets_for(N, N)
    return host, torch.tensor(host, dtype=torch.int64).to(dev())


def block_of(rows) -> np.ndarray:
    return np.stack([field.ints_to_vec(r) for r in rows])


def assert_block(got: torch.Tensor, rows, what):
    g, w = got.cpu().numpy(), block_of(rows)
    if not np.array_equal(g, w):
        n = len(rows[0])
        gl = np.stack([field.vec_to_limbs(r, n) for r in g])
        wl = np.stack([field.vec_to_limbs(r, n) for r in w])
        bad = np.argwhere((gl != wl).any(axis=2))
        where = f"{len(bad)} elements differ, first (row, element) {tuple(bad[0])}" if len(bad) else "tile padding differs"
        raise AssertionError(f"{what}: {where}")


def rng_at(state) -> random.Random:
    rng = random.Random()
    rng.setstate(state)
    return rng


def zeros(rows: int, N: int) -> torch.Tensor:
    return torch.zeros((rows, field.vec_bytes(N)), dtype=torch.uint8, device=dev())


def accepted_state(fam: str, N: int, tm1: int, fused: bool):
    spots = me.positions(N, tm1, fused)[fam]
    first, values = me.accepted_cluster(fam, spots, N * tm1)
    return me.craft_state(values, first, me.FAMILY_INDEX[fam], seed=f"acc-{fam}-{N}-{tm1}")


def rejected_states(fam: str, N: int, tm1: int, fused: bool):
    """One state per spot of the family, each with ONE rejected value (p - 1,
    the smallest, at the last spot; p at the one before): a call with both
    would still be flagged by a predicate that knows only one of them."""
    spots = me.positions(N, tm1, fused)[fam]
    out = []
    for i, d in enumerate(spots):
        v = me.REJECTED[1] if i == len(spots) - 1 else me.REJECTED[0]
        low = 0 if i % 2 else 0x7FFFFF
        out.append(me.craft_state({d: (v, low)}, d, me.FAMILY_INDEX[fam], seed=f"rej-{fam}-{N}-{tm1}-{i}"))
    return out


# ------------------------------------------------------------------ the fused draw + split
def fused_exact(rng, state, t, n, N, what):
    """mt_split_device from `state`: True, the reference's shares and final state."""
    host, sec = secrets(N)
    want, final = me.reference(state, N, t, n, host)
    out = zeros(n, N)
    assert _native.mt_split_device(rng, sec, out, N, t, n) is True, f"{what}: the device draw asked for a host redo"
    assert_block(out, want, what)
    assert rng.getstate() == final, what
    return final


@pytest.mark.parametrize("t,n,N,fam", FUSED_CASES)
def test_fused_split_accepts_the_edges(t, n, N, fam):
    """The ACCEPTED_EDGES cluster over the family's spots (for `after`: up to
    the last draw, a rejected value behind it): the call stays on the device
    and equals the reference."""
    state = accepted_state(fam, N, t - 1, True)
    fused_exact(rng_at(state), state, t, n, N, (t, n, N, fam))


@pytest.mark.parametrize("t,n,N,fam", [c for c in FUSED_CASES if c[3] != "after"])
def test_fused_split_flags_a_rejected_draw(t, n, N, fam):
    """A rejected value at each spot of the family: the primitive returns
    False through the kernel's own flag and leaves the generator alone;
    make_shares_vec returns the reference's shares and state and reports the
    redraw; a following clean call of the same size on the same object stays
    on the device and is exact (the flag does not stick)."""
    host, sec = secrets(N)
    for i, state in enumerate(rejected_states(fam, N, t - 1, True)):
        want, final = me.reference(state, N, t, n, host)
        assert final != me.skip_state(state, 17 * (t - 1) * N)
        ss = shamir.SecretShare(t)
        ss.random.setstate(state)
        assert _native.mt_split_device(ss.random, sec, zeros(n, N), N, t, n) is False, (fam, i)
        assert ss.random.getstate() == state, (fam, i)
        got = ss.make_shares_vec(sec, n, out=zeros(n, N))
        assert ss.last_draw_rejected is True, (fam, i)
        assert_block(got, want, (t, n, N, fam, i))
        assert ss.random.getstate() == final, (fam, i)
    fused_exact(ss.random, final, t, n, N, (t, n, N, fam, "the next call"))
    assert ss.make_shares_vec(sec, n) is not None and ss.last_draw_rejected is False


# ------------------------------------------------------------------ the coefficient draw (T = 0)
def coeffs_exact(rng, state, tm1, N, what):
    cols, final, redrawn = me.draw(state, N, tm1)
    assert not redrawn
    out = zeros(tm1, N)
    assert _native.mt_draw_coeffs_device(rng, N, tm1, out) is True, f"{what}: the device draw asked for a host redo"
    assert_block(out, cols, what)
    assert rng.getstate() == final, what
    return cols, final


@pytest.mark.parametrize("tm1,N,fam", COEF_CASES)
def test_coefficient_draw_accepts_the_edges(tm1, N, fam):
    """mt_draw_coeffs_device on the ACCEPTED_EDGES cluster: True and the
    reference's coefficients; draw_coeffs_vec and make_shares_vec at t = 4
    (no fused form: the draw, then the split) the same, unflagged."""
    state = accepted_state(fam, N, tm1, False)
    cols, final = coeffs_exact(rng_at(state), state, tm1, N, (tm1, N, fam))
    ss = shamir.SecretShare(tm1 + 1)
    ss.random.setstate(state)
    ss.last_draw_rejected = True
    assert_block(ss.draw_coeffs_vec(N), cols, (tm1, N, fam, "draw_coeffs_vec"))
    assert ss.last_draw_rejected is False and ss.random.getstate() == final
    host, sec = secrets(N)
    ss.random.setstate(state)
    ss.last_draw_rejected = True
    got = ss.make_shares_vec(sec, tm1 + 2, out=zeros(tm1 + 2, N))
    assert_block(got, me.shares_of(cols, host, tm1 + 2), (tm1, N, fam, "make_shares_vec"))
    assert ss.last_draw_rejected is False and ss.random.getstate() == final


@pytest.mark.parametrize("tm1,N,fam", [c for c in COEF_CASES if c[2] != "after"])
def test_coefficient_draw_flags_a_rejected_draw(tm1, N, fam):
    """A rejected value at each spot: mt_draw_coeffs_device returns False and
    leaves the generator alone; draw_coeffs_vec and make_shares_vec (t = 4)
    return the reference's values and state, flagged; the next clean call of
    the same size stays on the device."""
    host, sec = secrets(N)
    for i, state in enumerate(rejected_states(fam, N, tm1, False)):
        cols, final, redrawn = me.draw(state, N, tm1)
        assert redrawn
        ss = shamir.SecretShare(tm1 + 1)
        ss.random.setstate(state)
        assert _native.mt_draw_coeffs_device(ss.random, N, tm1, zeros(tm1, N)) is False, (fam, i)
        assert ss.random.getstate() == state, (fam, i)
        assert_block(ss.draw_coeffs_vec(N), cols, (tm1, N, fam, i, "draw_coeffs_vec"))
        assert ss.last_draw_rejected is True and ss.random.getstate() == final, (fam, i)
        ss.random.setstate(state)
        ss.last_draw_rejected = False
        got = ss.make_shares_vec(sec, tm1 + 2, out=zeros(tm1 + 2, N))
        assert_block(got, me.shares_of(cols, host, tm1 + 2), (tm1, N, fam, i, "make_shares_vec"))
        assert ss.last_draw_rejected is True and ss.random.getstate() == final, (fam, i)
    coeffs_exact(ss.random, final, tm1, N, (tm1, N, fam, "the next call"))


# ------------------------------------------------------------------ the one-wave kernel
@pytest.mark.parametrize("N,acc_fam,rej_fam", [(300, "sub_edge", "group_edge"), (8321, "back_to_fwd", "fwd_to_back")])
@pytest.mark.parametrize("kind", ["fused", "coeffs"])
def test_one_wave_kernel_on_the_same_states(kind, N, acc_fam, rej_fam, monkeypatch):
    """mt_gen_kernel (the tuning library with DN_MT_PC_FORCE=0; the product
    always takes mt_gen_pc_kernel) at t = 3 and for the coefficient draw, in
    both regimes: one accepted-edge state (True, exact) and the rejected states
    of one family (False, generator untouched)."""
    monkeypatch.setenv("DN_MT_PC_FORCE", "0")
    fused = kind == "fused"
    tm1, NN = (2, N) if fused else (3, {300: 300, 8321: 5548}[N])
    with _native.library(_native.TUNING_LIB):
        state = accepted_state(acc_fam, NN, tm1, fused)
        if fused:
            fused_exact(rng_at(state), state, 3, 5, NN, (kind, NN, acc_fam))
        else:
            coeffs_exact(rng_at(state), state, tm1, NN, (kind, NN, acc_fam))
        for state in rejected_states(rej_fam, NN, tm1, fused):
            rng = rng_at(state)
            if fused:
                ok = _native.mt_split_device(rng, secrets(NN)[1], zeros(5, NN), NN, 3, 5)
            else:
                ok = _native.mt_draw_coeffs_device(rng, NN, tm1, zeros(tm1, NN))
            assert ok is False and rng.getstate() == state, (kind, NN, rej_fam)
        final = me.draw(state, NN, tm1)[1]
        if fused:
            fused_exact(rng_at(final), final, 3, 5, NN, (kind, NN, "the next call"))
        else:
            coeffs_exact(rng_at(final), final, tm1, NN, (kind, NN, "the next call"))


# ------------------------------------------------------------------ speculation and a rejected draw
def test_rejected_draw_disarms_an_armed_speculation(monkeypatch):
    """Tuning library, DN_MT_SPEC_MIN=0: two clean calls arm a speculation on
    the third, whose stream holds a rejected value.  The third call uses the
    speculated windows (a hit), is flagged by the kernel, returns False with
    the generator untouched and leaves nothing armed; make_shares_vec redoes
    it exactly, and the calls after it are exact and on the device again."""
    t, n, N = 3, 5, 8321
    ncoef = N * (t - 1)
    host, sec = secrets(N)
    spot = 2 * ncoef + me.positions(N, t - 1)["back_top"][1]
    state = me.craft_state({spot: (me.REJECTED[1], 0)}, spot, 333, seed="spec")
    monkeypatch.setenv("DN_MT_SPEC_MIN", "0")
    with _native.library(_native.TUNING_LIB):
        ss = shamir.SecretShare(t)
        ss.random.setstate(state)
        for i in range(2):
            state = fused_exact(ss.random, state, t, n, N, ("spec", i))
        s0 = _native.mt_spec_stats()
        assert s0["armed"]
        assert _native.mt_split_device(ss.random, sec, zeros(n, N), N, t, n) is False
        s1 = _native.mt_spec_stats()
        assert s1["hits"] == s0["hits"] + 1 and not s1["armed"], (s0, s1)
        assert ss.random.getstate() == state
        want, final = me.reference(state, N, t, n, host)
        got = ss.make_shares_vec(sec, n, out=zeros(n, N))
        assert ss.last_draw_rejected is True
        assert_block(got, want, "the rejected call, redone")
        assert ss.random.getstate() == final and not _native.mt_spec_stats()["armed"]
        for i in range(3):
            final = fused_exact(ss.random, final, t, n, N, ("spec after", i))
        s2 = _native.mt_spec_stats()
        assert s2["armed"] and s2["hits"] >= s1["hits"] + 1, (s1, s2)


# ------------------------------------------------------------------ the tensor list
MANY_LISTS = {"small": [70, 63, 1, 200, 64, 30], "big": [70, 63, 1, 200, 64, 8000]}


def many_setup(sizes, n):
    N = sum(sizes)
    host, sec = secrets(N)
    tensors = list(torch.split(sec, sizes))
    outs = [zeros(n, k) for k in sizes]
    return N, host, sec, tensors, outs


def assert_many(outs, want_rows, sizes, what):
    e = 0
    for k, (out, size) in enumerate(zip(outs, sizes)):
        assert_block(out, [r[e:e + size] for r in want_rows], (what, "tensor", k))
        e += size


@pytest.mark.parametrize("which", list(MANY_LISTS))
def test_many_flags_a_rejected_draw(which):
    """make_shares_vec_many at t = 3, n = 5 over sizes that cut the 64-element
    groups, with a rejected draw in the first tensor, in the one-element
    tensor and in the last tensor: mt_split_many_device returns False with the
    generator untouched, and the call returns every tensor's reference shares
    and the reference's final state, flagged."""
    t, n = 3, 5
    sizes = MANY_LISTS[which]
    N, host, sec, tensors, _ = many_setup(sizes, n)
    for i, elem in enumerate((10, 70 + 63, N - 5)):
        d = elem * (t - 1) + i % 2
        state = me.craft_state({d: me.REJECTED[(i + 1) % 2]}, d, 333, seed=f"many-{which}-{i}")
        want, final = me.reference(state, N, t, n, host)
        ss = shamir.SecretShare(t)
        ss.random.setstate(state)
        outs = [zeros(n, k) for k in sizes]
        segs = [(k, o.data_ptr()) for k, o in zip(sizes, outs)]
        assert _native.mt_split_many_device(ss.random, sec, segs, t, n) is False, (which, elem)
        assert ss.random.getstate() == state
        outs = [zeros(n, k) for k in sizes]
        got = ss.make_shares_vec_many(tensors, n, outs=outs)
        assert ss.last_draw_rejected is True
        assert_many(got, want, sizes, (which, elem))
        assert ss.random.getstate() == final
    outs = [zeros(n, k) for k in sizes]
    want, after = me.reference(final, N, t, n, host)
    assert _native.mt_split_many_device(ss.random, sec, [(k, o.data_ptr()) for k, o in zip(sizes, outs)], t, n) is True
    assert_many(outs, want, sizes, (which, "the next call"))
    assert ss.random.getstate() == after


@pytest.mark.parametrize("which", list(MANY_LISTS))
@pytest.mark.parametrize("boundary", [70, 70 + 63])
def test_many_accepts_the_edges_across_a_tensor_boundary(which, boundary):
    """The ACCEPTED_EDGES cluster over the draws of the elements on both sides
    of a tensor boundary inside one 64-element group (elements 64 .. 127 hold
    the end of tensor 0 and the start of tensor 1; 128 .. 191 the end of tensor
    1, the one-element tensor and the start of the next: emit_pieces):
    mt_split_many_device returns True and every tensor is exact."""
    t, n = 3, 5
    sizes = MANY_LISTS[which]
    N, host, sec, _, outs = many_setup(sizes, n)
    first = boundary * (t - 1) - len(me.ACCEPTED_EDGES) // 2
    state = me.craft_state(me.ACCEPTED_EDGES, first, 623, seed=f"many-acc-{boundary}")
    want, final = me.reference(state, N, t, n, host)
    rng = rng_at(state)
    segs = [(k, o.data_ptr()) for k, o in zip(sizes, outs)]
    assert _native.mt_split_many_device(rng, sec, segs, t, n) is True
    assert_many(outs, want, sizes, (which, boundary))
    assert rng.getstate() == final


# ------------------------------------------------------------------ the sharded device draw
def test_sharded_device_draw():
    """draw_coeffs_vec(hi - lo, elem_offset=lo, n_total=n) on the device: a
    rejected draw inside the shard is flagged and the slice is the reference's;
    one after the shard leaves it unflagged, on the device and exact."""
    n, lo, hi, tm1 = 600, 256, 512, 2
    for where, flagged in ((lo * tm1, True), (300 * tm1 + 1, True), (hi * tm1 - 1, True), (hi * tm1, False),
                           (550 * tm1, False)):
        state = me.craft_state({where: me.REJECTED[where % 2]}, where, 333, seed=where)
        cols = me.draw(state, n, tm1)[0]
        ss = shamir.SecretShare(tm1 + 1)
        ss.random.setstate(state)
        got = ss.draw_coeffs_vec(hi - lo, elem_offset=lo, n_total=n)
        assert ss.last_draw_rejected is flagged, where
        assert_block(got, [c[lo:hi] for c in cols], ("shard", where))
        assert ss.random.getstate() == me.skip_state(state, 17 * tm1 * n)
