"""The MT19937 coefficient draw's host side at real rejected draws and crafted
coefficient words (tests/mt_edges.py builds the generator states; CPython's own
randint is the reference).  No device: the helper's self-checks, the host C
draw (dn_mt19937_draw_coeffs, whose redraw test ge_p_minus_1 a seeded
generator never reaches), draw_coeffs_vec on the host with its
last_draw_rejected flag, the sharded draw in one process and over gloo.
The device draw on the same states: tests/test_gpu_mt_edges.py."""
import os
import random
import socket

import numpy as np
import pytest
import torch

import mt_edges as me
from delta_node.crypto import shamir
from delta_node.crypto.shamir import _native, field

REJ = me.REJECTED


def block_of(cols):
    return np.stack([field.ints_to_vec(c) for c in cols])


def straddling_draw(index: int) -> int:
    """The first draw whose 17 words lie on both sides of a 624-word regeneration."""
    d = 0
    while (index + 17 * d) // 624 == (index + 17 * d + 16) // 624:
        d += 1
    return d


# ------------------------------------------------------------------ the helper
@pytest.mark.parametrize("first_draw,index", [(0, 624), (0, 100), (3, 100), (30, 100), (36, 624), (16641, 333)])
def test_crafted_draws_come_out_of_cpython(first_draw, index):
    """getrandbits(521) returns the cluster at its draws — at draw 0, inside
    the caller's own array (index 100: 17 * 17 words from word 151 on), across
    the regeneration (draw 30 from index 100 is words 610 .. 626; draw 36 from
    624 is 1236 .. 1252) and 16641 draws on — and randint redraws exactly the
    rejected values.  (craft_state asserts the same before it returns.)"""
    cluster = me.ACCEPTED_EDGES + me.REJECTED
    if (first_draw, index) == (3, 100):
        assert 17 * first_draw + 17 * len(cluster) <= 624 - index  # no word of it is regenerated
    state = me.craft_state(cluster, first_draw, index, seed=first_draw + index)
    assert state[1][624] == index and len(state[1]) == 625
    rng = random.Random()
    rng.setstate(state)
    for _ in range(first_draw):
        rng.getrandbits(521)
    assert [rng.getrandbits(521) for _ in cluster] == [me.raw(v) for v in cluster]
    rng.setstate(state)
    for _ in range(first_draw):
        rng.getrandbits(521)
    got = [rng.randint(1, me.P - 1) for _ in range(len(me.ACCEPTED_EDGES) + 1)]
    assert got[:-1] == [me.raw(v) + 1 for v in me.ACCEPTED_EDGES]  # the last one skipped both rejected draws
    assert me.ACCEPTED_EDGES[0] == me.P - 2 and got[0] == me.P - 1 and got[9] == 1 and got[8] == 1 << 512


def test_straddling_cluster_straddles():
    for index in (624, 100, 333):
        d = straddling_draw(index)
        lo, hi = index + 17 * d, index + 17 * d + 16
        assert lo // 624 + 1 == hi // 624 and hi - lo == 16 and d > 0, (index, d)


def test_uncrafted_draws_come_from_the_seed():
    """The draws before the cluster differ between seeds (the helper pins the
    cluster, not the stream), and one seed gives one state."""
    a = me.craft_state(me.REJECTED, 40, 333, seed=1)
    b = me.craft_state(me.REJECTED, 40, 333, seed=2)
    assert a == me.craft_state(me.REJECTED, 40, 333, seed=1)
    ra, rb = random.Random(), random.Random()
    ra.setstate(a)
    rb.setstate(b)
    da, db = [ra.getrandbits(521) for _ in range(42)], [rb.getrandbits(521) for _ in range(42)]
    assert da[40:] == db[40:] == me.REJECTED
    assert all(x != y for x, y in zip(da[:40], db[:40]))


def test_dict_draws_and_low_bits():
    """Separate crafted draws with seeded ones between them, and the dropped
    low 23 bits of the 17th word as asked."""
    state = me.craft_state({5: (me.ONES, 0), 9: (me.ONES - 1, 0x7FFFFF), 11: 7}, 5, 600, seed=3, low23=0x2AAAAA)
    rng = random.Random()
    rng.setstate(state)
    words = [rng.getrandbits(32) for _ in range(17 * 12)]
    assert words[17 * 5 + 16] == 0xFF800000 and words[17 * 9 + 16] == 0xFFFFFFFF
    assert words[17 * 11 + 16] == 0x2AAAAA and words[17 * 11] == 7
    assert me.temper(me.untemper(0x12345678)) == 0x12345678


def test_positions_follow_the_substream_geometry():
    """The (t, n, N) shapes of test_gpu_mt_edges.py are the smallest of their
    regimes: 300 / 200 elements are 2^8-draw substreams with a partial last
    group, and 8321 x 2 = 16642, 4161 x 4 = 16644 and 16641 x 1 are the first
    sizes past 65 * 2^8 = 16640 coefficients (seventeen 2^10-draw substreams,
    2 .. 14 backward)."""
    assert me.geometry(300, 2, True) == (600, 256, 3, 128, [])
    assert me.geometry(200, 4, True) == (800, 256, 4, 256, [])
    assert me.geometry(8320, 2, True)[1:3] == (256, 65)
    for n, tm1 in ((8321, 2), (4161, 4), (16641, 1)):
        ncoef, D, S, G, backward = me.geometry(n, tm1, True)
        assert (D, S, backward) == (1024, 17, [2, 4, 6, 8, 10, 12, 14]) and me.geometry(n - 1, tm1, True)[1] == 256
    assert me.geometry(5548, 3, False) == (16644, 1024, 17, 64, [2, 4, 6, 8, 10, 12, 14])
    pos = me.positions(8321, 2)
    assert pos["group_edge"] == [127, 128] and pos["fwd_to_back"] == [2047, 2048] and pos["back_to_fwd"] == [3071, 3072]
    assert pos["back_top"] == [3072 - 128 - 1, 3072 - 128] and pos["last"] == [16640, 16641] and pos["after"] == [16642]
    assert "group_edge" not in me.positions(200, 4) and "fwd_to_back" not in me.positions(300, 2)
    assert set(pos) <= set(me.FAMILY_INDEX)


# ------------------------------------------------------------------ the host C draw
N_HOST = 60  # elements: with one coefficient each, 60 draws reach past a cluster on the straddling draw


def host_cases(tm1: int, index: int):
    """name -> {stream draw: value}: where the rejected values sit."""
    ncoef = N_HOST * tm1
    e = N_HOST // 2
    sd = straddling_draw(index)
    assert sd < ncoef - 3
    cases = {}
    for k, v in enumerate(REJ):
        cases.update({
            f"first-{k}": {0: v}, f"middle-{k}": {ncoef // 2: v}, f"last-{k}": {ncoef - 1: v},
            f"slot0-{k}": {e * tm1: v}, f"slot_last-{k}": {e * tm1 + tm1 - 1: v},
            f"straddle-{k}": {sd: v},
            # a draw after the call: not consumed
            f"after-{k}": {ncoef: v},
        })
    cases["two_in_a_row"] = {7: REJ[1], 8: REJ[0]}
    cases["three_in_a_row"] = {sd - 1: REJ[0], sd: REJ[1], sd + 1: REJ[1]}
    cases["last_twice"] = {ncoef - 1: REJ[1], ncoef: REJ[1]}
    return cases


@pytest.mark.parametrize("index", [624, 333])
@pytest.mark.parametrize("tm1", [1, 2, 4])
def test_host_draw_redraws_as_randint(tm1, index):
    """dn_mt19937_draw_coeffs on states with rejected raw values (p and p - 1)
    at the first, a middle and the last draw, at coefficient 1 and t - 1 of an
    element, across the regeneration, two and three in a row, and at the draw
    after the call: coefficients and final state are randint's."""
    for name, draws in host_cases(tm1, index).items():
        state = me.craft_state(draws, min(draws), index, seed=f"{name}-{tm1}")
        cols, final, redrawn = me.draw(state, N_HOST, tm1)
        assert redrawn == (not name.startswith("after")), name
        rng = random.Random()
        rng.setstate(state)
        got = _native.mt_draw_coeffs(rng, N_HOST, tm1)
        assert np.array_equal(got, block_of(cols)), (name, tm1, index)
        assert rng.getstate() == final, (name, tm1, index)


@pytest.mark.parametrize("index", [624, 333])
@pytest.mark.parametrize("tm1", [1, 2, 4])
def test_host_draw_accepts_the_edges(tm1, index):
    """The ACCEPTED_EDGES cluster at draw 0, across the regeneration and at
    the end of the call: no redraw, coefficients raw + 1 limb for limb."""
    ncoef = N_HOST * tm1
    k = len(me.ACCEPTED_EDGES)
    for first in (0, straddling_draw(index) - 3, ncoef - k):
        state = me.craft_state(me.ACCEPTED_EDGES, first, index, seed=first)
        cols, final, redrawn = me.draw(state, N_HOST, tm1)
        assert not redrawn
        flat = [cols[d % tm1][d // tm1] for d in range(first, first + k)]
        assert flat == [me.raw(v) + 1 for v in me.ACCEPTED_EDGES]
        rng = random.Random()
        rng.setstate(state)
        assert np.array_equal(_native.mt_draw_coeffs(rng, N_HOST, tm1), block_of(cols)), (first, tm1, index)
        assert rng.getstate() == final


# ------------------------------------------------------------------ draw_coeffs_vec on the host
class Replaying(random.Random):
    """A generator that is not plain MT19937 to the library (it overrides
    getrandbits) but replays the same stream."""

    def getrandbits(self, k):
        return super().getrandbits(k)


@pytest.mark.parametrize("tm1", [1, 2, 4])
def test_draw_coeffs_vec_flags_exactly_the_redraws(tm1):
    """last_draw_rejected is True exactly when the reference consumed more
    than 17 (t - 1) n words, False on the accepted edges and on a rejected value
    behind the call; a generator served by the reference's own calls
    (_draw_coeffs_generic) draws the same coefficients."""
    ncoef = N_HOST * tm1
    cases = dict(host_cases(tm1, 333))
    cases["accepted"] = {ncoef - len(me.ACCEPTED_EDGES) + i: v for i, v in enumerate(me.ACCEPTED_EDGES)}
    for name, draws in cases.items():
        state = me.craft_state(draws, min(draws), 333, seed=name)
        cols, final, redrawn = me.draw(state, N_HOST, tm1)
        assert redrawn == (name != "accepted" and not name.startswith("after"))
        ss = shamir.SecretShare(tm1 + 1)
        ss.random.setstate(state)
        ss.last_draw_rejected = not redrawn
        got = ss.draw_coeffs_vec(N_HOST, device="cpu")
        assert ss.last_draw_rejected is redrawn, name
        assert np.array_equal(got.numpy(), block_of(cols)) and ss.random.getstate() == final, name
        ss.random = Replaying()
        ss.random.setstate(state)
        assert not _native.mt_compatible(ss.random)
        got = ss.draw_coeffs_vec(N_HOST, device="cpu")
        assert np.array_equal(got.numpy(), block_of(cols)) and ss.random.getstate() == final, name


def test_sharded_draw_in_one_process():
    """draw_coeffs_vec(hi - lo, elem_offset=lo, n_total=n): a rejected draw
    inside [lo, hi) is flagged and the slice is the reference's (redrawn where
    the reference redraws); one after hi leaves the shard unflagged and exact."""
    n, lo, hi, tm1 = 600, 256, 512, 2
    for where, flagged in ((lo * tm1, True), (300 * tm1 + 1, True), (hi * tm1 - 1, True), (hi * tm1, False),
                           (550 * tm1, False)):
        for v in REJ:
            state = me.craft_state({where: v}, where, 333, seed=where)
            cols, _, redrawn = me.draw(state, n, tm1)
            assert redrawn
            ss = shamir.SecretShare(tm1 + 1)
            ss.random.setstate(state)
            got = ss.draw_coeffs_vec(hi - lo, device="cpu", elem_offset=lo, n_total=n)
            assert ss.last_draw_rejected is flagged, where
            assert np.array_equal(got.numpy(), block_of([c[lo:hi] for c in cols])), where
            assert ss.random.getstate() == me.skip_state(state, 17 * tm1 * n)  # (the ranks' common end without a redraw)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def gloo_cases(n: int, tm1: int, world: int):
    """A rejected draw in rank 0's range, one in the last rank's, and the
    accepted edges (no rank redraws)."""
    from delta_node.crypto.shamir import dist as sd

    lo, hi = sd.shard_range(n, world - 1, world)
    assert lo < hi - 10
    return [({5 * tm1 + 1: REJ[1]}, True), ({(hi - 6) * tm1: REJ[0]}, True),
            ({lo * tm1 - 7 + i: v for i, v in enumerate(me.ACCEPTED_EDGES)}, False)]


def _gloo_worker(rank, world, port, n, t, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(root, "delta-node_amd"), os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist

    from delta_node.crypto.shamir import dist as sd

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        oks = []
        for draws, redraws in gloo_cases(n, t - 1, world):
            state = me.craft_state(draws, min(draws), 333, seed=world)
            cols, final, redrawn = me.draw(state, n, t - 1)
            ss = shamir.SecretShare(t)
            ss.random.setstate(state)
            blk = sd.draw_coeffs_sharded(ss, n, device="cpu")
            lo, hi = sd.shard_range(n, rank, world)
            want = np.zeros(tuple(blk.shape), dtype=np.uint8)
            if hi > lo:
                want[:, : field.vec_bytes(hi - lo)] = block_of([c[lo:hi] for c in cols])
            oks.append(redrawn == redraws and np.array_equal(blk.numpy(), want) and ss.random.getstate() == final)
        q.put((rank, oks))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_draw_over_gloo(world):
    """dist.draw_coeffs_sharded with a rejected draw in rank 0's range, in the
    last rank's range, and with the accepted edges: every rank's slice is the
    reference's and every rank's ss.random ends in the reference's final state."""
    import torch.multiprocessing as mp

    n, t = 1300, 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, world, port, n, t, q)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(180)
    assert all(p.exitcode == 0 for p in procs)
    res = [q.get(timeout=10) for _ in range(world)]
    assert sorted(r for r, _ in res) == list(range(world))
    assert all(all(oks) and len(oks) == 3 for _, oks in res), res
