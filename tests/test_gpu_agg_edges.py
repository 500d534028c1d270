"""The int64 member sum (csrc/sum_i64.hip, utils/agg.py) at its edges: sizes
across the 64-, 512- and 2048-pair steps of the kernel with an odd last
element, member counts across the 16-input launch, `out=` aliasing, int64 views
that are only 8-byte aligned, and the stride loop.  Against numpy's wrapping
`+`, bit for bit."""
import numpy as np
import pytest
import torch

import mask_edges as me
from delta_node import utils
from delta_node.utils import _mask_native as mn

pytestmark = pytest.mark.gpu
SENT = 0x5A5A5A5A5A5A5A5A


def members(k: int, n: int, seed: int) -> np.ndarray:
    """k full-range int64 rows; the first columns hold pairs whose sum wraps."""
    a = np.random.default_rng(seed).integers(me.INT64_MIN, me.INT64_MAX, size=(k, n), dtype=np.int64, endpoint=True)
    a[0, 0] = me.INT64_MAX
    if k > 1:
        a[1, 0] = 1  # INT64_MAX + 1
        a[:, n - 1] = me.INT64_MIN  # the (odd) last element: k * INT64_MIN
    return a


def numpy_sum(rows) -> np.ndarray:
    acc = np.array(rows[0], dtype=np.int64, copy=True)
    for r in rows[1:]:
        acc = acc + r  # int64 arrays wrap
    return acc


def odd_view(row: np.ndarray) -> torch.Tensor:
    """A device copy of `row` that starts at element 1 of its buffer: 8-byte aligned only."""
    buf = torch.full((row.size + 3,), SENT, dtype=torch.int64, device="cuda")
    v = buf[1:1 + row.size]
    v.copy_(torch.from_numpy(row))
    assert v.data_ptr() % 16 == 8 and v.is_contiguous()
    return v


@pytest.mark.parametrize("k", me.SUM_KS)
def test_sum_int64_sizes_and_counts(k):
    for n in me.SUM_NS:
        a = members(k, n, 1000 * k + n)
        got = utils.sum_int64([torch.from_numpy(r) for r in a])
        assert got.shape == (n,) and np.array_equal(got.cpu().numpy(), numpy_sum(a)), (k, n)


@pytest.mark.parametrize("k", [1, 3, 16, 17, 32])
@pytest.mark.parametrize("n", [1, 2, 129, 231, 4097])
def test_sum_int64_out_and_alignment(k, n):
    a = members(k, n, 7 * k + n)
    want = numpy_sum(a)
    dev = [torch.from_numpy(r).cuda() for r in a]
    # out is the first input (accumulate in place)
    first = dev[0].clone()
    got = utils.sum_int64([first] + dev[1:], out=first)
    assert got.data_ptr() == first.data_ptr() and np.array_equal(first.cpu().numpy(), want)
    # a misaligned out: written in full, nothing beside it
    buf = torch.full((n + 3,), SENT, dtype=torch.int64, device="cuda")
    out = buf[1:1 + n]
    assert out.data_ptr() % 16 == 8
    got = utils.sum_int64(dev, out=out)
    assert got.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), want)
    assert int(buf[0]) == SENT and bool((buf[n + 1:] == SENT).all())
    # misaligned inputs: every one, and only one in the middle
    views = [odd_view(r) for r in a]
    assert np.array_equal(utils.sum_int64(views).cpu().numpy(), want)
    mixed = list(dev)
    mixed[k // 2] = views[k // 2]
    assert np.array_equal(utils.sum_int64(mixed).cpu().numpy(), want)
    for v, r in zip(views, a):  # the inputs are left as they were
        assert np.array_equal(v.cpu().numpy(), r)
    # a misaligned out that is also the first (misaligned) input
    got = utils.sum_int64(views, out=views[0])
    assert got.data_ptr() == views[0].data_ptr() and np.array_equal(views[0].cpu().numpy(), want)


@pytest.mark.parametrize("k", [2, 5, 17])
def test_sum_member_results_over_flat_buffers(k):
    """Each member's results are views carved out of one received buffer, with
    odd sizes: every other view starts 8-byte aligned only."""
    shapes = {"w": {"a": (33, 7), "b": (5,), "c": (1001,)}, "v": {"d": (3, 3), "e": (1,), "f": (64,)}}
    total = sum(int(np.prod(s)) for keys in shapes.values() for s in keys.values())
    rng = np.random.default_rng(k)
    flats = [rng.integers(me.INT64_MIN, me.INT64_MAX, size=total, dtype=np.int64, endpoint=True) for _ in range(k)]
    results, misaligned = [], 0
    for flat in flats:
        buf, off, res = torch.from_numpy(flat).cuda(), 0, {}
        for var, keys in shapes.items():
            res[var] = {}
            for key, shp in keys.items():
                cnt = int(np.prod(shp))
                res[var][key] = buf[off:off + cnt].reshape(shp)
                misaligned += res[var][key].data_ptr() % 16 == 8
                off += cnt
        results.append(res)
    assert misaligned >= 2 * k
    valid, got = utils.sum_member_results(results, ["w", "v"])
    assert valid == list(range(k))
    off = 0
    for var, keys in shapes.items():
        for key, shp in keys.items():
            cnt = int(np.prod(shp))
            want = numpy_sum([f[off:off + cnt] for f in flats]).reshape(shp)
            assert got[var][key].shape == shp and np.array_equal(got[var][key].cpu().numpy(), want), (var, key)
            off += cnt


def test_sum_stride_loop_product_build():
    """n / 2 > 8192 workgroups x 2048 pairs: the kernel's stride loop takes a
    second step (and n is odd).  Compared on the device with torch's wrapping add."""
    n = me.BIG_SUM_N
    assert n % 2 == 1 and n // 2 > 8192 * 2048
    g = torch.Generator(device="cuda").manual_seed(25)
    # random_ fills [0, 2^63); an odd multiplier (wrapping) spreads it over the full int64 range
    a = torch.empty(n, dtype=torch.int64, device="cuda").random_(generator=g).mul_(-7046029254386353131)
    b = torch.empty(n, dtype=torch.int64, device="cuda").random_(generator=g).mul_(-7046029254386353131)
    a[-1], b[-1] = me.INT64_MAX, 1
    got = utils.sum_int64([a, b])
    assert torch.equal(got, a + b)
    assert int(got[-1]) == me.INT64_MIN
    del a, b, got
    torch.cuda.empty_cache()


def test_dn_i64_sum_refusals():
    out = torch.full((8,), SENT, dtype=torch.int64, device="cuda")
    x = torch.arange(10, dtype=torch.int64, device="cuda")
    with pytest.raises(NotImplementedError):
        mn.i64_sum([], out, 8)
    with pytest.raises(NotImplementedError):
        mn.i64_sum([x[:8]] * 17, out, 8)
    # the C entry point keeps its 16-byte rule (agg.sum_int64 stages such views)
    with pytest.raises(ValueError):
        mn.i64_sum([x[1:9]], out, 8)
    with pytest.raises(ValueError):
        mn.i64_sum([x[:6]], out[1:7], 6)
    mn.i64_sum([x[:8]], out, 0)  # nothing to do
    with pytest.raises(ValueError):
        utils.sum_int64([])
    with pytest.raises(TypeError):
        utils.sum_int64([x.to(torch.int32)])
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
