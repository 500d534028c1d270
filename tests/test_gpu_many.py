"""make_shares_vec_many (MI355X): one fused draw + split over a list of tensors.

The reference draws every coefficient from one sequential MT19937 stream
(shamir.py:59-61) and its runner splits a model tensor by tensor
(runner/horizontal/agg.py:294-316), so the many-call must equal the per-tensor
make_shares_vec loop element for element, with the same final generator state,
each tensor's shares in that tensor's own tiled block.  Checked here against
that loop, against the reference's own golden outputs and digests, and for
writes outside the blocks.  The n_k real elements of every row are compared;
padding lanes of a last tile are unspecified, as in make_shares_vec.
"""
import importlib.util
import os
import random

import numpy as np
import pytest
import torch

from delta_node.crypto import shamir
from delta_node.crypto.shamir import _native, field
from golden.fixtures import P, chunk_digests, combine_digests, load_npz, manifest, secrets_int64

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ragged: tiny segments, a group spanning four segments (1, 1, 1 and the start
# of 300), an empty tensor; 8861 elements = 17722 coefficients at t = 3 (above
# the 65 * 2^8 bound: ~18 substreams of 2^10 draws, backward ones in the middle)
LIST_A = [1, 63, 64, 65, 0, 127, 128, 1, 1, 1, 300, 257, 256, 1000, 4097, 2500]
# (5, 9): 1704 elements = 6816 coefficients, 2^8-draw substreams of one group each
LIST_A59 = LIST_A[:11] + [700]
# every size a multiple of 64, some not of 256: the single-tile stores with per-segment bases
LIST_B = [64, 192, 256, 320, 1024, 4096, 2048, 832]


def dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _native.lib()


def block_limbs(block: torch.Tensor, n: int) -> np.ndarray:
    """uint8 [S, vec_bytes(n)] device block -> uint32 [S, n, 17] (the n real elements)."""
    h = block.cpu().numpy()
    if n == 0:
        return np.zeros((h.shape[0], 0, 17), dtype=np.uint32)
    return np.stack([field.vec_to_limbs(h[s], n) for s in range(h.shape[0])])


def gathered_planes(outs, sizes) -> np.ndarray:
    """The pieces' blocks as uint32 [S, 17, sum sizes] limb planes, pieces in order."""
    S = outs[0].shape[0]
    planes = np.empty((S, 17, sum(sizes)), dtype=np.uint32)
    off = 0
    for out, n in zip(outs, sizes):
        if n:
            h = out.cpu().numpy()
            for s in range(S):
                planes[s, :, off:off + n] = field.vec_to_planes(h[s], n)
            off += n
    return planes


def cut(vec: np.ndarray, sizes):
    """`vec` cut into consecutive pieces: host and device tensors alternating,
    a composite size as a 2-D tensor (each is read flattened in C order)."""
    pieces, off = [], 0
    for k, n in enumerate(sizes):
        x = torch.from_numpy(vec[off:off + n].copy())
        if n and n % 5 == 0:
            x = x.reshape(5, n // 5)
        pieces.append(x.to(dev()) if k % 2 else x)
        off += n
    assert off == len(vec)
    return pieces


def pair(t: int, seed: int):
    a, b = shamir.SecretShare(t), shamir.SecretShare(t)
    a.random.seed(seed)
    b.random.seed(seed)
    return a, b


def assert_equal_lists(got, want, sizes, shares):
    assert len(got) == len(want) == len(sizes)
    for k, (g, w, n) in enumerate(zip(got, want, sizes)):
        assert g.dtype == torch.uint8 and g.is_cuda and g.is_contiguous(), k
        assert tuple(g.shape) == (shares, field.vec_bytes(n)), k
        assert np.array_equal(block_limbs(g, n), block_limbs(w, n)), (k, n)


def _not_the_loop(*args, **kwargs):
    raise AssertionError("make_shares_vec_many fell back to the per-tensor loop")


# ------------------------------------------------------------ 1. equals the sequential calls
@pytest.mark.parametrize("t,n,sizes", [(3, 5, LIST_A), (3, 7, LIST_A), (2, 3, LIST_A), (5, 9, LIST_A59),
                                       (3, 5, LIST_B), (3, 7, LIST_B), (2, 3, LIST_B), (5, 9, LIST_B)],
                         ids=["A-3of5", "A-3of7", "A-2of3", "A-5of9", "B-3of5", "B-3of7", "B-2of3", "B-5of9"])
def test_many_equals_sequential_calls(t, n, sizes, monkeypatch):
    tensors = cut(secrets_int64(100 * t + n, sum(sizes)), sizes)
    a, b = pair(t, 4242 + t)
    monkeypatch.setattr(a, "make_shares_vec", _not_the_loop)  # these shapes take the fused many-form
    got = a.make_shares_vec_many(tensors, n)
    want = [b.make_shares_vec(x, n) for x in tensors]
    assert_equal_lists(got, want, sizes, n)
    assert a.random.getstate() == b.random.getstate()
    assert not a.last_draw_rejected


def test_many_default_outs_are_views_of_one_block_and_secrets_pass_through():
    """Default outs: contiguous views laid back to back in one block.  Inputs
    that are consecutive views of one device buffer (no concatenation copy)
    give the same result as separate tensors."""
    sizes = LIST_A
    flat = torch.from_numpy(secrets_int64(11, sum(sizes))).to(dev())
    views = list(torch.split(flat, sizes))
    a, b = pair(3, 99)
    got = a.make_shares_vec_many(views, 5)
    want = [b.make_shares_vec(x.clone(), 5) for x in views]
    assert_equal_lists(got, want, sizes, 5)
    assert a.random.getstate() == b.random.getstate()
    ptr = got[0].data_ptr()
    for k, n in enumerate(sizes):
        if n:  # (an empty view has no address)
            assert got[k].data_ptr() == ptr, k
            ptr += 5 * field.vec_bytes(n)


# ------------------------------------------------------------ 2. nothing outside the blocks
def test_many_writes_nothing_outside_its_blocks():
    sizes, shares, guard = LIST_A, 5, 4096
    vbs = [field.vec_bytes(n) for n in sizes]
    total = guard + sum(shares * vb + guard for vb in vbs)
    buf = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev())
    outs, gaps, off = [], [(0, guard)], guard
    for vb in vbs:
        outs.append(buf[off:off + shares * vb].view(shares, vb))
        off += shares * vb
        gaps.append((off, off + guard))
        off += guard
    assert off == total
    tensors = cut(secrets_int64(21, sum(sizes)), sizes)
    a, b = pair(3, 555)
    a.make_shares_vec = _not_the_loop
    got = a.make_shares_vec_many(tensors, shares, outs=outs)
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, outs))
    h = buf.cpu().numpy()
    for lo, hi in gaps:
        assert (h[lo:hi] == 0xA5).all(), (lo, hi)
    assert_equal_lists(got, [b.make_shares_vec(x, shares) for x in tensors], sizes, shares)


# ------------------------------------------------------------ 3. reference pins
@pytest.mark.parametrize("key,sizes", [("f1", [1, 200, 63, 500, 260]), ("f2", [100, 1, 155])])
def test_many_matches_reference_shares(key, sizes):
    cfg = manifest()[key]
    z = load_npz(cfg["file"])
    N, t, n = cfg["N"], cfg["t"], cfg["n"]
    assert sum(sizes) == N
    ss = shamir.SecretShare(t)
    ss.random.seed(cfg["mt_seed"])
    ss.make_shares_vec = _not_the_loop
    outs = ss.make_shares_vec_many(cut(z["secrets"], sizes), n)
    got = np.concatenate([block_limbs(o, k) for o, k in zip(outs, sizes)], axis=1)  # [n, N, 17]
    assert np.array_equal(got.transpose(1, 0, 2), z["share_limbs"])
    r = random.Random(cfg["mt_seed"])
    for _ in range(N * (t - 1)):
        r.randint(1, P - 1)
    assert ss.random.getstate() == r.getstate()


@pytest.mark.parametrize("name", ["split_t3n5_2e16", "split_t5n9_2e16"])
def test_many_2e16_reference_digests(name):
    d = [d for d in manifest()["digests"] if d["name"] == name][0]
    N = d["N"]
    cuts = [0] + sorted(random.Random(7).sample(range(1, N), 23)) + [N]
    sizes = [hi - lo for lo, hi in zip(cuts, cuts[1:])]
    ss = shamir.SecretShare(d["t"])
    ss.random.seed(d["mt_seed"])
    outs = ss.make_shares_vec_many(cut(secrets_int64(d["secret_seed"], N), sizes), d["n"])
    assert combine_digests(chunk_digests(gathered_planes(outs, sizes))) == d["digest"]


# ------------------------------------------------------------ 4. full size
def _measure_many():
    spec = importlib.util.spec_from_file_location("measure_many", os.path.join(ROOT, "scripts", "measure_many.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.slow
def test_many_2e24_ragged_mix_reference_digest():
    """The ragged 127-tensor mix of scripts/measure_many.py (2^24 elements,
    3-of-5, MT seed 1) against the reference's own 2^24 digest: the only case
    that reaches the 2^12- and 2^14-draw substream lengths."""
    d = [d for d in manifest()["digests"] if d["name"] == "split_t3n5_2e24"][0]
    sizes = _measure_many().mix_sizes(ragged=True)
    assert sum(sizes) == d["N"] == 1 << 24 and len(sizes) == 127
    flat = torch.from_numpy(secrets_int64(d["secret_seed"], d["N"])).to(dev())
    ss = shamir.SecretShare(3)
    ss.random.seed(d["mt_seed"])
    outs = ss.make_shares_vec_many(list(torch.split(flat, sizes)), 5)
    assert combine_digests(chunk_digests(gathered_planes(outs, sizes))) == d["digest"]


# ------------------------------------------------------------ 5. speculation is blind to segmentation
def test_speculation_is_blind_to_segmentation():
    """Four consecutive many-calls of 2^16 elements in four different
    segmentations speculate and hit as four plain make_shares_vec(2^16) calls
    do; every output equals the host draw + split."""
    N, t, n = 1 << 16, 3, 5
    sec = torch.from_numpy(secrets_int64(31, N)).to(dev())

    def host_shares(rng):
        co = torch.from_numpy(_native.mt_draw_coeffs(rng, N, t - 1)).to(dev())
        want = torch.zeros((n, field.vec_bytes(N)), dtype=torch.uint8, device=dev())
        _native.split_u64(sec, co, want, N, t, n)
        return block_limbs(want, N)

    def hits():
        return _native.mt_spec_stats()["hits"]

    plain, ref = pair(t, 8001)
    h0 = hits()
    for i in range(4):
        got = plain.make_shares_vec(sec, n)
        assert np.array_equal(block_limbs(got, N), host_shares(ref.random)), i
        assert plain.random.getstate() == ref.random.getstate(), i
    plain_hits = hits() - h0

    many, ref = pair(t, 8002)
    many.make_shares_vec = _not_the_loop
    h0 = hits()
    for i in range(4):
        cuts = [0] + sorted(random.Random(70 + i).sample(range(1, N), 5 + 9 * i)) + [N]
        sizes = [hi - lo for lo, hi in zip(cuts, cuts[1:])]
        outs = many.make_shares_vec_many(list(torch.split(sec, sizes)), n)
        got = np.concatenate([block_limbs(o, k) for o, k in zip(outs, sizes)], axis=1)
        assert np.array_equal(got, host_shares(ref.random)), i
        assert many.random.getstate() == ref.random.getstate(), i
    assert hits() - h0 >= plain_hits, (hits() - h0, plain_hits)


# ------------------------------------------------------------ 6. fallbacks and errors
class _OwnBits(random.Random):
    """Not CPython's plain MT19937 draw for mt_compatible: getrandbits overridden."""

    def getrandbits(self, k):
        return super().getrandbits(k)


def test_many_threshold_4_runs_the_per_tensor_loop():
    sizes = [1, 0, 300, 64, 257]
    tensors = cut(secrets_int64(41, sum(sizes)), sizes)
    a, b = pair(4, 77)
    got = a.make_shares_vec_many(tensors, 6)
    assert_equal_lists(got, [b.make_shares_vec(x, 6) for x in tensors], sizes, 6)
    assert a.random.getstate() == b.random.getstate()


def test_many_with_a_generator_that_is_not_plain_mt_runs_the_loop():
    sizes = [5, 70, 0, 3]
    tensors = cut(secrets_int64(42, sum(sizes)), sizes)
    a, b = shamir.SecretShare(3), shamir.SecretShare(3)
    a.random, b.random = _OwnBits(5), _OwnBits(5)
    assert not _native.mt_compatible(a.random)
    got = a.make_shares_vec_many(tensors, 5)
    assert_equal_lists(got, [b.make_shares_vec(x, 5) for x in tensors], sizes, 5)
    assert a.random.getstate() == b.random.getstate()
    assert a.last_draw_rejected == b.last_draw_rejected


def test_many_argument_errors():
    x = [torch.arange(4, dtype=torch.int64), torch.arange(300, dtype=torch.int64)]
    with pytest.raises(ValueError, match="^threshold should be little equal than shares$"):
        shamir.SecretShare(3).make_shares_vec_many(x, 2)
    with pytest.raises(NotImplementedError, match="at most 65535 shares and threshold 64"):
        shamir.SecretShare(3).make_shares_vec_many(x, 65536)
    with pytest.raises(NotImplementedError, match="GF\\(2\\^521 - 1\\) only"):
        shamir.SecretShare(3, prime=(1 << 127) - 1).make_shares_vec_many(x, 5)
    good = [torch.empty((5, field.vec_bytes(4)), dtype=torch.uint8, device=dev()),
            torch.empty((5, field.vec_bytes(300)), dtype=torch.uint8, device=dev())]
    bad_shape = [good[0], torch.empty((5, field.vec_bytes(300) + 1), dtype=torch.uint8, device=dev())]
    bad_dtype = [good[0].to(torch.int8), good[1]]
    strided = [good[0], torch.empty((5, 2 * field.vec_bytes(300)), dtype=torch.uint8, device=dev())[:, ::2]]
    for outs, vb in ((bad_shape, field.vec_bytes(300)), (bad_dtype, field.vec_bytes(4)),
                     (strided, field.vec_bytes(300))):
        with pytest.raises(ValueError) as ei:
            shamir.SecretShare(3).make_shares_vec_many(x, 5, outs=outs)
        assert str(ei.value) == f"make_shares_vec_many: out must be contiguous uint8 [5, {vb}] on {dev()}"
    with pytest.raises(ValueError, match="make_shares_vec_many: 1 outs for 2 tensors"):
        shamir.SecretShare(3).make_shares_vec_many(x, 5, outs=good[:1])
    with pytest.raises(TypeError, match="make_shares_vec_many: values must be an int64 tensor"):
        shamir.SecretShare(3).make_shares_vec_many([torch.zeros(4)], 5)


def test_many_of_nothing():
    ss = shamir.SecretShare(3)
    ss.random.seed(1)
    before = ss.random.getstate()
    assert ss.make_shares_vec_many([], 5) == []
    outs = ss.make_shares_vec_many([torch.zeros(0, dtype=torch.int64)] * 2, 5)
    assert [tuple(o.shape) for o in outs] == [(5, 0), (5, 0)]
    assert ss.random.getstate() == before
