"""resolve_shares_vec_many (MI355X): one reconstruct launch over a list of tensors.

Every tensor's shares lie in that tensor's own tiled block (as
make_shares_vec_many leaves them), so the many-call must equal the per-tensor
resolve_shares_vec loop bit for bit — values, tiled field outputs and
per-tensor overflow counts — for every kernel form the single-vector path
reaches.  Checked here against that loop, against the reference's own golden
outputs and digests, as a round trip of make_shares_vec_many, for reads and
writes outside the blocks, and for calls issued back to back without a host
synchronisation.  Integer field arithmetic: every comparison is bit-exact.
"""
import importlib.util
import os
import random
import sys
import threading

import numpy as np
import pytest
import torch

from delta_node.crypto import shamir
from delta_node.crypto.shamir import _native, field
from golden.fixtures import chunk_digests, combine_digests, load_npz, manifest, secrets_int64

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
shamir_mod = sys.modules["delta_node.crypto.shamir.shamir"]

# an empty tensor, one-element tensors, sizes just below, at and above a tile,
# whole multi-tile tensors: the load-ahead path and the guarded last tile
# within one launch (10837 elements, 53 tiles: 14 workgroups)
RAGGED = [1, 63, 64, 65, 0, 127, 128, 255, 256, 257, 1, 1, 300, 512, 1000, 4097, 2500]
KMAX = 17  # share rows drawn per tensor (test 6's k = 17)

# xs -> the descriptor dn_m521_lagrange gives (a_limbs, has_inv, shift): every
# kernel form of the single-vector path — the unrolled K = 2..5 (one-limb
# weights), the runtime-K kernel (k = 7, 16, and every two-limb / full-width
# set), and each (a_limbs, has_inv) pair the host can produce: full-width
# weights are lambda_i mod p themselves and carry no divisor, so (17, 1) and
# (17, 2) do not occur.
B33 = 1 << 33
FORMS = [
    ([1, 3], (1, 0, 1)), ([1, 4], (1, 2, 0)), ([1040758, 758791], (1, 1, 0)),
    ([B33, B33 + 1], (2, 0, 0)), ([B33, B33 + 3], (2, 2, 0)),
    ([1, 3, 5], (1, 0, 3)), ([2, 4, 5], (1, 2, 0)), ([98, 19, 222], (1, 1, 1)),
    ([1 << 20, (1 << 20) + 1, (1 << 20) + 2], (2, 0, 0)), ([35016, 60626, 7492], (2, 1, 0)),
    ([88159051, 658814259, 702745590], (17, 0, 0)),
    ([1, 2, 3, 4], (1, 0, 0)), ([1, 2, 3, 6], (1, 2, 1)), ([217, 19, 197, 46], (1, 1, 2)),
    ([1, 3, 5, 7, 9], (1, 0, 7)), ([1, 2, 3, 4, 6], (1, 2, 0)), ([162, 232, 144, 246, 154], (1, 1, 0)),
    ([1, 2, 3, 4, 5, 6, 7], (1, 0, 0)), ([1, 2, 3, 4, 5, 6, 8], (1, 2, 0)),
    ([136, 9, 74, 114, 243, 52, 54], (2, 1, 0)), ([196, 228, 135, 45, 210, 22, 59], (17, 0, 0)),
    ([128, 224, 164, 228, 136, 238, 174, 177, 179, 147, 115, 151, 24, 88, 157, 159], (17, 0, 0)),
]


def dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _native.lib()


def random_rows(seed: int, n: int, k: int) -> torch.Tensor:
    """k tiled vectors of n random field elements in [1, p - 1] (inconsistent
    shares; almost all >= 2^64), as a device block [k, vec_bytes(n)]."""
    ys = _native.mt_draw_coeffs(random.Random(seed), n, k)
    return torch.from_numpy(np.ascontiguousarray(ys).reshape(k, field.vec_bytes(n))).to(dev())


@pytest.fixture(scope="module")
def ragged_blocks():
    """One block of KMAX random share rows per tensor of RAGGED (never written)."""
    return [random_rows(1000 + j, n, KMAX) for j, n in enumerate(RAGGED)]


def rows_of(blocks, k):
    return [[b[i] for i in range(k)] for b in blocks]


def the_loop(ss, shares, xs, ns, out):
    """The per-tensor calls the many-call stands for: (results, per-tensor counts)."""
    res, cnt = [], []
    for sh, n in zip(shares, ns):
        r, c = ss.resolve_shares_vec(sh, xs, n, out=out, return_overflow=True)
        res.append(r)
        cnt.append(int(c.item()))
    return res, cnt


def _not_the_loop(*args, **kwargs):
    raise AssertionError("resolve_shares_vec_many fell back to the per-tensor loop")


def fused(monkeypatch, ss, *args, **kwargs):
    """ss.resolve_shares_vec_many(...) with the per-tensor path made an error."""
    with monkeypatch.context() as m:
        m.setattr(shamir_mod, "_resolve_vectors", _not_the_loop)
        return ss.resolve_shares_vec_many(*args, **kwargs)


def live_mask(n: int) -> np.ndarray:
    """bool [vec_bytes(n)]: the bytes of a tiled vector that belong to its n elements."""
    nt = (n + 255) // 256
    m = np.zeros((nt, 66 * 256), dtype=bool)
    live = (np.arange(nt * 256) < n).reshape(nt, 256)
    m[:, :16 * 1024].reshape(nt, 16, 256, 4)[:] = live[:, None, :, None]
    m[:, 16 * 1024:].reshape(nt, 256, 2)[:] = live[:, :, None]
    return m.reshape(-1)


def assert_same(got, want, ns, out):
    assert len(got) == len(want) == len(ns)
    for j, (g, w, n) in enumerate(zip(got, want, ns)):
        assert g.is_cuda and g.is_contiguous() and g.dtype == w.dtype and g.shape == w.shape, j
        if out == "int64":
            assert torch.equal(g, w), (j, n)
        else:  # the n real elements; padding lanes of a last tile are unspecified
            m = torch.from_numpy(live_mask(n)).to(g.device)
            assert torch.equal(g[m], w[m]), (j, n)


# ------------------------------------------------------------ 1. equals the per-tensor loop
@pytest.mark.parametrize("xs,form", FORMS, ids=["k%d-a%d-inv%d-sh%d" % ((len(x),) + f) for x, f in FORMS])
def test_many_equals_the_per_tensor_loop(xs, form, ragged_blocks, monkeypatch):
    k = len(xs)
    w = _native.lagrange(xs, 2)
    assert (w.k, w.a_limbs, w.has_inv, w.shift) == (k,) + form  # the coverage is stated, not assumed
    ss = shamir.SecretShare(2)
    shares = rows_of(ragged_blocks, k)
    for out in ("int64", "field"):
        want, want_cnt = the_loop(ss, shares, xs, RAGGED, out)
        got, over = fused(monkeypatch, ss, shares, xs, RAGGED, out=out, return_overflow=True)
        assert_same(got, want, RAGGED, out)
        assert over.dtype == torch.int32 and tuple(over.shape) == (len(RAGGED),) and over.is_cuda
        assert over.tolist() == want_cnt
        # random field elements: the counts are non-zero and differ per tensor
        assert want_cnt[4] == 0 and min(c for c, n in zip(want_cnt, RAGGED) if n > 1) > 0
        assert len(set(want_cnt)) > 8
        plain = fused(monkeypatch, ss, shares, xs, RAGGED, out=out)
        assert_same(plain, want, RAGGED, out)


def test_default_outs_are_consecutive_views_of_one_allocation(ragged_blocks):
    ss = shamir.SecretShare(3)
    for out, step in (("int64", 8), ("field", 1)):
        got = ss.resolve_shares_vec_many(rows_of(ragged_blocks, 3), [1, 3, 5], RAGGED, out=out)
        ptr = got[0].data_ptr()
        for g, n in zip(got, RAGGED):
            size = n if out == "int64" else field.vec_bytes(n)
            assert tuple(g.shape) == (size,)
            if n:  # (an empty view has no address)
                assert g.data_ptr() == ptr
                ptr += step * size


# ------------------------------------------------------------ 2. reference pins
@pytest.mark.parametrize("key,sizes", [("f1", [1, 200, 63, 500, 260]), ("f2", [100, 1, 155])])
def test_reference_shares_cut_into_tensors(key, sizes, monkeypatch):
    """The reference's own shares, cut and re-tiled per tensor: every golden
    subset reconstructs the reference's secrets, nothing overflows."""
    cfg = manifest()[key]
    z = load_npz(cfg["file"])
    assert sum(sizes) == cfg["N"]
    cuts = np.cumsum([0] + sizes)
    blocks = [torch.from_numpy(np.stack([field.limbs_to_vec(z["share_limbs"][a:b, s, :]) for s in range(cfg["n"])]))
              .to(dev()) for a, b in zip(cuts[:-1], cuts[1:])]
    sec = torch.from_numpy(z["secrets"]).to(dev())
    ss = shamir.SecretShare(cfg["t"])
    for sub, size in zip(z["recon_subsets"], z["recon_sizes"]):
        xs = [int(x) for x in sub[:size]]
        shares = [[b[x - 1] for x in xs] for b in blocks]
        got, over = fused(monkeypatch, ss, shares, xs, sizes, return_overflow=True)
        assert torch.equal(torch.cat(got), sec), xs
        assert over.tolist() == [0] * len(sizes), xs


@pytest.mark.parametrize("name", ["recon_13579_2e16", "recon_245_2e18"])
def test_reference_digest_cut_at_random_points(name, monkeypatch):
    """The reference's resolve_shares digest over random field elements, the
    inputs cut at 23 seeded points and re-tiled per tensor."""
    d = [d for d in manifest()["digests"] if d["name"] == name][0]
    N, xs = d["N"], d["xs"]
    k = len(xs)
    ys = np.ascontiguousarray(_native.mt_draw_coeffs(random.Random(d["mt_seed"]), N, k)).reshape(k, -1)
    planes = np.stack([field.vec_to_planes(ys[s], N) for s in range(k)])  # [k, 17, N]
    assert combine_digests(chunk_digests(planes)) == d["input_digest"], name
    limbs = np.ascontiguousarray(planes.transpose(0, 2, 1))  # [k, N, 17]
    del planes, ys
    cuts = [0] + sorted(random.Random(len(name)).sample(range(1, N), 23)) + [N]
    sizes = [b - a for a, b in zip(cuts[:-1], cuts[1:])]
    blocks = [torch.from_numpy(np.stack([field.limbs_to_vec(limbs[s, a:b]) for s in range(k)])).to(dev())
              for a, b in zip(cuts[:-1], cuts[1:])]
    got = fused(monkeypatch, shamir.SecretShare(k), blocks, xs, sizes, out="field")
    out = np.empty((1, 17, N), dtype=np.uint32)
    for g, a, b in zip(got, cuts[:-1], cuts[1:]):
        out[0, :, a:b] = field.vec_to_planes(g.cpu().numpy(), b - a)
    assert combine_digests(chunk_digests(out)) == d["digest"], name


# ------------------------------------------------------------ 3. round trip
@pytest.mark.parametrize("t,n,xs", [(3, 5, [1, 3, 5]), (3, 5, [2, 4, 5]), (5, 9, [2, 3, 5, 8, 9])],
                         ids=["3of5-135", "3of5-245", "5of9"])
def test_round_trip_of_make_shares_vec_many(t, n, xs, monkeypatch):
    sec = torch.from_numpy(secrets_int64(7 * t + n, sum(RAGGED))).to(dev())
    tensors = list(torch.split(sec, RAGGED))
    ss = shamir.SecretShare(t)
    ss.random.seed(31 + t)
    blocks = ss.make_shares_vec_many(tensors, n)
    got, over = fused(monkeypatch, ss, [[b[x - 1] for x in xs] for b in blocks], xs, RAGGED, return_overflow=True)
    assert over.tolist() == [0] * len(RAGGED)
    for g, x in zip(got, tensors):
        assert torch.equal(g, x)
    # the 2-D form: the first t rows of each block as a view, and a gathered [k, vb] tensor
    first = list(range(1, t + 1))
    got = fused(monkeypatch, ss, [b[:t] for b in blocks], first, RAGGED)
    assert torch.equal(torch.cat(got), sec)
    got = fused(monkeypatch, ss, [torch.stack([b[x - 1] for x in xs]) for b in blocks], xs, RAGGED)
    assert torch.equal(torch.cat(got), sec)


# ------------------------------------------------------------ 4. nothing outside the outputs
@pytest.mark.parametrize("out", ["int64", "field"])
def test_writes_nothing_outside_its_outputs_and_leaves_the_shares(out, ragged_blocks, monkeypatch):
    guard, xs = 4096, [1, 3, 5]
    sizes = [8 * n if out == "int64" else field.vec_bytes(n) for n in RAGGED]
    buf = torch.full((guard + sum(s + guard for s in sizes),), 0xA5, dtype=torch.uint8, device=dev())
    outs, spans, off = [], [], guard
    for s in sizes:
        o = buf[off:off + s]
        outs.append(o.view(torch.int64) if out == "int64" else o)
        spans.append((off, off + s))
        off += s + guard
    before = [b.clone() for b in ragged_blocks]
    ss = shamir.SecretShare(3)
    shares = rows_of(ragged_blocks, 3)
    got = fused(monkeypatch, ss, shares, xs, RAGGED, out=out, outs=outs)
    assert all(g is o for g, o in zip(got, outs))
    want, _ = the_loop(ss, shares, xs, RAGGED, out)
    assert_same(got, want, RAGGED, out)
    host = buf.cpu().numpy().copy()
    for (a, b), n in zip(spans, RAGGED):  # blank what the call may write: the rest must be the fill
        if out == "int64":
            host[a:b] = 0xA5
        else:
            host[a:b][live_mask(n)] = 0xA5  # (lanes past n_k of a last tile are not written either)
    assert np.all(host == 0xA5)
    for b0, b1 in zip(before, ragged_blocks):
        assert torch.equal(b0, b1)


# ------------------------------------------------------------ 5. no sync, no shared staging
def test_back_to_back_calls_and_two_threads(ragged_blocks, monkeypatch):
    """Two many-calls with different lists and abscissas issued with no host
    synchronisation in between (the second call's table must not overwrite the
    first one's before its copy has run), then the same pair from two threads
    on two streams."""
    ss = shamir.SecretShare(2)
    sizes_b = [300, 1, 257, 64, 4097]
    blocks_b = [random_rows(2000 + j, n, 4) for j, n in enumerate(sizes_b)]
    calls = [(rows_of(ragged_blocks, 3), [1, 3, 5], RAGGED), (rows_of(blocks_b, 4), [1, 2, 3, 6], sizes_b)]
    want = [the_loop(ss, *c, "int64") for c in calls]
    torch.cuda.synchronize()
    monkeypatch.setattr(shamir_mod, "_resolve_vectors", _not_the_loop)

    got = [ss.resolve_shares_vec_many(*c, return_overflow=True) for c in calls]  # back to back, one stream
    for (g, over), (w, cnt), c in zip(got, want, calls):
        assert_same(g, w, c[2], "int64")
        assert over.tolist() == cnt

    res, errs = [None, None], []

    def work(i):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                for _ in range(3):
                    res[i] = shamir.SecretShare(2).resolve_shares_vec_many(*calls[i], return_overflow=True)
        except Exception as e:  # noqa: BLE001 (reported by the asserting thread)
            errs.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errs, errs
    torch.cuda.synchronize()
    for (g, over), (w, cnt), c in zip(res, want, calls):
        assert_same(g, w, c[2], "int64")
        assert over.tolist() == cnt


# ------------------------------------------------------------ 6. fallbacks and errors
@pytest.mark.parametrize("xs", [list(range(1, 18)), [1, 2, 1 << 70]], ids=["k17", "x-beyond-64-bits"])
def test_the_grouped_path_runs_the_loop(xs, ragged_blocks, monkeypatch):
    k = len(xs)
    ss = shamir.SecretShare(3)
    shares = rows_of(ragged_blocks, k)
    for out in ("int64", "field"):
        want, want_cnt = the_loop(ss, shares, xs, RAGGED, out)
        calls, real = [], shamir_mod._resolve_vectors
        with monkeypatch.context() as m:
            m.setattr(shamir_mod, "_resolve_vectors", lambda *a, **kw: (calls.append(a[2]), real(*a, **kw))[1])
            m.setattr(_native, "reconstruct_many", _not_the_loop)
            got, over = ss.resolve_shares_vec_many(shares, xs, RAGGED, out=out, return_overflow=True)
        assert calls == RAGGED  # the per-tensor loop ran, tensor by tensor
        assert_same(got, want, RAGGED, out)
        assert over.tolist() == want_cnt


def test_argument_errors(ragged_blocks):
    ss = shamir.SecretShare(3)
    xs, ns = [1, 3, 5], RAGGED[:3]
    shares = rows_of(ragged_blocks[:3], 3)
    many = ss.resolve_shares_vec_many
    with pytest.raises(ValueError, match="resolve_shares_vec_many: 3 share entries for 2 tensors"):
        many(shares, xs, ns[:2])
    with pytest.raises(ValueError, match="resolve_shares_vec_many: 2 outs for 3 tensors"):
        many(shares, xs, ns, outs=[torch.empty(n, dtype=torch.int64, device=dev()) for n in ns[:2]])
    good = [torch.empty(n, dtype=torch.int64, device=dev()) for n in ns]
    for j, bad in [(1, torch.empty(ns[1] + 1, dtype=torch.int64, device=dev())),             # shape
                   (1, torch.empty(ns[1], dtype=torch.int32, device=dev())),                  # dtype
                   (2, torch.empty(2 * ns[2], dtype=torch.int64, device=dev())[::2]),         # stride
                   (0, torch.empty(ns[0], dtype=torch.int64))]:                               # device
        outs = list(good)
        outs[j] = bad
        with pytest.raises(ValueError, match="resolve_shares_vec_many: out must be contiguous int64"):
            many(shares, xs, ns, outs=outs)
    with pytest.raises(ValueError, match="resolve_shares_vec_many: out must be contiguous field"):
        many(shares, xs, ns, out="field", outs=good)
    with pytest.raises(ValueError, match="resolve_shares_vec_many: share vectors must be contiguous uint8"):
        many(shares, xs, [ns[0], ns[1], 257])  # rows of one tile for a two-tile tensor
    with pytest.raises(ValueError, match="resolve_shares_vec_many: share rows must be contiguous uint8"):
        many([b[:3, ::2] if j == 1 else b[:3] for j, b in enumerate(ragged_blocks[:3])], xs, ns)
    with pytest.raises(ValueError, match="resolve_shares_vec_many: share vectors must be contiguous uint8"):
        many([[v.cpu() for v in sh] for sh in shares], xs, ns)


def test_empty_calls():
    ss = shamir.SecretShare(3)
    xs = [1, 3, 5]
    assert ss.resolve_shares_vec_many([], xs, []) == []
    got, over = ss.resolve_shares_vec_many([], xs, [], return_overflow=True)
    assert got == [] and tuple(over.shape) == (0,) and over.dtype == torch.int32
    empty = [torch.empty(0, dtype=torch.uint8, device=dev()) for _ in xs]
    for out, dt in (("int64", torch.int64), ("field", torch.uint8)):
        got, over = ss.resolve_shares_vec_many([empty, torch.empty((3, 0), dtype=torch.uint8, device=dev())], xs, [0, 0],
                                               out=out, return_overflow=True)
        assert [tuple(g.shape) for g in got] == [(0,), (0,)] and all(g.dtype == dt and g.is_cuda for g in got)
        assert over.tolist() == [0, 0]


# ------------------------------------------------------------ 7. the model-sized mix
@pytest.mark.slow
def test_round_trip_of_the_127_tensor_mix(monkeypatch):
    """make_shares_vec_many -> resolve_shares_vec_many over the ragged 127-tensor
    mix of 2^24 elements (scripts/measure_many.py), compared on the device."""
    spec = importlib.util.spec_from_file_location("measure_many", os.path.join(ROOT, "scripts", "measure_many.py"))
    mm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mm)
    sizes = mm.mix_sizes(True)
    sec = torch.from_numpy(secrets_int64(5, sum(sizes))).to(dev())
    ss = shamir.SecretShare(3)
    ss.random.seed(77)
    blocks = ss.make_shares_vec_many(list(torch.split(sec, sizes)), 5)
    xs = [1, 3, 5]
    got, over = fused(monkeypatch, ss, [[b[x - 1] for x in xs] for b in blocks], xs, sizes, return_overflow=True)
    assert torch.equal(torch.cat(got), sec)
    assert int(over.sum().item()) == 0
