"""MiMC7 BN254 kernels at their field, float-conversion and shape edges.

tests/test_mimc7.py checks the kernels with three known answers and a few
hundred uniformly random inputs, and dn_mimc7_hash — the only entry point that
takes chosen field operands — runs none of the product code (mont_sqr, hash_m,
arr_step, addmod29 of csrc/mimc7_field.hpp).  Here the inputs are built to
reach what random ones do not (tests/mimc7_edges.py; test_mimc7_field_host.py
asserts that they do and rehearses the same arithmetic on the host): limb
boundaries, all-ones limbs and round sums of exactly 0 and q through the
Merkle kernel; every (limb, bit) placement, the q - a branch, the 2^53
crossing and the refusals of the device float_to_field in both kernels that
contain it; the packed Merkle kernels and their switch-over block counts
against the oracle itself; and the row pass around one 128-row block and one
256-thread workgroup.  Every reference is oracle/py_mimc7.py (Python integers)
and every comparison is bit for bit.
"""
import numpy as np
import pytest
import torch

import mimc7_edges as me
from delta_node.crypto.shamir import _native
from delta_node.utils import mimc7
from oracle import py_mimc7 as om

pytestmark = pytest.mark.gpu

Q = om.Q
SENTINEL = 0x5A5A5A5A


def dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mimc7._lib()


def to_dev_limbs(limbs: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(limbs, dtype="<u4").view(np.int32).copy()).to(dev())


def host_ints(t) -> list:
    return me.ints_of(t.cpu().numpy().view(np.uint32))


def merkle_roots(limbs: np.ndarray, blocks: int) -> list:
    """dn_mimc7_merkle_blocks on [blocks * 128, 8] leaves; one guard row behind the roots."""
    assert limbs.shape == (blocks * 128, 8)
    leaves = to_dev_limbs(limbs)
    roots = torch.full((blocks + 1, 8), SENTINEL, dtype=torch.int32, device=dev())
    _native.check(mimc7._lib().dn_mimc7_merkle_blocks(leaves.data_ptr(), blocks, roots.data_ptr(),
                                                     _native.stream_ptr()))
    out = host_ints(roots)
    assert out[blocks] == int.from_bytes(SENTINEL.to_bytes(4, "little") * 8, "little"), "a root beyond the last block"
    return out[:blocks]


def weight_chain(w, precision: int):
    """dn_mimc7_weight_chain through the C-ABI: (return code, field value, bad_count)."""
    wd = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64).copy()).to(dev())
    out = torch.full((8,), SENTINEL, dtype=torch.int32, device=dev())
    bad = torch.zeros(1, dtype=torch.int32, device=dev())
    rc = mimc7._lib().dn_mimc7_weight_chain(wd.data_ptr(), wd.numel(), precision, out.data_ptr(), bad.data_ptr(),
                                           _native.stream_ptr())
    return rc, host_ints(out.reshape(1, 8))[0], int(bad.item())


# ------------------------------------------------------------------ field operands
def test_hash_kernel_pool_squared():
    """dn_mimc7_hash (hash_kernel: four mont_mul per round) over pool x pool,
    the unreduced r + key as the API returns it."""
    pool = me.field_pool()
    xs = [a for a in pool for _ in pool]
    ks = [b for _ in pool for b in pool]
    got = mimc7.mimc7_hash(xs, ks)
    want = [me.expected_hash(x, k) for x, k in zip(xs, ks)]
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (f"{len(bad)} of {len(xs)} differ, first x={xs[bad[0]]:#x} key={ks[bad[0]]:#x}: "
                     f"got {got[bad[0]]:#x}, want {want[bad[0]]:#x}")


def test_merkle_kernel_pool_pairs():
    """hash_m / mont_sqr / arr_step / addmod29 on chosen operands: every level-0
    node of the Merkle kernel is one pair (a, b), a over the pool, b over 16
    fixed picks; the last block is zero-padded.  Each root against the oracle."""
    pool, partners = me.field_pool(), me.merkle_partners()
    leaves = [v for a in pool for b in partners for v in (a, b)]
    blocks = -(-len(leaves) // 128)
    leaves += [0] * (blocks * 128 - len(leaves))
    got = merkle_roots(me.limbs_of(leaves), blocks)
    for b in range(blocks):
        block = leaves[128 * b:128 * (b + 1)]
        assert got[b] == me.expected_merkle(block), f"block {b}, leaves {[hex(v) for v in block]}"


@pytest.mark.parametrize("blocks", [1, 2, 2047, 2048, 2049, 8191, 8192, 8192 + 15])
def test_packed_merkle_blocks_vs_oracle(blocks):
    """merkle_kernel<1>, <4> (from 2048 blocks) and <16> (from 8192) against
    the oracle itself, at the switch-over counts, one below and above, and a
    partial last workgroup: blocks at the start, around workgroup boundaries,
    in the middle and the last 17."""
    rng = np.random.default_rng(1000 + blocks)
    limbs = rng.integers(0, 1 << 32, size=(blocks * 128, 8), dtype=np.uint32)
    limbs[:, 7] = rng.integers(0, Q >> 224, size=blocks * 128, dtype=np.uint32)  # top limb below q's: value < q
    got = merkle_roots(limbs, blocks)
    last = blocks - 1
    picks = sorted(b for b in {0, 1, 3, 4, 15, 16, 17, blocks // 2, *range(last - 16, last + 1)} if 0 <= b < blocks)
    for b in picks:
        block = me.ints_of(limbs[128 * b:128 * (b + 1)])
        assert max(block) < Q
        assert got[b] == me.expected_merkle(block), f"block {b} of {blocks}"


# ------------------------------------------------------------------ float_to_field
def assert_rows(data: np.ndarray, what: str):
    n = data.shape[0]
    got = host_ints(mimc7.data_row_hashes(data))
    want = me.expected_row_hashes(data.tolist())
    assert len(got) == len(want) == -(-n // 128) * 128
    for i, (g, w) in enumerate(zip(got, want)):
        row = [f"{float(x)!r} = {float(x).hex()}" for x in data[i]] if i < n else "padding"
        assert g == w, f"{what}: row {i} {row}: got {g:#x}, want {w:#x}"


def test_float_to_field_row_pass_features():
    """Scale 10^8: one row [v, 0.0] per pool value."""
    pool = me.float_pool(1e8)
    data = np.array([[v, 0.0] for v in pool], dtype=np.float64)
    assert_rows(data, "feature column")


def test_float_to_field_row_pass_label():
    """Scale 10^21: data of shape (n, 1) — the only column is the label."""
    pool = me.float_pool(1e21)
    data = np.array(pool, dtype=np.float64).reshape(-1, 1)
    assert_rows(data, "label column")


def test_float_to_field_chain_precision_8():
    """chain_kernel through weight_commitment_device: the pool as one chain,
    and as consecutive chunks of 257 so that a failure is localised."""
    pool = me.float_pool(1e8)
    for lo in range(0, len(pool), 257):
        part = pool[lo:lo + 257]
        assert mimc7.weight_commitment_device(part) == om.weight_commitment(part), f"weights {lo}..{lo + len(part) - 1}"
    assert mimc7.weight_commitment_device(pool) == om.weight_commitment(pool)


@pytest.mark.parametrize("precision", [0, 21, 22])
def test_weight_chain_other_precisions(precision):
    """dn_mimc7_weight_chain's precision argument (the wrapper only passes 8):
    the pool rebuilt for that scale."""
    pool = me.float_pool(float(10 ** precision))
    rc, got, bad = weight_chain(pool, precision)
    assert rc == _native.DN_OK and bad == 0
    assert got == me.expected_hash_arr([om.float2int(w, precision) for w in pool])
    good = me.good_neighbour(float(10 ** precision))
    rc, got, bad = weight_chain([good, -good], precision)
    assert rc == _native.DN_OK and bad == 0
    assert got == me.expected_hash_arr([om.float2int(good, precision), om.float2int(-good, precision)])


@pytest.mark.parametrize("precision", [-1, 23])
def test_weight_chain_precision_out_of_range(precision):
    rc, got, bad = weight_chain([1.0, 2.0], precision)
    assert rc == _native.DN_ERR_ARG and bad == 0
    assert got == int.from_bytes(SENTINEL.to_bytes(4, "little") * 8, "little"), "nothing may be written"
    with pytest.raises(ValueError, match="precision 0..22"):
        _native.check(rc)


# ------------------------------------------------------------------ refusal path
ROWS_REFUSE = 300  # padded to 384: row 299 is the last real one, rows >= 256 are the second workgroup


@pytest.fixture(scope="module")
def good_data():
    rng = np.random.default_rng(77)
    data = rng.standard_normal((ROWS_REFUSE, 2)) * 10
    data[:, -1] = rng.integers(0, 2, ROWS_REFUSE)
    return data, om.data_commitment(data.tolist())


def test_refused_values_raise_everywhere(good_data):
    """NaN, +-inf, an overflowing product and +-(the smallest v with
    |v 10^p| >= 2^253): NotImplementedError from row 0, the last real row and
    a row of the second workgroup, in the feature and the label column, and
    from the first and last position of a device chain.  The double just below
    is accepted and exact; so is the next good call on the same stream."""
    data, want = good_data
    for col, scale in ((0, 1e8), (1, 1e21)):
        for v in me.bad_floats(scale):
            for row in (0, ROWS_REFUSE - 1, 257):
                d = data.copy()
                d[row, col] = v
                with pytest.raises(NotImplementedError, match="2\\^253"):
                    mimc7.calc_data_commitment(d)
    assert mimc7.calc_data_commitment(data) == want
    for v in me.bad_floats(1e8):
        for w in ([v, 1.0, -2.5, 3.0], [1.0, -2.5, 3.0, v]):
            with pytest.raises(NotImplementedError, match="2\\^253"):
                mimc7.weight_commitment_device(w)
    w = [1.0, -2.5, 3.0]
    assert mimc7.weight_commitment_device(w) == om.weight_commitment(w)
    # the neighbours just inside the range, at every such place at once
    d = data.copy()
    for col, scale in ((0, 1e8), (1, 1e21)):
        g = me.good_neighbour(scale)
        d[0, col], d[ROWS_REFUSE - 1, col], d[257, col] = g, -g, g
    assert mimc7.calc_data_commitment(d) == om.data_commitment(d.tolist())
    g = me.good_neighbour(1e8)
    assert mimc7.weight_commitment_device([g, 1.0, -g]) == om.weight_commitment([g, 1.0, -g])


def test_bad_count_counts_rows(good_data):
    """*bad_count of dn_mimc7_data_rows is the number of ROWS holding at least
    one refused value (include/dn_mimc7.h); the chain adds one, once."""
    rng = np.random.default_rng(78)
    data = rng.standard_normal((ROWS_REFUSE, 3))
    f, lab = me.bad_floats(1e8), me.bad_floats(1e21)
    data[0, 0] = f[0]                                         # one value
    data[5, 1], data[5, 2] = f[4], lab[5]                     # two in one row
    data[256, 0], data[256, 1], data[256, 2] = f[1], f[2], lab[3]  # three in one row
    data[ROWS_REFUSE - 1, 2] = lab[4]                         # the last real row, label only
    arr = torch.from_numpy(data).to(dev())
    out = torch.empty((384, 8), dtype=torch.int32, device=dev())
    bad = torch.zeros(1, dtype=torch.int32, device=dev())
    _native.check(mimc7._lib().dn_mimc7_data_rows(arr.data_ptr(), ROWS_REFUSE, 3, out.data_ptr(), bad.data_ptr(),
                                                 _native.stream_ptr()))
    assert int(bad.item()) == 4
    rc, _, nbad = weight_chain([f[0], 1.0, f[4], f[5], 2.0, f[1]], 8)
    assert rc == _native.DN_OK and nbad == 1
    good, want = good_data
    assert mimc7.calc_data_commitment(good) == want  # a following good call is exact


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("cols", [1, 2, 7])
@pytest.mark.parametrize("rows", [1, 127, 128, 129, 255, 256, 257, 385])
def test_data_commitment_shapes(rows, cols):
    """Around one 128-row block and one 256-thread workgroup; cols == 1 makes
    the only column the label (10^21)."""
    rng = np.random.default_rng(1000 * rows + cols)
    data = rng.standard_normal((rows, cols)) * np.array(([1.0, 1e5, 1e-7] * 3)[:cols])
    data[:, -1] = rng.integers(-1, 3, rows) if cols > 1 else rng.standard_normal(rows) * 3
    got = mimc7.calc_data_commitment(data)
    assert len(got) == -(-rows // 128)
    assert got == om.data_commitment(data.tolist())


def test_data_commitment_float32_and_strided_input():
    rng = np.random.default_rng(9)
    d32 = torch.from_numpy(rng.standard_normal((300, 3)).astype(np.float32)).to(dev())
    assert mimc7.calc_data_commitment(d32) == om.data_commitment(d32.cpu().to(torch.float64).numpy().tolist())
    wide = torch.from_numpy(rng.standard_normal((300, 6))).to(dev())
    view = wide[:, 1:4]  # a column slice: row stride 6, storage offset 1
    assert not view.is_contiguous()
    assert mimc7.calc_data_commitment(view) == om.data_commitment(view.cpu().contiguous().numpy().tolist())
    w32 = wide.to(torch.float32)[:, 2:5]
    assert not w32.is_contiguous()
    assert mimc7.calc_data_commitment(w32) == om.data_commitment(w32.cpu().to(torch.float64).contiguous().numpy().tolist())
