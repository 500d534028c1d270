"""GF(2^521 - 1) kernels at their carry, bound and canonical-form edges.

The rest of the suite feeds the kernels uniformly random field elements, for
which the rare branches of csrc/m521_device.hpp (the carry ripple of
reduce(), canon(), the wave-uniform slow path of the stores, the borrow chain
of exact_div_small(), rotr521()'s two arms, the 2^544 bound of the lazy
form) are close to unreachable.  Here the inputs are built to reach them
(tests/field_edges.py; test_field_edges_host.py asserts that they do), the
reference is Python integers and every comparison is exact, over every
output element unless a test states a subset.
"""
import random

import numpy as np
import pytest
import torch

import field_edges as fe
from delta_node.crypto import shamir
from delta_node.crypto.shamir import _native, field
from field_edges import M64, N_LAYOUT, P

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _native.lib()


def to_vec(vals):
    return torch.from_numpy(field.ints_to_vec(vals)).to(dev())


def to_block(rows):
    return torch.from_numpy(np.stack([field.ints_to_vec(r) for r in rows])).to(dev())


def to_i64(vals):
    return torch.tensor([fe.to_i64(v) for v in vals], dtype=torch.int64)


def assert_vec_equals(vec_host: np.ndarray, want, what):
    """A downloaded tiled vector against Python integers, limb for limb."""
    n = len(want)
    got = field.vec_to_limbs(vec_host, n)
    exp = field.ints_to_limbs(want)
    if not np.array_equal(got, exp):
        bad = np.nonzero((got != exp).any(axis=1))[0]
        i = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {n} elements differ, first at element {i} (tile {i // 256}, "
                             f"lane {i % 256}): got {field.limbs_to_ints(got[i:i + 1])[0]:#x}, "
                             f"want {want[i]:#x}")


def check_shares(out, case, rows=None):
    h = out.cpu().numpy()
    for x in (rows if rows is not None else range(1, case.n + 1)):
        assert_vec_equals(h[x - 1], case.expected(x), f"t={case.t} n={case.n} share {x}")


def run_split(case, out=None):
    t, n, N = case.t, case.n, case.N
    if out is None:
        out = torch.full((n, field.vec_bytes(N)), 0xA5, dtype=torch.uint8, device=dev())
    co = to_block([case.coeffs(j) for j in range(1, t)]) if t > 1 else None
    if case.fe:
        _native.split_fe(to_vec(case.secrets()), co, out, N, t, n)
    else:
        _native.split_u64(to_i64(case.secrets()).to(dev()), co, out, N, t, n)
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------ a. split, explicit coefficients, edge layout
@pytest.mark.parametrize("t,n", fe.SPLIT_U64_SHAPES)
def test_split_u64_on_edge_layout(t, n):
    """split_kernel<T, false, false> for T = 1..4, 6, 7 (n = T and T + 4), the
    product default of t = 5 (split_wide_kernel<5, 2>: four full tiles and the
    partial one), the folding Horner kernels ((4, 300), (8, 8)) and
    split_kernel_generic (t = 9, 20)."""
    case = fe.split_case(t, n)
    check_shares(run_split(case), case)


@pytest.mark.parametrize("t,n,knob,value", [(5, 9, "DN_SPLIT_E", "0"), (3, 5, "DN_SPLIT_E", "2"),
                                            (3, 5, "DN_SPLIT_E", "4"), (2, 3, "DN_SPLIT_HORNER", "1"),
                                            (3, 5, "DN_SPLIT_HORNER", "1"), (5, 9, "DN_SPLIT_HORNER", "1")])
def test_split_u64_kernel_variants_on_edge_layout(t, n, knob, value, monkeypatch):
    """The kernels only the tuning library's knobs select: the one-element
    split_kernel<5> (DN_SPLIT_E=0), split_wide_kernel<3, 2> and <3, 4>, and
    the Horner form of T = 2, 3, 5."""
    case = fe.split_case(t, n)
    monkeypatch.setenv(knob, value)
    with _native.library(_native.TUNING_LIB):
        out = run_split(case)
    check_shares(out, case)


@pytest.mark.parametrize("t,n", fe.SPLIT_FE_SHAPES)
def test_split_fe_on_edge_layout(t, n):
    """FE_SECRET kernels: secrets from the pool, p itself included."""
    case = fe.split_case(t, n, fe=True)
    check_shares(run_split(case), case)


def test_make_shares_vec_explicit_coeffs_on_edge_layout():
    case = fe.split_case(3, 5)
    co = to_block([case.coeffs(1), case.coeffs(2)])
    out = shamir.SecretShare(3).make_shares_vec(to_i64(case.secrets()), 5, coeffs=co)
    torch.cuda.synchronize()
    check_shares(out, case)


# ------------------------------------------------------------ b. the forward-difference bound
class _ConstCase:
    """Every coefficient and the secret the same value: expected per share only."""

    def __init__(self, t, n, N, v, fe_secret=True):
        self.t, self.n, self.N, self.fe, self.v = t, n, N, fe_secret, v
        self.sec = v if fe_secret else M64  # (an int64 secret: all 64 bits set)

    def secrets(self):
        return [self.sec] * self.N

    def coeffs(self, j):
        return [self.v] * self.N

    def expected(self, x):
        return [fe.split_expected([self.sec] + [self.v] * (self.t - 1), x)] * self.N


@pytest.mark.parametrize("inputs", ["p-1", "p", "pool"])
@pytest.mark.parametrize("over", [0, 1])
@pytest.mark.parametrize("t", [3, 4, 5, 6, 7])
def test_split_at_the_forward_difference_bound(t, over, inputs):
    """The largest n whose difference table stays below 2^544 (derived from
    the restated fd_needs_fold: 2892, 198, 48, 18, 7 for t = 3..7) and n + 1,
    the first shape that folds; N = 300 is one full tile and a partial one.
    With every coefficient p - 1 the table of t = 3, 4, 5 needs all 544 bits
    (test_field_edges_host.py)."""
    n = fe.fd_max_n(t) + over
    assert fe.fd_needs_fold(t, n) == bool(over)
    if inputs == "pool":
        case = fe.SplitCase(t, n, 300)
    else:
        case = _ConstCase(t, n, 300, P - 1 if inputs == "p-1" else P)
    check_shares(run_split(case), case)


@pytest.mark.parametrize("secret", ["field", "int64"])
@pytest.mark.parametrize("value", ["p-1", "p"])
@pytest.mark.parametrize("t", [3, 4, 5, 6, 7])
def test_split_where_an_unfolded_table_would_overflow(t, value, secret):
    """A few share counts past the bound (2896, 203, 54 for t = 3, 4, 5) the
    last share itself, unreduced, no longer fits 17 limbs when every
    coefficient is p - 1: the shape must take the folding kernel.  (At n + 1 of
    the bound test above an unfolded table still happens to fit, so a bound
    that is too generous would pass there.)  Field secrets run the FE_SECRET
    kernels, int64 secrets the product's (the wide one for t = 5)."""
    n = fe.fd_overflow_n(t)
    assert fe.fd_needs_fold(t, n)
    case = _ConstCase(t, n, 300, P - 1 if value == "p-1" else P, fe_secret=secret == "field")
    check_shares(run_split(case), case)


@pytest.mark.parametrize("inputs", ["p-1", "p", "pool"])
def test_split_t2_at_the_share_limit(inputs):
    """t = 2, n = 65535 (the table never folds), N = 40.  Compared: shares
    1..64, every 257th share, and the last 64."""
    t, n, N = 2, 65535, 40
    assert not fe.fd_needs_fold(t, n)
    case = fe.SplitCase(t, n, N) if inputs == "pool" else _ConstCase(t, n, N, P - 1 if inputs == "p-1" else P)
    out = run_split(case)
    rows = sorted(set(range(1, 65)) | set(range(1, n + 1, 257)) | set(range(n - 63, n + 1)))
    vb = field.vec_bytes(N)
    sel = out[torch.tensor([x - 1 for x in rows], device=dev())].cpu().numpy()
    del out
    for r, x in enumerate(rows):
        assert_vec_equals(sel[r].reshape(vb), case.expected(x), f"t=2 n=65535 share {x}")


# ------------------------------------------------------------ c. fused draw + split, steered secrets
def _drawn_rows(seed, N, t):
    co = _native.mt_draw_coeffs(random.Random(seed), N, t - 1)
    cols = [field.vec_to_ints(co[j], N) for j in range(t - 1)]
    return [[c[e] for c in cols] for e in range(N)]


def _cpython_state_after(seed, draws):
    r = random.Random(seed)
    for _ in range(draws):
        r.randint(1, P - 1)
    return r.getstate()


class _RowsCase:
    def __init__(self, t, n, secrets, rows):
        self.t, self.n, self.N = t, n, len(secrets)
        self.rows = [[s] + list(r) for s, r in zip(secrets, rows)]

    def expected(self, x):
        return [fe.split_expected(r, x) for r in self.rows]


@pytest.mark.parametrize("N", [N_LAYOUT, 8320 + 5])
@pytest.mark.parametrize("t,n", [(2, 3), (3, 5), (5, 9)])
def test_fused_draw_split_with_steered_secrets(t, n, N):
    """make_shares_vec's coefficients are fixed by the seed: they are drawn on
    the host, and each element's int64 secret is set so that the low 64 bits
    of F at its target share x* = 1 + e mod n are all ones — the fold then
    carries out of limb 0 and past limb 1 (for 40 / 88 / 99 % of the elements,
    test_field_edges_host.py).  N = 8325 is past the one-substream sizes."""
    seed = 7
    rows = _drawn_rows(seed, N, t)
    sec = fe.steer_secrets(rows, n)
    assert _native.lib().dn_mt19937_split_supported(N, t, n) == 1
    ss = shamir.SecretShare(t)
    ss.random.seed(seed)
    out = ss.make_shares_vec(to_i64(sec), n)
    torch.cuda.synchronize()
    check_shares(out, _RowsCase(t, n, sec, rows))
    assert ss.random.getstate() == _cpython_state_after(seed, N * (t - 1))


def test_fused_draw_split_many_with_steered_secrets():
    t, n, N, seed = 3, 5, N_LAYOUT, 7
    rows = _drawn_rows(seed, N, t)
    sec = fe.steer_secrets(rows, n)
    sizes = [37, 256, 1, 300, 0, 467]
    ss = shamir.SecretShare(t)
    ss.random.seed(seed)
    outs = ss.make_shares_vec_many([to_i64(s) for s in fe.ragged(sec, sizes)], n)
    torch.cuda.synchronize()
    for out, s, r in zip(outs, fe.ragged(sec, sizes), fe.ragged(rows, sizes)):
        if len(s):
            check_shares(out, _RowsCase(t, n, s, r))
    assert ss.random.getstate() == _cpython_state_after(seed, N * (t - 1))


@pytest.mark.parametrize("t,n", [(2, 3), (3, 5)])
def test_chacha_split_with_steered_secrets(t, n):
    N, key, nonce, rounds = N_LAYOUT, bytes(range(7, 39)), 0x1234567, 20
    vb = field.vec_bytes(N)
    co = torch.zeros((t - 1, vb), dtype=torch.uint8, device=dev())
    _native.prng_coeffs(key, nonce, rounds, 0, co, N, t - 1)
    torch.cuda.synchronize()
    h = co.cpu().numpy()
    cols = [field.vec_to_ints(h[j], N) for j in range(t - 1)]
    assert all(1 <= c <= P - 1 for col in cols for c in col)
    rows = [[c[e] for c in cols] for e in range(N)]
    sec = fe.steer_secrets(rows, n)
    assert fe.steered_multi_share(rows, sec, n) >= (0.25 if t == 2 else 0.5)
    out = torch.full((n, vb), 0xA5, dtype=torch.uint8, device=dev())
    _native.split_prng(to_i64(sec).to(dev()), key, nonce, rounds, 0, out, N, t, n)
    torch.cuda.synchronize()
    check_shares(out, _RowsCase(t, n, sec, rows))


# ------------------------------------------------------------ d. reconstruct, crafted descriptors
def run_recon(case, w):
    N = case.N
    vecs = [to_vec(y) for y in case.ys]
    out = torch.full((field.vec_bytes(N),), 0xA5, dtype=torch.uint8, device=dev())
    _native.reconstruct(vecs, w, out_fe=out, n=N)
    torch.cuda.synchronize()
    return out.cpu().numpy()


_RECON = {c[0]: c for c in fe.recon_cases()}


@pytest.mark.parametrize("name", list(_RECON))
def test_reconstruct_crafted_descriptor(name):
    """A in {1, 2, 17} x INV in {0, 1, 2}; k = 2..6, 16 (every unrolled K and
    the runtime-k kernel); every small and full-width divisor; every rotation
    1..31 on residues whose low bits are all ones.  The last share is solved,
    so the residue the division sees walks multiples of d and their
    neighbours, limb boundaries, all-ones low limbs, p - 1 and p - d."""
    spec = _RECON[name]
    case = fe.recon_case_of(spec)
    assert_vec_equals(run_recon(case, fe.recon_desc_of(spec, case)), case.expected(), name)


@pytest.mark.parametrize("name", ["k3-inv0", "k5-inv2", "shift9-inv1"])
def test_reconstruct_runtime_k_kernel(name, monkeypatch):
    """DN_RECON_UNROLL=0 (tuning library): the runtime-k kernel at unrolled share counts."""
    spec = _RECON[name]
    case = fe.recon_case_of(spec)
    monkeypatch.setenv("DN_RECON_UNROLL", "0")
    with _native.library(_native.TUNING_LIB):
        got = run_recon(case, fe.recon_desc_of(spec, case))
    assert_vec_equals(got, case.expected(), name)


@pytest.mark.parametrize("neg_all", [False, True])
@pytest.mark.parametrize("A", [1, 2, 17])
def test_reconstruct_accumulator_bound(A, neg_all):
    """k = 16, every |a_i| the maximum of its width (2^32 - 1, 2^64 - 1;
    lambda_i = p - 1 for the full-width form) and every share p: the stated
    bound of the unreduced accumulator.  With every sign bit set each share
    enters as p - y = 0.  Then the same weights on the pool layout."""
    k = 16
    amax = P - 1 if A == 17 else (1 << (32 * A)) - 1
    neg = (1 << k) - 1 if neg_all else 0
    for const in (P, P - 1, None):
        case = fe.ReconCase([amax] * k, neg, N=fe.TILE + 37, const_y=const)
        w = fe.make_desc(case.a, neg, A)
        assert_vec_equals(run_recon(case, w), case.expected(), f"A={A} neg_all={neg_all} y={const and hex(const)}")


# ------------------------------------------------------------ e. results at the output edges
_OUT_TARGETS = [0, 1, M64, 1 << 64, (1 << 64) + 1, P - 1]


def _output_edge_shares(xs, N, seed):
    """k share columns whose interpolant at 0 is an output edge: shares
    0..k-2 from the layout (all zero in places), the last one solved.  A
    result 0 then comes from all-zero shares at some elements and from a
    non-zero multiple of p at others."""
    k = len(xs)
    lams = fe.lagrange_at_zero(xs)
    linv = pow(lams[-1], -1, P)
    ys = [fe.layout_values(N, seed + i, 29 * i + k) for i in range(k)]
    kinds = fe.layout_kinds(N)
    e = 0
    for i in range(N):
        if kinds[i] == "R":
            continue
        if e % 7 == 6:
            for j in range(k):
                ys[j][i] = 0  # the result 0 from zero shares
        else:
            part = sum(l * ys[j][i] for j, l in enumerate(lams[:-1]))
            ys[-1][i] = (_OUT_TARGETS[e % len(_OUT_TARGETS)] - part) * linv % P
        e += 1
    want = [sum(l * ys[j][i] for j, l in enumerate(lams)) % P for i in range(N)]
    return ys, want


@pytest.mark.parametrize("xs", [[1, 3, 5], [2, 4, 5], [1, 2, 4, 5], [2, 3, 5, 8, 9]])
def test_results_at_the_output_edges(xs):
    N, k = N_LAYOUT, len(xs)
    ys, want = _output_edge_shares(xs, N, 70)
    zero_from_multiple = sum(1 for i in range(N) if want[i] == 0 and any(ys[j][i] % P for j in range(k)))
    zero_from_zero = sum(1 for i in range(N) if want[i] == 0 and not any(ys[j][i] % P for j in range(k)))
    assert zero_from_multiple >= 8 and zero_from_zero >= 8
    assert all(want.count(v) >= 8 for v in _OUT_TARGETS)
    vecs = [to_vec(y) for y in ys]
    ss = shamir.SecretShare(k)
    res, over = ss.resolve_shares_vec(vecs, xs, N, return_overflow=True)
    fld, over_f = ss.resolve_shares_vec(vecs, xs, N, out="field", return_overflow=True)
    torch.cuda.synchronize()
    assert res.cpu().tolist() == [fe.to_i64(v & M64) for v in want]
    assert_vec_equals(fld.cpu().numpy(), want, f"xs={xs}")
    n_over = sum(v >> 64 != 0 for v in want)
    assert 0 < n_over < N
    assert int(over.item()) == n_over and int(over_f.item()) == n_over


def test_results_at_the_output_edges_many():
    xs, N = [2, 4, 5], N_LAYOUT
    k = len(xs)
    ys, want = _output_edge_shares(xs, N, 80)
    sizes = [37, 256, 0, 300, 1, 467]
    blocks = [to_block(cols) if len(cols[0]) else torch.empty((k, 0), dtype=torch.uint8, device=dev())
              for cols in zip(*[fe.ragged(y, sizes) for y in ys])]
    ss = shamir.SecretShare(k)
    res, over = ss.resolve_shares_vec_many(blocks, xs, sizes, return_overflow=True)
    fld = ss.resolve_shares_vec_many(blocks, xs, sizes, out="field")
    torch.cuda.synchronize()
    over = over.cpu().tolist()
    for j, w in enumerate(fe.ragged(want, sizes)):
        assert res[j].cpu().tolist() == [fe.to_i64(v & M64) for v in w], j
        if len(w):
            assert_vec_equals(fld[j].cpu().numpy(), w, f"segment {j}")
        assert over[j] == sum(v >> 64 != 0 for v in w), j


# ------------------------------------------------------------ f. the segmented reconstruct kernel
@pytest.mark.parametrize("name", [c[0] for c in fe.recon_many_specs()])
def test_reconstruct_many_crafted_descriptor(name):
    """reconstruct_many_kernel keeps its own copy of the loop body: every (A,
    INV) pair, every K, both rotation arms with both divisions, over three
    segments of 37, 256 and 300 elements."""
    spec = _RECON[name]
    sizes = [37, 256, 300]
    case = fe.recon_case_of(spec, N=sum(sizes))
    w = fe.recon_desc_of(spec, case)
    want = fe.ragged(case.expected(), sizes)
    segs = [[to_vec(col) for col in cols] for cols in zip(*[fe.ragged(y, sizes) for y in case.ys])]
    outs = [torch.full((field.vec_bytes(s),), 0xA5, dtype=torch.uint8, device=dev()) for s in sizes]
    u64s = [torch.zeros(s, dtype=torch.int64, device=dev()) for s in sizes]
    over = torch.zeros(len(sizes), dtype=torch.int32, device=dev())
    _native.reconstruct_many(sizes, [v.data_ptr() for seg in segs for v in seg], w, dev(),
                             out_fe_ptrs=[o.data_ptr() for o in outs], out_u64_ptrs=[o.data_ptr() for o in u64s],
                             overflow=over)
    torch.cuda.synchronize()
    for j, wj in enumerate(want):
        assert_vec_equals(outs[j].cpu().numpy(), wj, f"{name} segment {j}")
        assert u64s[j].cpu().tolist() == [fe.to_i64(v & M64) for v in wj], (name, j)
    assert over.cpu().tolist() == [sum(v >> 64 != 0 for v in wj) for wj in want]
