"""Shamir secret sharing over GF(2^521 - 1) — the `delta_node.crypto.shamir` surface.

Drop-in for delta_node/crypto/shamir/shamir.py (same names, arguments, return
values and exceptions), backed by the MI355X HIP library through its C-ABI
(`_native`, include/dn_shamir.h):

=============================  =============================================
reference (shamir.py)          here
=============================  =============================================
``Share``, ``PRIME`` :14-16    same objects
``_eval_at`` :19-25            device Horner (`dn_m521_split_fe`)
``_share_to_bytes`` :28-33     same codec (host, per share)
``_bytes_to_share`` :36-45     same codec (host, per share)
``SecretShare.__init__`` :49   same attributes: threshold, prime, random
``make_shares`` :55-66         coefficients from ``self.random`` exactly as
                               the reference draws them; evaluation in the
                               library's host path (one secret per call)
``resolve_shares`` :68-90      same checks/messages/exceptions, library host
                               path (any prime)
=============================  =============================================

Vector extension (the hot path, new): ``make_shares_vec`` splits a whole
int64 tensor, element e behaving exactly like
``make_shares(v_e.to_bytes(8, "big", signed=True), n)`` called in order on the
same instance; ``resolve_shares_vec`` interpolates whole share vectors.

There is no CPU fallback: without the native library every call raises, and
without a HIP device every vector call raises.  The byte API (one secret per
call, as the reference's callers use it) runs in the library's native host
path (csrc/host_shamir.cpp) for any prime, like the reference's
``SecretShare(t, prime=q)``; the vector API is GF(2^521 - 1) on the GPU.
"""
from __future__ import annotations

import numbers
import random
from functools import reduce
from typing import List, Optional, Sequence, Tuple, Union

from ... import serialize
from . import _args, _native, field, memory, op

__all__ = ["Share", "PRIME", "SecretShare"]

Share = Tuple[int, int]

PRIME = (1 << 521) - 1  # 0x01FF...FF, the Mersenne prime M521 (shamir.py:16)


# ------------------------------------------------------------------ codec
def _share_to_bytes(share: Share) -> bytes:
    """``[len(x) as 1 byte][x minimal BE][y minimal BE]`` (shamir.py:28-33)."""
    x, y = share
    xb = serialize.int_to_bytes(x)
    return len(xb).to_bytes(1, "big") + xb + serialize.int_to_bytes(y)


def _bytes_to_share(data: bytes) -> Share:
    """Inverse of `_share_to_bytes` (shamir.py:36-45)."""
    xl = int.from_bytes(data[:1], "big")
    return serialize.bytes_to_int(data[1:1 + xl]), serialize.bytes_to_int(data[1 + xl:])


# ------------------------------------------------------- device helpers
def _device():
    _native.lib()
    return _native.require_device()


def _to_device_vecs(ints: Sequence[int], dev):
    """Python ints (each < 2^521) -> uint8 device tensor [len, vec_bytes(1)]."""
    import numpy as np
    import torch

    host = np.stack([field.ints_to_vec([v]) for v in ints]) if ints else np.zeros((0, field.vec_bytes(1)), np.uint8)
    return torch.from_numpy(host).to(dev)


def _device_values(values, dev, name: str):
    """`values` as a contiguous 1-D int64 tensor on `dev` (no conversion when
    it already is one: the common call, a resident vector)."""
    import torch

    if (isinstance(values, torch.Tensor) and values.device == dev and values.dtype == torch.int64
            and values.dim() == 1 and values.is_contiguous()):
        return values
    vals = torch.as_tensor(values)
    if vals.dtype not in (torch.int64, torch.uint64):
        raise TypeError(f"{name}: values must be an int64 tensor")
    return vals.reshape(-1).to(dev).contiguous()


def _concat_values(vals: Sequence):
    """The concatenation of contiguous 1-D int64 device tensors (at least one
    non-empty) as one such tensor: the tensors' own memory when they lie back
    to back in one buffer (a model kept as views of one flat parameter
    vector), else one torch.cat on the device."""
    import torch

    live = [v for v in vals if v.numel()]
    if len(live) == 1:
        return live[0]
    base, end = live[0].untyped_storage().data_ptr(), live[0].data_ptr()
    for v in live:
        if v.untyped_storage().data_ptr() != base or v.data_ptr() != end:
            return torch.cat(live)
        end += 8 * v.numel()
    return torch.as_strided(live[0], (sum(v.numel() for v in live),), (1,))


def _eval_many(coeffs: Sequence[int], n_shares: int) -> List[int]:
    """y(x) = sum_j coeffs[j] x^j mod p for x = 1..n_shares, on the GPU.
    coeffs[0] is the secret (any size; reduced mod p here).  The split takes
    no threshold above its share count, which `_eval_at` does not know of
    (the reference evaluates t coefficients at x = 1): with more coefficients
    than shares, len(coeffs) rows are computed and the first n_shares kept."""
    import torch

    dev = _device()
    t = len(coeffs)
    rows = max(n_shares, t)
    sec = _to_device_vecs([coeffs[0] % PRIME], dev)
    cof = _to_device_vecs(list(coeffs[1:]), dev) if t > 1 else None
    out = torch.empty((rows, field.vec_bytes(1)), dtype=torch.uint8, device=dev)
    _native.split_fe(sec, cof, out, 1, t, rows)
    host = out[:n_shares].cpu().numpy()
    return [field.vec_to_ints(host[i], 1)[0] for i in range(n_shares)]


def _eval_at(coeffs: List[int], x: int, prime: int) -> int:
    """Horner evaluation of `coeffs` at x mod prime (shamir.py:19-25).

    GF(2^521 - 1) with 1 <= x <= 65535 and at most 64 coefficients runs the
    device split (`dn_m521_split_fe`); every other input — another prime
    (negative too), x = 0, a negative or larger x, more coefficients — runs
    the library's host Horner (`dn_shamir_eval_at_host`), which computes
    exactly what the reference's loop computes for any integers."""
    if not coeffs:
        return 0
    if prime == PRIME and 1 <= x <= _native.MAX_SHARES and len(coeffs) <= _native.MAX_THRESHOLD:
        return _eval_many([c % prime for c in coeffs], x)[x - 1]
    return _native.host_eval_at([int(c) for c in coeffs], int(x), int(prime))


def _draw_coeffs_generic(rng, n: int, tm1: int):
    """The reference's own draw for a generator that is not plain MT19937
    (random.SystemRandom, a subclass overriding randint / getrandbits ...):
    `rng.randint(1, p - 1)` per coefficient, element-major (shamir.py:59-61),
    packed as a host block [tm1, vec_bytes(n)]."""
    import numpy as np

    cols = [[0] * n for _ in range(tm1)]
    for e in range(n):
        for j in range(tm1):
            cols[j][e] = rng.randint(1, PRIME - 1)
    return np.stack([field.ints_to_vec(c) for c in cols])


def _lagrange_generic(xs: Sequence[int], prime: int) -> List[int]:
    """lambda_i = prod_{j!=i} (-x_j) / prod_{j!=i} (x_i - x_j) mod p, as the
    reference forms nums/dens (shamir.py:77-83) and divides (op.py:28-29)."""
    k = len(xs)
    lams = []
    for i in range(k):
        num = reduce(lambda a, b: a * b, [-xs[j] for j in range(k) if j != i])
        den = reduce(lambda a, b: a * b, [xs[i] - xs[j] for j in range(k) if j != i])
        lams.append(op.div_mod(num % prime, den, prime))
    return lams


def _resolve_vectors(vecs: Sequence, xs: Sequence[int], n: int, threshold: int,
                     out_fe=None, out_u64=None, overflow=None) -> None:
    """Lagrange-at-0 of device share vectors `vecs` (abscissas xs) into
    out_fe / out_u64, on the GPU.  k <= 16 with 64-bit xs uses the native
    small-rational weights; otherwise full-width weights in groups of 16 whose
    partial vectors are then summed mod p on the device."""
    import torch

    k = len(xs)
    if k <= _native.MAX_RESOLVE and all(_args.fits_u64(int(x)) for x in xs):
        w = _native.lagrange(xs, threshold)
        _native.reconstruct(vecs, w, out_fe=out_fe, out_u64=out_u64, overflow=overflow, n=n)
        return
    lams = _lagrange_generic([int(x) for x in xs], PRIME)
    vb = field.vec_bytes(n)
    dev = vecs[0].device
    G = _native.MAX_RESOLVE
    parts = []
    for g in range(0, k, G):
        part = torch.empty(vb, dtype=torch.uint8, device=dev)
        _native.reconstruct(vecs[g:g + G], _native.generic_weights(lams[g:g + G]), out_fe=part, n=n)
        parts.append(part)
    while len(parts) > G:  # sum partial vectors mod p, 16 at a time
        merged = []
        for g in range(0, len(parts), G):
            dst = torch.empty(vb, dtype=torch.uint8, device=dev)
            _native.reconstruct(parts[g:g + G], _native.ones_weights(len(parts[g:g + G])), out_fe=dst, n=n)
            merged.append(dst)
        parts = merged
    _native.reconstruct(parts, _native.ones_weights(len(parts)), out_fe=out_fe, out_u64=out_u64,
                        overflow=overflow, n=n)


def _i64(x: int) -> int:
    """A 64-bit abscissa as the int64 a decoded `xs` tensor holds for it."""
    return x - (1 << 64) if x >= (1 << 63) else x


def _first_record_xs(recs, what: str = "resolve_records_vec") -> List[int]:
    """The abscissa in the header `[len(x)][x]` of every wire's first record
    (`_bytes_to_share`, shamir.py:36-45): offsets[0:2] and at most 9 bytes per
    wire, gathered on the device and read back in one copy."""
    import torch

    idx = torch.arange(9, device=recs[0][0].device)
    heads, spans = [], []
    for packed, offsets in recs:
        spans.append(offsets[:2])
        if packed.numel():
            heads.append(packed[(offsets[0] + idx).clamp(0, packed.numel() - 1)].to(torch.int64))
        else:
            heads.append(torch.zeros(9, dtype=torch.int64, device=packed.device))
    host = torch.cat(spans + heads).cpu().tolist()
    k = len(recs)
    xs = []
    for i, (packed, _) in enumerate(recs):
        o0, o1 = host[2 * i], host[2 * i + 1]
        head = host[2 * k + 9 * i:2 * k + 9 * i + 9]
        if not (0 <= o0 < o1 <= packed.numel()) or head[0] > 8 or 1 + head[0] > o1 - o0:
            raise ValueError(f"{what}: the first record of wire {i} has no readable x")
        xs.append(int.from_bytes(bytes(head[1:1 + head[0]]), "big"))
    return xs


# ------------------------------------------------------------------ API
class SecretShare(object):
    """Threshold-`threshold` Shamir scheme over GF(PRIME) (shamir.py:48-90)."""

    def __init__(self, threshold: int, *, prime: int = PRIME):
        self.threshold = threshold
        self.prime = prime
        self.random = random.Random()
        self.last_draw_rejected = False

    def _require_m521(self):
        if self.prime != PRIME:
            raise NotImplementedError("the vector (GPU) path is GF(2^521 - 1) only; the byte API takes any prime")

    # ---- reference byte API -------------------------------------------
    def make_shares(self, value: bytes, shares: int) -> List[bytes]:
        """Split `value` into `shares` byte shares (shamir.py:55-66).

        One secret per call — the reference's callers' pattern — so the field
        arithmetic runs in the library's host path (dn_shamir_make_shares_host:
        a GPU launch and two copies would cost ~20x the reference's latency);
        the coefficients are drawn from `self.random` exactly as the reference
        draws them."""
        if self.threshold > shares:
            raise ValueError("threshold should be little equal than shares")
        serialize.bytes_to_int(value)  # the reference's conversion (and its errors)
        coeffs = [self.random.randint(1, self.prime - 1) for _ in range(self.threshold - 1)]
        if shares <= 0:
            return []
        return _native.host_make_shares(bytes(value), coeffs, self.prime, self.threshold, shares)

    def resolve_shares(self, shares: List[bytes]) -> bytes:
        """Recover the secret from byte shares (shamir.py:68-90): the
        Lagrange interpolant of ALL given shares at 0, minimal big-endian, with
        the reference's checks and messages (dn_shamir_resolve_shares_host)."""
        shares = [bytes(s) for s in shares]
        if not shares:  # zip(*[]) unpacked into xs, ys
            raise ValueError("not enough values to unpack (expected 2, got 0)")
        return _native.host_resolve_shares(shares, self.threshold, self.prime)

    # ---- vector extension (the hot path) -------------------------------
    def draw_coeffs_vec(self, n: int, device=None, *, elem_offset: int = 0, n_total: Optional[int] = None):
        """The (t-1) x n coefficients that n sequential `make_shares` calls
        would draw from `self.random` (advancing it identically), as a uint8
        device tensor [t-1, vec_bytes(n)] in the tiled layout.

        Sharded form (elem_offset / n_total): the coefficients of elements
        [elem_offset, elem_offset + n) of an n_total-element draw — the words
        before the shard are skipped by jump-ahead (dn_mt19937_skip) — and
        `self.random` ends as after the whole n_total-element draw.  Exact
        unless a 521-bit draw is rejected (odds ~2^-520 each) in the skipped
        range; `self.last_draw_rejected` reports one in this shard's range, and
        `dist.draw_coeffs_sharded` combines the flags over ranks."""
        self._require_m521()
        import torch

        dev = device if device is not None else _device()
        tm1 = max(self.threshold, 1) - 1
        sharded = elem_offset != 0 or (n_total is not None and n_total != n)
        if not _native.mt_compatible(self.random):
            # not CPython's MT19937 draw: call it, as the reference does
            if sharded:
                raise NotImplementedError("draw_coeffs_vec: a sharded draw needs a plain random.Random "
                                          f"(jump-ahead), not {type(self.random).__name__}")
            self.last_draw_rejected = False
            if tm1 <= 0 or n <= 0:
                return torch.zeros((max(tm1, 0), field.vec_bytes(n)), dtype=torch.uint8, device=dev)
            return torch.from_numpy(_draw_coeffs_generic(self.random, n, tm1)).to(dev)
        if sharded:
            if n_total is None or not 0 <= elem_offset <= elem_offset + n <= n_total:
                raise ValueError("draw_coeffs_vec: shard [elem_offset, elem_offset + n) must lie in [0, n_total)")
            rng = random.Random()
            rng.setstate(self.random.getstate())
            _native.mt_skip(rng, 17 * tm1 * elem_offset)
        else:
            rng = self.random
        self.last_draw_rejected = False
        blk = None
        if tm1 > 0 and n > 0 and torch.device(dev).type == "cuda":
            # bit-exact MT19937 on the GPU (jump-ahead substreams); the host
            # draw below is the fallback for a rejected draw (odds ~2^-520)
            vb = field.vec_bytes(n)
            # a share-block allocation (memory.py): the split reads it at 2 x 66 B per
            # element; 1-2 % faster from a probed 2 MiB-chunk block (profiles/r04/p/)
            blk = memory.share_block((tm1, vb), dev)
            if n % field.TILE:
                blk[:, vb - field.TILE_BYTES:].zero_()  # padding lanes of the last tile, as the host draw leaves them
            if not _native.mt_draw_coeffs_device(rng, n, tm1, blk):
                blk = None
        if blk is None:
            probe = random.Random()
            probe.setstate(rng.getstate())
            host = _native.mt_draw_coeffs(rng, n, tm1)
            _native.mt_skip(probe, 17 * tm1 * n)
            self.last_draw_rejected = probe.getstate() != rng.getstate()  # a rejection consumed extra words
            blk = torch.from_numpy(host).to(dev)
        if sharded:
            _native.mt_skip(self.random, 17 * tm1 * n_total)
        return blk

    def make_shares_vec(self, values, shares: int, *, coeffs=None, out=None):
        """Split every element of an int64 tensor.

        values  int64 tensor [N] (any device; copied to the current HIP device)
        coeffs  optional uint8 device tensor [t-1, vec_bytes(N)]; default: drawn
                from `self.random` as N sequential `make_shares` calls would
        out     optional uint8 device tensor [shares, vec_bytes(N)]; default: a
                pooled block of 16 MiB physical chunks (memory.share_block)
        Returns uint8 device tensor [shares, vec_bytes(N)]: row x-1 holds share x
        of every element (tiled M521 layout, canonical residues).
        """
        self._require_m521()
        import torch

        _args.check_limits("make_shares_vec", self.threshold, shares, _native.MAX_SHARES, _native.MAX_THRESHOLD)
        dev = _device()
        vals = _device_values(values, dev, "make_shares_vec")
        n = vals.numel()
        t = max(self.threshold, 1)
        vb = field.vec_bytes(n)
        if out is None:  # pooled chunked block (memory.py: the split's fast placement)
            out = memory.share_block((max(shares, 0), vb), dev)
        else:
            _args.check_share_out("make_shares_vec", out, shares, vb, dev)
        if (coeffs is None and t > 1 and n > 0 and shares > 0 and _native.mt_compatible(self.random)
                and _native.mt_split_device(self.random, vals, out, n, t, shares)):
            # fused: the reference's MT19937 draws feed the split in registers (no coefficient block)
            self.last_draw_rejected = False
            return out
        if coeffs is None:
            coeffs = self.draw_coeffs_vec(n, dev) if t > 1 else None
        elif t > 1:
            if coeffs.dtype != torch.uint8 or tuple(coeffs.shape) != (t - 1, vb) or coeffs.device != dev:
                raise ValueError(f"make_shares_vec: coeffs must be uint8 [{t - 1}, {vb}] on {dev}")
            coeffs = coeffs.contiguous()
        if shares > 0:
            _native.split_u64(vals, coeffs if t > 1 else None, out, n, t, shares)
        return out

    def make_shares_vec_many(self, tensors, shares: int, *, outs=None) -> list:
        """`[self.make_shares_vec(x, shares) for x in tensors]` in one fused
        draw + split — the runner's walk over a model's tensors
        (runner/horizontal/agg.py:294-316) as one call.

        make_shares draws every coefficient from one sequential stream
        (shamir.py:59-61), so the per-tensor calls draw exactly the words one
        split of the tensors' concatenation draws: the results, element for
        element, and the final `self.random.getstate()` are identical.

        tensors  sequence of int64 tensors (any shape and device; each read
                 flattened in C order, as make_shares_vec reads one)
        outs     optional list of uint8 device tensors, outs[k] contiguous
                 [shares, vec_bytes(n_k)]; default: contiguous views of ONE
                 pooled block (memory.share_block) of shares * sum
                 vec_bytes(n_k) bytes, reused as a whole
        Returns one uint8 device tensor [shares, vec_bytes(n_k)] per input, in
        order ([shares, 0] for an empty one).

        The secrets go to the kernel as one int64 vector: the inputs' own
        buffer when they are consecutive views of one contiguous device
        buffer, else one torch.cat on the device (16 B per element against
        338 B of share traffic at 3-of-5).  Where the fused form does not
        apply (a generator that is not plain MT19937, t not in {2, 3, 5}, a
        stream beyond the jump table, a rejected draw) the per-tensor
        make_shares_vec loop runs into the same outputs, and
        `self.last_draw_rejected` reports a redraw in any of the tensors."""
        self._require_m521()
        import torch

        _args.check_limits("make_shares_vec_many", self.threshold, shares, _native.MAX_SHARES, _native.MAX_THRESHOLD)
        dev = _device()
        vals = [_device_values(x, dev, "make_shares_vec_many") for x in tensors]
        ns = [v.numel() for v in vals]
        vbs = [field.vec_bytes(n) for n in ns]
        t = max(self.threshold, 1)
        rows = max(shares, 0)
        if outs is None:
            blk = memory.share_block((rows * sum(vbs),), dev)
            parts = torch.split(blk, [rows * vb for vb in vbs]) if vbs else ()
            outs = [p.view(rows, vb) for p, vb in zip(parts, vbs)]
            ptrs, off = [], blk.data_ptr()
            for vb in vbs:
                ptrs.append(off)
                off += rows * vb
        else:
            outs = list(outs)
            if len(outs) != len(vals):
                raise ValueError(f"make_shares_vec_many: {len(outs)} outs for {len(vals)} tensors")
            for out, vb in zip(outs, vbs):
                if (out.dtype != torch.uint8 or tuple(out.shape) != (shares, vb) or not out.is_contiguous()
                        or out.device != dev):  # (inline: no call per tensor)
                    _args.check_share_out("make_shares_vec_many", out, shares, vb, dev)
            ptrs = [out.data_ptr() for out in outs]
        if (t in (2, 3, 5) and shares > 0 and sum(ns) > 0 and _native.mt_compatible(self.random)
                and _native.mt_split_many_device(self.random, _concat_values(vals), list(zip(ns, ptrs)), t, shares)):
            self.last_draw_rejected = False
            return outs
        rejected = self.last_draw_rejected = False
        for v, out in zip(vals, outs):  # the calls this one stands for, into the same outputs
            self.make_shares_vec(v, shares, out=out)
            rejected = rejected or self.last_draw_rejected
        self.last_draw_rejected = rejected  # a redraw in any tensor, not only in the last one
        return outs

    def make_shares_vec_prng(self, values, shares: int, *, key: Optional[bytes] = None, nonce: int = 0,
                             rounds: int = 20, elem_offset: int = 0, out=None):
        """Split every element with coefficients generated on the device.

        Same shares layout as `make_shares_vec`, but the coefficients come from
        a keyed ChaCha stream (dn_m521_split_prng) instead of `self.random`:
        each is uniform in [1, p-1] and depends only on (key, nonce, global
        element index elem_offset + e), so sharded calls reproduce the
        unsharded result.  key: 32 bytes (default: fresh from `secrets`);
        rounds: 20 (default), 12 or 8.  Returns (shares block, key).
        """
        self._require_m521()
        import secrets as _secrets

        import torch

        _args.check_limits("make_shares_vec_prng", self.threshold, shares, _native.MAX_SHARES, 8)
        if key is None:
            key = _secrets.token_bytes(32)
        dev = _device()
        vals = _device_values(values, dev, "make_shares_vec_prng")
        n = vals.numel()
        vb = field.vec_bytes(n)
        if out is None:
            out = memory.share_block((max(shares, 0), vb), dev)
        else:
            _args.check_share_out("make_shares_vec_prng", out, shares, vb, dev)
        if shares > 0:
            if self.threshold <= 1:
                _native.split_u64(vals, None, out, n, 1, shares)
            else:
                _native.split_prng(vals, key, nonce, rounds, elem_offset, out, n, self.threshold, shares)
        return out, key

    def resolve_shares_vec(self, shares, xs: Sequence[int], n: int, *, out: str = "int64",
                           return_overflow: bool = False):
        """Interpolate share vectors at 0 (vector form of `resolve_shares`).

        shares  sequence of k uint8 device tensors [vec_bytes(n)] (or a [k, vec_bytes(n)] tensor)
        xs      their abscissas (share x of `make_shares_vec` is row x-1)
        out     "int64": int64 tensor [n] holding the low 64 bits (the secret's
                two's-complement view); "field": uint8 tiled vector [vec_bytes(n)]
        return_overflow  also return a uint32 device counter of elements >= 2^64
                (and read every limb: without it the int64 words come from the
                five limbs of each share they depend on, exact for every result
                below 2^480 — dn_m521_reconstruct in include/dn_shamir.h)
        Same checks as `resolve_shares` (too few, duplicates, k == 1).
        """
        self._require_m521()
        import torch

        vecs = _args.rows_of(shares)
        xs = [int(x) for x in xs]
        if len(vecs) != len(xs):
            raise ValueError("resolve_shares_vec: one abscissa per share vector")
        self._check_abscissas(xs)
        dev = _device()
        vb = field.vec_bytes(n)
        for v in vecs:
            if v.dtype != torch.uint8 or v.numel() != vb or v.device != dev or not v.is_contiguous():
                raise ValueError(f"resolve_shares_vec: share vectors must be contiguous uint8 [{vb}] on {dev}")
        over = torch.zeros(1, dtype=torch.int32, device=dev) if return_overflow else None
        _args.check_out_form("resolve_shares_vec", out)
        res, out_fe, out_u64 = _args.result(out, n, vb, dev)
        _resolve_vectors(vecs, xs, n, self.threshold, out_fe=out_fe, out_u64=out_u64, overflow=over)
        return (res, over) if return_overflow else res

    def resolve_records_vec(self, records, xs: Optional[Sequence[int]], n: int, *, out: str = "int64",
                            return_overflow: bool = False, bad=None):
        """Interpolate at 0 straight from wire records — `resolve_shares`
        (shamir.py:68-90) takes the shares as they arrive, a list of
        `_share_to_bytes` records; this is its vector form, in one launch and
        without the k decoded vectors (dn_m521_reconstruct_records).

        records  sequence of k (packed, offsets) pairs as
                 `codec.encode_share_vec` returns them: packed a contiguous
                 uint8 device tensor, offsets a contiguous int64 device tensor
                 of at least n + 1 entries.  A `packed` view that is not 4-byte
                 aligned is copied once, as decode_share_vec copies it
        xs       the k abscissas; None takes each wire's x from its first
                 record, as the reference takes it from the data — one
                 read-back of offsets[0:2] and at most 9 record bytes per wire,
                 the only form that synchronises before the launch
        n        elements
        out, return_overflow  as resolve_shares_vec
        bad      None: one read-back after the launch, and ValueError naming
                 both counts when a record cannot be represented (x > 8 bytes,
                 y > 68 bytes, offsets decreasing or past the wire) or carries
                 an x other than its wire's.  An int32 device tensor [2]: the
                 two counts are ADDED to it on the device and the call does not
                 synchronise; `codec.check_bad_records(bad)` raises later.
                 This form (with xs given) can be captured into a graph; there
                 is no out= tensor, so the result is then allocated from the
                 graph's pool and rewritten by every replay
        Same checks, messages and exception types as `resolve_shares_vec`, all
        before any device use.  The results are those of decode_share_vec on
        every wire followed by resolve_shares_vec, bit for bit (an
        unrepresentable record counts as y = 0 there and here).  Where the
        native form does not apply (k > 16, an abscissa outside 64 bits) the
        wires are decoded with decode_share_vec and interpolated by the grouped
        full-width path: the same results, on the GPU (there the second count
        comes from the decoded xs, so it also counts the unrepresentable
        records, whose x the decoder leaves unparsed)."""
        self._require_m521()
        import torch

        from . import codec

        what = "resolve_records_vec"
        recs = _args.wire_pairs(what, records)
        if xs is not None:
            xs = [int(x) for x in xs]
            if len(recs) != len(xs):
                raise ValueError("resolve_records_vec: one abscissa per wire")
            self._check_abscissas(xs)
        elif not recs:
            raise ValueError("not enough values to unpack (expected 2, got 0)")
        _args.check_out_form(what, out)
        n = int(n)
        if n < 0:
            raise ValueError("resolve_records_vec: n must not be negative")
        first = _args.check_wires(what, recs, n)
        _args.check_bad_flag(what, bad, first, "records")
        if xs is None and n == 0:
            raise ValueError("resolve_records_vec: xs=None needs a first record to read each abscissa from")
        dev = _device()
        if first != dev:
            raise ValueError(f"resolve_records_vec: records must be on {dev}")
        if xs is None:
            xs = _first_record_xs(recs)
            self._check_abscissas(xs)
        k = len(xs)
        bad, checked = _args.bad_flag(bad, dev)
        over = torch.zeros(1, dtype=torch.int32, device=dev) if return_overflow else None
        res, out_fe, out_u64 = _args.result(out, n, field.vec_bytes(n), dev)
        if k <= _native.MAX_RESOLVE and all(_args.fits_u64(x) for x in xs):
            recs, wires = _args.aligned_wires(recs)
            w = _native.lagrange(xs, self.threshold)
            _native.reconstruct_records(wires, xs, w, bad, out_fe=out_fe, out_u64=out_u64, overflow=over, n=n)
        else:  # decode every wire, then the grouped full-width interpolation: the same results
            vecs = []
            for (p, o), x in zip(recs, xs):
                v, got = codec.decode_share_vec(p, o, n, bad=bad[0:1])
                if _args.fits_u64(x):  # (a record's x is 64 bits at most: a larger abscissa never matches)
                    bad[1:2] += (got != _i64(x)).sum().to(torch.int32)
                else:
                    bad[1:2] += n
                vecs.append(v)
            _resolve_vectors(vecs, xs, n, self.threshold, out_fe=out_fe, out_u64=out_u64, overflow=over)
        if checked:
            codec.check_bad_records(bad)
        return (res, over) if return_overflow else res

    def _check_abscissas(self, xs: Sequence[int]) -> None:
        """resolve_shares' checks on the abscissas (shamir.py:70-83), with its messages."""
        if len(xs) == 0:
            raise ValueError("not enough values to unpack (expected 2, got 0)")
        k = len(xs)
        if k < self.threshold:
            raise ValueError("need at least {} shares".format(self.threshold))
        if k != len(set(xs)):
            raise ValueError("shares must be distinct")
        if k == 1:
            raise TypeError("reduce() of empty iterable with no initial value")

    def resolve_shares_vec_many(self, shares, xs: Sequence[int], ns: Sequence[int], *, out: str = "int64",
                                outs=None, return_overflow: bool = False):
        """`[self.resolve_shares_vec(shares[j], xs, ns[j], out=out) for j ...]`
        in one launch — the receiving side of `make_shares_vec_many`.

        shares  per tensor j: a uint8 device tensor [k, vec_bytes(ns[j])] whose
                rows are in `xs` order, or a sequence of k contiguous vectors
                [vec_bytes(ns[j])] (`[blk[x - 1] for x in xs]` on a block of
                make_shares_vec_many)
        xs      the k abscissas, shared by all tensors
        ns      elements per tensor
        out     as resolve_shares_vec
        outs    optional caller outputs, outs[j] contiguous int64 [ns[j]]
                (out="int64") or uint8 [vec_bytes(ns[j])] (out="field");
                default: consecutive views of ONE allocation
        return_overflow  also return one int32 device tensor [len(ns)]: per
                tensor, its elements >= 2^64
        Same checks as `resolve_shares_vec`, before any device work.  The
        Lagrange weights are computed once.  Nothing here synchronises.  Where
        the one-launch form does not apply (k > 16, an abscissa outside 64
        bits: the grouped full-width path) the per-tensor loop runs into the
        same outputs."""
        self._require_m521()
        import torch

        shares, ns = list(shares), [int(n) for n in ns]
        xs = [int(x) for x in xs]
        k = len(xs)
        if len(shares) != len(ns):
            raise ValueError(f"resolve_shares_vec_many: {len(shares)} share entries for {len(ns)} tensors")
        for sh in shares:
            if (sh.shape[0] if isinstance(sh, torch.Tensor) and sh.dim() == 2 else len(sh)) != k:
                raise ValueError("resolve_shares_vec: one abscissa per share vector")
        self._check_abscissas(xs)
        _args.check_out_form("resolve_shares_vec_many", out)
        dev = _device()
        vbs = [field.vec_bytes(n) for n in ns]
        u8 = torch.uint8
        rows: List[int] = []  # k row addresses per tensor
        for sh, vb in zip(shares, vbs):
            if isinstance(sh, torch.Tensor) and sh.dim() == 2:
                if sh.dtype != u8 or sh.shape[1] != vb or sh.device != dev or not sh.is_contiguous():
                    raise ValueError(f"resolve_shares_vec_many: share rows must be contiguous uint8 [{k}, {vb}] on {dev}")
                p = sh.data_ptr()
                rows.extend(range(p, p + k * vb, vb) if vb else [p] * k)
                continue
            for v in sh:
                if v.dtype != u8 or v.numel() != vb or v.device != dev or not v.is_contiguous():
                    raise ValueError(f"resolve_shares_vec_many: share vectors must be contiguous uint8 [{vb}] on {dev}")
                rows.append(v.data_ptr())
        as_int = out == "int64"
        sizes = ns if as_int else vbs
        if outs is None:
            flat = torch.empty(sum(sizes), dtype=torch.int64 if as_int else u8, device=dev)
            outs = list(torch.split(flat, sizes)) if sizes else []
            optrs, off, step = [], flat.data_ptr(), 8 if as_int else 1
            for sz in sizes:
                optrs.append(off)
                off += step * sz
        else:
            outs = list(outs)
            if len(outs) != len(ns):
                raise ValueError(f"resolve_shares_vec_many: {len(outs)} outs for {len(ns)} tensors")
            want = torch.int64 if as_int else u8
            for o, sz in zip(outs, sizes):
                if o.dtype != want or tuple(o.shape) != (sz,) or not o.is_contiguous() or o.device != dev:
                    raise ValueError(f"resolve_shares_vec_many: out must be contiguous {out} [{sz}] on {dev}")
            optrs = [o.data_ptr() for o in outs]
        over = torch.zeros(len(ns), dtype=torch.int32, device=dev) if return_overflow else None
        if k <= _native.MAX_RESOLVE and all(_args.fits_u64(x) for x in xs):
            if ns:
                w = _native.lagrange(xs, self.threshold)
                _native.reconstruct_many(ns, rows, w, dev, out_fe_ptrs=None if as_int else optrs,
                                         out_u64_ptrs=optrs if as_int else None, overflow=over)
        else:  # the calls this one stands for, into the same outputs
            for j, (sh, n, o) in enumerate(zip(shares, ns, outs)):
                _resolve_vectors(_args.rows_of(sh), xs, n, self.threshold, out_fe=None if as_int else o,
                                 out_u64=o if as_int else None, overflow=None if over is None else over[j:j + 1])
        return (outs, over) if return_overflow else outs

    def sum_shares_vec(self, blocks, *, signs=None, out=None):
        """Sum members' share vectors mod p, element-wise, in one launch —
        the party-side step of share-domain aggregation.

        Shamir is additively homomorphic: party x that receives share x of
        every member's tensor and adds the m vectors holds share x of the
        tensors' sum, so `resolve_shares_vec` on any t parties' sums gives the
        sum of the members' tensors and nobody sees a single member's.

        blocks  sequence of m uint8 device tensors of one shape, contiguous,
                numel a multiple of field.TILE_BYTES: vectors [vec_bytes(n)],
                blocks [S, vec_bytes(n)] or the flat buffer behind a
                make_shares_vec_many result alike (the sum is tile-local; all
                256 lanes of every tile are summed: zero padding in, zero
                padding out).  One tensor [m, ...] is unbound along dim 0
        signs   optional m values, each +1 or -1 (-1: subtract that member —
                one dropped after the sum was taken)
        out     optional tensor of the blocks' shape, dtype and device; it may
                be one of the blocks (accumulate in place).  Default:
                torch.empty_like(blocks[0])
        Returns the output tensor: canonical residues.  Runs on the current
        stream and does not synchronise; uses neither self.threshold nor
        self.random.  Any m: beyond DN_M521_SUM_GROUP inputs the native entry
        point chains launches that accumulate into `out`."""
        self._require_m521()
        import torch

        blocks = list(blocks.unbind(0)) if isinstance(blocks, torch.Tensor) and blocks.dim() >= 1 else list(blocks)
        if not blocks:
            raise ValueError("sum_shares_vec: no blocks")
        first = blocks[0]
        for b in blocks:
            if not isinstance(b, torch.Tensor) or b.dtype != torch.uint8:
                raise ValueError("sum_shares_vec: blocks must be uint8 tensors")
            if b.shape != first.shape or b.device != first.device:
                raise ValueError(f"sum_shares_vec: blocks must share one shape and device, got {tuple(b.shape)} on "
                                 f"{b.device} next to {tuple(first.shape)} on {first.device}")
            if not b.is_contiguous():
                raise ValueError("sum_shares_vec: blocks must be contiguous")
        if first.numel() % field.TILE_BYTES:
            raise ValueError(f"sum_shares_vec: blocks must be whole {field.TILE_BYTES}-byte tiles, "
                             f"got {first.numel()} bytes")
        negate = _args.negate_flags("sum_shares_vec", signs, len(blocks), "blocks")
        if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8
                                or out.shape != first.shape or out.device != first.device
                                or not out.is_contiguous()):
            raise ValueError(f"sum_shares_vec: out must be contiguous uint8 {tuple(first.shape)} on {first.device}")
        dev = _device()
        if first.device != dev:
            raise ValueError(f"sum_shares_vec: blocks must be on {dev}")
        if out is None:
            out = torch.empty_like(first)
        _native.sum_vecs([b.data_ptr() for b in blocks], negate, out.data_ptr(), first.numel() // field.TILE_BYTES)
        return out

    def sum_records_vec(self, records, x: Optional[int], n: int, *, signs=None, acc=None, out=None, bad=None):
        """`sum_shares_vec` straight from wire records — the party-side sum as
        the shares arrive: party x holds share x of every member's tensor as m
        wires, and their sum mod p is share x of the tensors' sum.  One launch,
        without the m decoded vectors (dn_m521_sum_records).

        records  sequence of m >= 1 (packed, offsets) pairs as
                 `codec.encode_share_vec` returns them: packed a contiguous
                 uint8 device tensor, offsets a contiguous int64 device tensor
                 of at least n + 1 entries.  A `packed` view that is not 4-byte
                 aligned is copied once, as decode_share_vec copies it
        x        the abscissa every record should carry (below 2^64); None
                 takes it from each wire's first record — one read-back of
                 offsets[0:2] and at most 9 record bytes per wire, the only form
                 that synchronises before the launch — and raises ValueError if
                 the wires disagree (it needs n > 0)
        n        elements
        signs    optional m values, each +1 or -1 (-1: subtract that member),
                 as in sum_shares_vec
        acc      optional tiled vector added to the sum: contiguous uint8
                 [vec_bytes(n)] on the records' device.  It may be `out`
                 (accumulate as members' wires arrive)
        out      optional output of the same form; default: a fresh tensor.
                 Every byte is written: the lanes past n of the last tile as
                 zero, whatever acc holds there
        bad      None: one read-back after the launch, and ValueError naming
                 both counts when a record cannot be represented (x > 8 bytes,
                 y > 68 bytes, offsets decreasing or past the wire) or carries
                 an x other than `x`.  An int32 device tensor [2]: the two
                 counts are ADDED to it on the device and the call does not
                 synchronise; `codec.check_bad_records(bad,
                 what="sum_records_vec")` raises later
        Returns `out`: canonical residues, bit for bit those of
        decode_share_vec on every wire followed by sum_shares_vec (an
        unrepresentable record counts as y = 0 there and here).  Every argument
        error is raised before any device use; n = 0 returns an empty vector.
        Uses neither self.threshold nor self.random.  Any m: beyond
        DN_M521_SUM_RECORDS_GROUP wires the native entry point chains launches
        that accumulate into `out`.

        There is no tensor-list form because none is needed: the concatenated
        wire of `codec.encode_shares_many` IS the wire of one n_total-element
        vector, so the m members' list wires are summed by this method with
        n = n_total, and the sum re-encoded with `codec.encode_share_vec(sum,
        n_total, x)` is what `resolve_records_vec(..., n_total)` reads."""
        self._require_m521()
        import torch

        from . import codec

        what = "sum_records_vec"
        recs = _args.wire_pairs(what, records)
        if not recs:
            raise ValueError(f"{what}: no records")
        n = int(n)
        if n < 0:
            raise ValueError(f"{what}: n must not be negative")
        first = _args.check_wires(what, recs, n)
        if x is not None:
            if isinstance(x, bool) or not isinstance(x, numbers.Integral):
                raise ValueError(f"{what}: x must be an integer or None")
            x = int(x)
            if not _args.fits_u64(x):
                raise ValueError(f"{what}: x must fit 64 bits")
        elif n == 0:
            raise ValueError(f"{what}: x=None needs a first record to read the abscissa from")
        negate = _args.negate_flags(what, signs, len(recs), "wires")
        vb = field.vec_bytes(n)
        for name, t in (("acc", acc), ("out", out)):
            if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == torch.uint8
                                      and tuple(t.shape) == (vb,) and t.is_contiguous() and t.device == first):
                raise ValueError(f"{what}: {name} must be a contiguous uint8 tensor [{vb}] on the records' device")
        _args.check_bad_flag(what, bad, first, "records")
        dev = _device()
        if first != dev:
            raise ValueError(f"{what}: records must be on {dev}")
        if x is None:
            got = _first_record_xs(recs, what)
            if len(set(got)) != 1:
                raise ValueError(f"{what}: the wires' first records carry different abscissas: {got}")
            x = got[0]
        if out is None:
            out = torch.empty(vb, dtype=torch.uint8, device=dev)
        if n == 0:
            return out
        bad, checked = _args.bad_flag(bad, dev)
        recs, wires = _args.aligned_wires(recs)
        _native.sum_records(wires, x, negate, bad, out, acc=acc, n=n)
        if checked:
            codec.check_bad_records(bad, what=what)
        return out
