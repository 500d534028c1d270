"""Share wire codec over whole vectors.

Record e of an encoded share vector is exactly the reference's
`_share_to_bytes((x, y_e))` (shamir.py:28-33): `[len(xb)][xb][yb]` with
minimal big-endian xb / yb.  Records are packed back to back in one uint8
device tensor with int64 offsets[n + 1] (record e = packed[offsets[e]:offsets[e+1]]),
which is what goes to the HTTP peer for receiver x instead of n Python
`bytes` objects.  Encoding / decoding run on the GPU (dn_m521_encode_shares /
dn_m521_decode_shares); `records_to_list` turns a host copy into the
reference's List[bytes] when a caller needs it.  `encode_shares_many` is the
list form: the wires of a tensor list's share rows (make_shares_vec_many's
blocks), each the tensors' records back to back, in three launches.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

from . import _native, field

EXPORTS = ("dn_m521_codec_scratch_bytes", "dn_m521_encoded_capacity", "dn_m521_encode_shares",
           "dn_m521_decode_shares", "dn_m521_encode_many_scratch_bytes", "dn_m521_encode_shares_many")


def _lib():
    L = _native.lib()
    if not getattr(L, "_dn_codec_bound", False):  # argtypes, once per loaded library
        vp, u64, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
        L.dn_m521_codec_scratch_bytes.restype = u64
        L.dn_m521_codec_scratch_bytes.argtypes = [u64]
        L.dn_m521_encoded_capacity.restype = u64
        L.dn_m521_encoded_capacity.argtypes = [u64, u64]
        L.dn_m521_encode_shares.restype = i32
        L.dn_m521_encode_shares.argtypes = [vp, u64, u64, vp, vp, u64, vp, u64, vp]
        L.dn_m521_decode_shares.restype = i32
        L.dn_m521_decode_shares.argtypes = [vp, u64, vp, u64, vp, vp, vp, vp]
        if hasattr(L, "dn_m521_encode_shares_many"):  # (an A/B baseline built from an older revision lacks these)
            L.dn_m521_encode_many_scratch_bytes.restype = u64
            L.dn_m521_encode_many_scratch_bytes.argtypes = [u64, u64, u64]
            L.dn_m521_encode_shares_many.restype = i32
            L.dn_m521_encode_shares_many.argtypes = [ctypes.POINTER(u64), ctypes.POINTER(vp), ctypes.POINTER(u64), u64,
                                                     ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(u64),
                                                     ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(u64), u64,
                                                     vp, vp, u64, vp]
        L._dn_codec_bound = True
    return L


_scratch_cache = {}  # (device index, stream) -> uint8 scratch tensor (grown on demand)


def _scratch(dev, nbytes: int):
    """Encoder scratch, cached per device and stream (the kernels of one stream
    run in order, so one buffer serves every call queued on it)."""
    import torch

    key = (dev.index, _native.stream_ptr())
    buf = _scratch_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        _scratch_cache[key] = buf
    return buf


def _out(t, numel: int, dtype, dev, what: str):
    import torch

    if t is None:
        return torch.empty(numel, dtype=dtype, device=dev)
    if not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == dev and t.is_contiguous()
            and t.numel() >= numel):
        raise ValueError(f"{what}: expected a contiguous {dtype} tensor of >= {numel} elements on {dev}")
    return t


def encode_share_vec(vec, n: int, x: int, *, trim: bool = True, out=None, offsets=None):
    """Share x of n elements (uint8 device tensor, tiled) -> (packed uint8, offsets int64[n+1]).
    out / offsets: caller buffers (>= encoded_capacity(n, x) bytes, 4-byte aligned; >= n + 1 entries), else allocated.
    trim=True cuts `packed` to its length (one read-back of offsets[n])."""
    import torch

    if not 0 <= x < (1 << 64):
        raise NotImplementedError("encode_share_vec: x must fit 64 bits")
    L = _lib()
    dev = vec.device
    cap = int(L.dn_m521_encoded_capacity(n, x))
    out = _out(out, max(cap, 1), torch.uint8, dev, "encode_share_vec out")
    if out.data_ptr() & 3:
        raise ValueError("encode_share_vec out: the buffer must be 4-byte aligned (the encoder stores dwords)")
    # every entry is written by the encoder (offsets[n] by the last element)
    if n:
        offsets = _out(offsets, n + 1, torch.int64, dev, "encode_share_vec offsets")[: n + 1]
    else:
        offsets = _out(offsets, 1, torch.int64, dev, "encode_share_vec offsets")[:1]
        offsets.zero_()
    sb = int(L.dn_m521_codec_scratch_bytes(n))
    scratch = _scratch(dev, sb)
    _native.check(L.dn_m521_encode_shares(vec.data_ptr(), n, x, offsets.data_ptr(), out.data_ptr(), cap,
                                          scratch.data_ptr(), sb, _native.stream_ptr()))
    if trim:
        out = out[: int(offsets[n].item())]
    return out, offsets


def _check_block(what: str, k: int, b, vb: int, S, dev) -> int:
    """Block k of encode_shares_many against its form (contiguous uint8 [S, vb]
    or [vb]) and, from the second block on, block 0's S and device: its S."""
    import torch

    if not (isinstance(b, torch.Tensor) and b.dtype == torch.uint8 and b.dim() in (1, 2) and b.is_contiguous()
            and b.shape[-1] == vb):
        raise ValueError(f"{what}: block {k} must be a contiguous uint8 tensor [S, {vb}] or [{vb}]")
    s_k = b.shape[0] if b.dim() == 2 else 1
    if S is not None and (s_k != S or b.device != dev):
        raise ValueError(f"{what}: block {k} has {s_k} rows on {b.device}, block 0 has {S} on {dev}")
    return s_k


def encode_shares_many(blocks, ns: Sequence[int], xs: Optional[Sequence[int]] = None, *,
                       rows: Optional[Sequence[int]] = None, trim: bool = True, outs=None, offsets=None
                       ) -> List[Tuple[object, object]]:
    """The wires of a tensor list's share rows in one pass: for each x the
    records of every tensor back to back, in element order — record e of the
    concatenation is the reference's `_share_to_bytes((x, y_e))`
    (shamir.py:28-33), as in `encode_share_vec` on each (tensor, row),
    concatenated, with one offsets[n_total + 1].  Three launches instead of
    three per tensor and row (dn_m521_encode_shares_many).

    blocks   sequence of contiguous uint8 device tensors, blocks[k] of shape
             [S, vec_bytes(ns[k])] (what make_shares_vec_many returns: share x
             at row x - 1) or 1-D [vec_bytes(ns[k])] (S = 1); one S, one device
    ns       the tensors' element counts (n_total = sum(ns))
    xs       the abscissas to encode, each below 2^64; default 1..S
    rows     the block row behind each x; default x - 1.  (A row under an
             abscissa that is not its index + 1: a sum_shares_vec result.)
    outs, offsets  optional caller buffers per x: outs[i] a uint8 device tensor
             of >= encoded_capacity(n_total, xs[i]) bytes, 4-byte aligned (a
             16-byte aligned one takes the wide store path); offsets[i] int64,
             >= n_total + 1 entries.  Default: allocated
    trim     True cuts every `packed` to its length with ONE read-back for all
             wires; False returns the full-capacity tensors without
             synchronising (the length is offsets[n_total])
    Returns one (packed, offsets[: n_total + 1]) per x.  Such a wire is the
    wire of one n_total-element vector to `decode_share_vec` and
    `SecretShare.resolve_records_vec`, whose result the caller splits by `ns`.
    Argument errors are raised before any device use; n_total == 0 gives empty
    wires with offsets == [0]."""
    import torch

    what = "encode_shares_many"
    blocks, ns = list(blocks), [int(n) for n in ns]
    if len(blocks) != len(ns):
        raise ValueError(f"{what}: {len(blocks)} blocks for {len(ns)} sizes")
    if ns and min(ns) < 0:
        raise ValueError(f"{what}: negative element count")
    # One walk over the list (a model's hundred tensors; the device idles
    # meanwhile): a block that is not exactly the first block's form —
    # the same dimension, S, device — is looked at again by _check_block.
    S = dev = form = None
    u8, tile_bytes = torch.uint8, field.TILE_BYTES
    ptrs, pitches, tiles = [], [], 0
    for k, (b, n) in enumerate(zip(blocks, ns)):
        nt = (n + 255) >> 8  # field.TILE = 256
        vb = nt * tile_bytes
        if form is None:
            S = _check_block(what, k, b, vb, None, None)
            dev, form = b.device, b.dim()
        elif not (type(b) is torch.Tensor and b.shape == ((S, vb) if form == 2 else (vb,)) and b.dtype == u8
                  and b.is_contiguous() and b.device == dev):
            _check_block(what, k, b, vb, S, dev)
        ptrs.append(b.data_ptr())
        pitches.append(vb)
        tiles += nt
    if xs is None:
        if rows is not None:
            raise ValueError(f"{what}: rows without xs")
        xs = range(1, (S or 0) + 1)
    xs = [int(x) for x in xs]
    if any(not 0 <= x < (1 << 64) for x in xs):
        raise NotImplementedError(f"{what}: x must fit 64 bits")
    rows = [x - 1 for x in xs] if rows is None else [int(r) for r in rows]
    if len(rows) != len(xs):
        raise ValueError(f"{what}: {len(rows)} rows for {len(xs)} abscissas")
    if S is not None and any(not 0 <= r < S for r in rows):
        raise ValueError(f"{what}: rows must lie in [0, {S}): the blocks have {S} share rows")
    for name, bufs in (("outs", outs), ("offsets", offsets)):
        if bufs is not None and len(bufs) != len(xs):
            raise ValueError(f"{what}: {len(bufs)} {name} for {len(xs)} abscissas")
    if not xs:
        return []
    n_total = sum(ns)
    if dev is None or dev.type != "cuda":
        if dev is not None:
            raise ValueError(f"{what}: the blocks must be on a HIP device (they are on {dev})")
        dev = _native.require_device()
    L = _lib()
    if not hasattr(L, "dn_m521_encode_shares_many"):
        raise RuntimeError(f"{_native.lib_path()} lacks dn_m521_encode_shares_many: rebuild the native library")
    m = len(xs)
    caps = [int(L.dn_m521_encoded_capacity(n_total, x)) for x in xs]
    packed, offs = [], []
    for i in range(m):
        o = _out(None if outs is None else outs[i], max(caps[i], 1), torch.uint8, dev, f"{what} outs[{i}]")
        if o.data_ptr() & 3:
            raise ValueError(f"{what} outs[{i}]: the buffer must be 4-byte aligned (the encoder stores dwords)")
        packed.append(o)
        # every entry is written by the encoder (offsets[n_total] by the list's last element)
        offs.append(_out(None if offsets is None else offsets[i], n_total + 1, torch.int64, dev,
                         f"{what} offsets[{i}]")[: n_total + 1])
    if n_total == 0:
        for o in offs:
            o.zero_()
        return [(p[:0] if trim else p, o) for p, o in zip(packed, offs)]
    nseg = len(ns)
    sb = int(L.dn_m521_encode_many_scratch_bytes(nseg, tiles, m))
    scratch = _scratch(dev, sb)
    totals = torch.empty(m, dtype=torch.int64, device=dev)
    u64s, vps = ctypes.c_uint64 * nseg, ctypes.c_void_p * nseg
    wu64, wvp = ctypes.c_uint64 * m, ctypes.c_void_p * m
    _native.check(L.dn_m521_encode_shares_many(
        u64s(*ns), vps(*ptrs), u64s(*pitches), nseg,
        (ctypes.c_uint32 * m)(*rows), wu64(*xs), wvp(*[o.data_ptr() for o in offs]),
        wvp(*[p.data_ptr() for p in packed]), wu64(*caps), m, totals.data_ptr(), scratch.data_ptr(), sb,
        _native.stream_ptr()))
    if trim:
        packed = [p[:t] for p, t in zip(packed, totals.tolist())]  # one read-back for all wires
    return list(zip(packed, offs))


def encoded_capacity(n: int, x: int) -> int:
    """Bytes the encoder may write for n records of share x (an `out` buffer's size)."""
    return int(_lib().dn_m521_encoded_capacity(n, x))


_flags = {}  # (device index, stream) -> int32 bad-record counter of the checked form


def decode_share_vec(packed, offsets, n: int, *, out=None, xs=None, bad=None):
    """(packed, offsets[n+1]) -> (tiled uint8 vector of y mod p, uint64 xs as int64 tensor).

    out / xs: caller buffers (>= vec_bytes(n) bytes, >= n entries), else allocated.
    A `packed` view that is not 4-byte aligned is copied once (the kernels load dwords).
    bad=None: the call checks for records it cannot represent (x > 8 bytes,
    y > 68 bytes) with one read-back and raises ValueError.  bad=<int32 device
    tensor>: the count of such records is ADDED to it on the device and the
    call does not synchronise — the caller checks it once, at its next sync
    (`check_bad(bad)`), over any number of decodes."""
    import torch

    L = _lib()
    dev = packed.device
    if packed.data_ptr() & 3:  # the decoder loads dwords: one aligned device copy of a misaligned view
        packed = packed.clone()
    vec = _out(out, field.vec_bytes(n), torch.uint8, dev, "decode_share_vec out")
    xs = _out(xs, max(n, 1), torch.int64, dev, "decode_share_vec xs")
    checked = bad is None
    if checked:
        key = (dev.index, _native.stream_ptr())
        bad = _flags.get(key)
        if bad is None:
            bad = _flags[key] = torch.zeros(1, dtype=torch.int32, device=dev)
        else:
            bad.zero_()
    elif not (isinstance(bad, torch.Tensor) and bad.dtype == torch.int32 and bad.device == dev):
        raise ValueError("decode_share_vec: bad must be an int32 tensor on the packed records' device")
    _native.check(L.dn_m521_decode_shares(packed.data_ptr(), packed.numel(), offsets.data_ptr(), n, vec.data_ptr(),
                                          xs.data_ptr(), bad.data_ptr(), _native.stream_ptr()))
    if checked:
        check_bad(bad)
    return vec, xs[:n]


def check_bad(bad) -> None:
    """Raise if a deferred decode (decode_share_vec(..., bad=flag)) met records
    it cannot represent (one read-back)."""
    nbad = int(bad.item())
    if nbad:
        raise ValueError(f"decode_share_vec: {nbad} records with x > 8 bytes or y > 68 bytes")


def check_bad_records(bad, what: str = "resolve_records_vec") -> None:
    """Raise if a deferred `SecretShare.resolve_records_vec(..., bad=flag)` (or
    `sum_records_vec`: what="sum_records_vec" names it in the message) met
    records it cannot represent (flag[0]) or records whose x is not their
    wire's abscissa (flag[1]): one read-back of the two counts."""
    nbad, nmis = (int(c) for c in bad.tolist())
    if nbad or nmis:
        raise ValueError(f"{what}: {nbad} records with x > 8 bytes or y > 68 bytes, "
                         f"{nmis} records whose x is not their wire's abscissa")


def records_to_list(packed_host, offsets_host) -> List[bytes]:
    """Host copy -> the reference's List[bytes] (one record per element)."""
    buf = bytes(packed_host.numpy() if hasattr(packed_host, "numpy") else packed_host)
    off = offsets_host.tolist()
    return [buf[off[i]:off[i + 1]] for i in range(len(off) - 1)]
