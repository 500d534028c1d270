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

A wire frame carries one wire and its record lengths in one buffer, so that
the offsets reach the receiver: `encode_share_frame` / `encode_frames_many`
encode straight into frames, `open_frames` turns received frames back into
(packed, offsets) with one validated scan, `frame_fields_host` parses a host
copy with numpy alone.

`commit_records_vec` / `verify_records_vec` are the commitment step of the
same path: SHA-256 of every record (the reference's `calc_commitment` per
share), computed or checked on the device in one launch.
"""
from __future__ import annotations

import ctypes
import threading
from typing import List, NamedTuple, Optional, Sequence, Tuple

from . import _args, _native, field

vp, u64, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
pvp, pu64 = ctypes.POINTER(vp), ctypes.POINTER(u64)
_SYMBOLS = {  # name -> (restype, argtypes, required), as _native._SYMBOLS
    "dn_m521_codec_scratch_bytes": (u64, [u64], True),
    "dn_m521_encoded_capacity": (u64, [u64, u64], True),
    "dn_m521_encode_shares": (i32, [vp, u64, u64, vp, vp, u64, vp, u64, vp], True),
    "dn_m521_decode_shares": (i32, [vp, u64, vp, u64, vp, vp, vp, vp], True),
    "dn_m521_encode_many_scratch_bytes": (u64, [u64, u64, u64], False),
    "dn_m521_encode_shares_many": (i32, [pu64, pvp, pu64, u64, ctypes.POINTER(ctypes.c_uint32), pu64, pvp, pvp, pu64,
                                         u64, vp, vp, u64, vp], False),
    "dn_m521_frame_records_offset": (u64, [u64], False),
    "dn_m521_frame_capacity": (u64, [u64, u64], False),
    "dn_m521_frame_finish": (i32, [pvp, pvp, pu64, u64, u64, vp], False),
    "dn_m521_frame_scratch_bytes": (u64, [u64, u64], False),
    "dn_m521_frame_open": (i32, [pvp, pu64, pu64, u64, u64, pvp, vp, vp, u64, vp], False),
    "dn_sha256_commit_records": (i32, [vp, u64, vp, u64, vp, vp, vp], False),
    "dn_sha256_verify_records": (i32, [vp, u64, vp, u64, vp, vp, vp, vp], False),
}
EXPORTS = tuple(_SYMBOLS)


def _lib():
    L = _native.lib()  # (the flag is looked at here: no further call once the library is bound)
    return L if getattr(L, "_dn_codec_bound", False) else _native.bind(L, _SYMBOLS, "_dn_codec_bound")


_tls = threading.local()  # per thread: .scratch, .flags (dicts keyed by (device index, stream))


def _cache(name: str) -> dict:
    cache = getattr(_tls, name, None)
    if cache is None:
        cache = {}
        setattr(_tls, name, cache)
    return cache


def _scratch(dev, nbytes: int):
    """Encoder scratch, cached per thread, device and stream (grown on demand).
    The kernels of one stream run in order, so one buffer serves every call
    that ONE thread queues on it: a call's launches are queued back to back
    before the thread's next call starts.  Two threads on one stream are not
    ordered against each other — the entry points are entered with the GIL
    released, so their launches interleave — and a buffer they shared would
    carry one call's lengths, table or totals into the other's launches.
    Hence the thread in the key, as `_native._mt_scratch`."""
    import torch

    cache = _cache("scratch")
    key = (dev.index, _native.stream_ptr())
    buf = cache.get(key)
    if buf is None or buf.numel() < nbytes:
        cache[key] = buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    return buf


def _checked_flag(dev):
    """The zeroed int32 bad-record counter of decode_share_vec's checked form,
    cached per thread, device and stream: the call zeroes it, launches and
    reads it back, and another thread's zero or count must not fall between."""
    import torch

    cache = _cache("flags")
    key = (dev.index, _native.stream_ptr())
    bad = cache.get(key)
    if bad is None:
        bad = cache[key] = torch.zeros(1, dtype=torch.int32, device=dev)
    else:
        bad.zero_()
    return bad


def _out(t, numel: int, dtype, dev, what: str):
    import torch

    if t is None:
        return torch.empty(numel, dtype=dtype, device=dev)
    if not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == dev and t.is_contiguous()
            and t.numel() >= numel):
        raise ValueError(f"{what}: expected a contiguous {dtype} tensor of >= {numel} elements on {dev}")
    return t


def _wire_out(t, cap: int, dev, what: str):
    """A wire buffer: the caller's (>= cap bytes, 4-byte aligned) or a fresh one."""
    import torch

    t = _out(t, max(cap, 1), torch.uint8, dev, what)
    if t.data_ptr() & 3:
        raise ValueError(f"{what}: the buffer must be 4-byte aligned (the encoder stores dwords)")
    return t


def encode_share_vec(vec, n: int, x: int, *, trim: bool = True, out=None, offsets=None):
    """Share x of n elements (uint8 device tensor, tiled) -> (packed uint8, offsets int64[n+1]).
    out / offsets: caller buffers (>= encoded_capacity(n, x) bytes, 4-byte aligned; >= n + 1 entries), else allocated.
    trim=True cuts `packed` to its length (one read-back of offsets[n])."""
    import torch

    if not _args.fits_u64(x):
        raise NotImplementedError("encode_share_vec: x must fit 64 bits")
    L = _lib()
    dev = vec.device
    cap = int(L.dn_m521_encoded_capacity(n, x))
    out = _wire_out(out, cap, dev, "encode_share_vec out")
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
    return _encode_list("encode_shares_many", lambda: _native.need(_lib(), "dn_m521_encode_shares_many"), False,
                        blocks, ns, xs, rows, trim, outs, offsets)


def _encode_list(what: str, library, framed: bool, blocks, ns, xs, rows, trim: bool, outs, offsets):
    """encode_shares_many (framed=False: wire i's records at the start of its
    buffer, a `_wire_out`) and encode_frames_many (framed=True: at R(n_total)
    of a `_frame_out`, then one finish launch for all wires)."""
    import torch

    ns, ptrs, pitches, tiles, xs, rows, dev = _many_args(what, blocks, ns, xs, rows, outs, offsets)
    if not xs:
        return []
    n_total = sum(ns)
    dev = _many_device(what, dev)
    L = library()
    m = len(xs)
    R = int(L.dn_m521_frame_records_offset(n_total)) if framed else 0
    caps = [int(L.dn_m521_encoded_capacity(n_total, x)) for x in xs]
    buffer = _frame_out if framed else _wire_out
    bufs, offs = [], []
    for i in range(m):
        bufs.append(buffer(None if outs is None else outs[i], R + caps[i], dev, f"{what} outs[{i}]"))
        # every entry is written by the encoder (offsets[n_total] by the list's last element)
        offs.append(_out(None if offsets is None else offsets[i], n_total + 1, torch.int64, dev,
                         f"{what} offsets[{i}]")[: n_total + 1])
    totals = None
    if n_total:
        totals = _encode_many(L, ns, ptrs, pitches, tiles, xs, rows, [b[R:] for b in bufs] if framed else bufs, offs,
                              caps, dev)
    else:
        for o in offs:
            o.zero_()
    if framed:
        _finish(L, offs, bufs, xs, n_total)
    if trim:
        lens = totals.tolist() if totals is not None else [0] * m  # one read-back for all wires
        bufs = [b[: R + t] for b, t in zip(bufs, lens)]
    return list(zip(bufs, offs))


def _many_args(what: str, blocks, ns, xs, rows, outs, offsets):
    """The argument rules of encode_shares_many (and encode_frames_many), no
    device use: (ns, block addresses, pitches, tiles, xs, rows, the blocks'
    device or None for an empty list)."""
    import torch

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
    if not all(_args.fits_u64(x) for x in xs):
        raise NotImplementedError(f"{what}: x must fit 64 bits")
    rows = [x - 1 for x in xs] if rows is None else [int(r) for r in rows]
    if len(rows) != len(xs):
        raise ValueError(f"{what}: {len(rows)} rows for {len(xs)} abscissas")
    if S is not None and any(not 0 <= r < S for r in rows):
        raise ValueError(f"{what}: rows must lie in [0, {S}): the blocks have {S} share rows")
    for name, bufs in (("outs", outs), ("offsets", offsets)):
        if bufs is not None and len(bufs) != len(xs):
            raise ValueError(f"{what}: {len(bufs)} {name} for {len(xs)} abscissas")
    return ns, ptrs, pitches, tiles, xs, rows, dev


def _many_device(what: str, dev):
    """The device of a tensor list's blocks (the current one for an empty list)."""
    if dev is None or dev.type != "cuda":
        if dev is not None:
            raise ValueError(f"{what}: the blocks must be on a HIP device (they are on {dev})")
        dev = _native.require_device()
    return dev


def _encode_many(L, ns, ptrs, pitches, tiles, xs, rows, packed, offs, caps, dev):
    """dn_m521_encode_shares_many over validated arguments (n_total > 0): wire
    i into packed[i] / offs[i]; returns the device int64[m] of the wires' lengths."""
    import torch

    nseg, m = len(ns), len(xs)
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
    return totals


def encoded_capacity(n: int, x: int) -> int:
    """Bytes the encoder may write for n records of share x (an `out` buffer's size)."""
    return int(_lib().dn_m521_encoded_capacity(n, x))


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
        bad = _checked_flag(dev)
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


# ------------------------------------------------------------------ share commitments
# utils.calc_commitment (utils/commitment.py:5-12) of every record of a wire,
# as the reference's runner computes it per share before sealing it
# (runner/horizontal/agg.py:160-162) and checks it on receipt
# (runner/horizontal/agg.py:257-272, coord/horizontal/agg.py:309-318, 342-348).
DIGEST_BYTES = 32


def _commit_args(what: str, packed, offsets, n: int, bad):
    """The wire and the flag of commit_records_vec / verify_records_vec, no device use: (n, the wire's device)."""
    n = int(n)
    if n < 0:
        raise ValueError(f"{what}: n must not be negative")
    dev = _args.check_wires(what, [(packed, offsets)], n)
    _args.check_bad_flag(what, bad, dev, "records")
    return n, dev


def _overlaps(a, b) -> bool:
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a.numel() > 0 and b.numel() > 0 and a0 < b0 + b.numel() * b.element_size() \
        and b0 < a0 + a.numel() * a.element_size()


def _commit_device(what: str, dev):
    got = _native.require_device()
    if dev != got:
        raise ValueError(f"{what}: records must be on {got}")
    return got


def commit_records_vec(packed, offsets, n: int, *, out=None, bad=None):
    """SHA-256 of every record of a wire -> uint8 device tensor [n, 32]: row e
    is `utils.calc_commitment(packed[offsets[e]:offsets[e + 1]])`, bit for bit,
    in one launch (dn_sha256_commit_records) — the commitments of
    `upload_secret_shares` for a whole share vector, between the encode and
    `aes.encrypt_vec`.

    packed, offsets  a wire as `encode_share_vec` / `encode_shares_many` return
             it, or the record view frame[R(n):] of a frame with its offsets
             (on the sender's side, or out of `open_frames`): contiguous 1-D
             uint8 / int64 device tensors, n + 1 offsets.  A `packed` view that
             is not 4-byte aligned is copied once
    out      optional contiguous uint8 device tensor of >= 32 n bytes, 4-byte
             aligned (a 16-byte aligned one is stored as 16-byte words), not
             overlapping `packed`; bytes past 32 n are left alone
    bad      None: one read-back after the launch, and ValueError naming the
             count of records whose offsets leave their window (decreasing,
             below their wave's first offset, past its last or past `packed`).
             An int32 device tensor [2]: that count is ADDED to bad[0] and the
             call does not synchronise; such a record's digest is 32 zero
             bytes; `check_bad_commit(bad, what="commit_records_vec")` raises later
    An empty record is hashed as b"".  Argument errors are raised before any
    device use; n = 0 returns an empty [0, 32] tensor."""
    import torch

    what = "commit_records_vec"
    n, first = _commit_args(what, packed, offsets, n, bad)
    if out is not None:
        out = _wire_out(out, DIGEST_BYTES * n, first, f"{what} out")
        if _overlaps(out, packed):
            raise ValueError(f"{what}: out overlaps packed")
    dev = _commit_device(what, first)
    if out is None:
        out = torch.empty(DIGEST_BYTES * n, dtype=torch.uint8, device=dev)
    res = out.view(-1)[: DIGEST_BYTES * n].view(n, DIGEST_BYTES)
    if n == 0:
        return res
    L = _native.need(_lib(), "dn_sha256_commit_records")
    bad, checked = _args.bad_flag(bad, dev)
    recs, ((p, nbytes, o),) = _args.aligned_wires([(packed, offsets)])
    _native.check(L.dn_sha256_commit_records(p, nbytes, o, n, out.data_ptr(), bad.data_ptr(), _native.stream_ptr()))
    if checked:
        check_bad_commit(bad, what=what)
    return res


def verify_records_vec(packed, offsets, n: int, commitments, *, ok=None, bad=None) -> None:
    """Check every record of a wire against its commitment, in one launch
    (dn_sha256_verify_records): record e passes if
    `commitments[e] == utils.calc_commitment(packed[offsets[e]:offsets[e + 1]])`
    — the check of `get_secret_shares` and of the coordinator for a whole
    share vector, between `open_frames` and `resolve_records_vec` /
    `sum_records_vec`.

    packed, offsets  as in `commit_records_vec`
    commitments  contiguous uint8 tensor on the wire's device holding 32 n
             bytes, as [n, 32] (what commit_records_vec returns) or flat
    ok       optional contiguous uint8 device tensor of >= n entries, not
             overlapping `packed`: ok[e] = 1 where record e passes, else 0
    bad      None: one read-back after the launch, and ValueError naming the
             records whose offsets leave their window and the records whose
             SHA-256 is not their commitment (where the reference drops the
             share).  An int32 device tensor [2]: the two counts are ADDED to
             it and the call does not synchronise;
             `check_bad_commit(bad)` raises later
    Argument errors are raised before any device use."""
    import torch

    what = "verify_records_vec"
    n, first = _commit_args(what, packed, offsets, n, bad)
    c = commitments
    if not (isinstance(c, torch.Tensor) and c.dtype == torch.uint8 and c.is_contiguous() and c.device == first
            and tuple(c.shape) in ((n, DIGEST_BYTES), (DIGEST_BYTES * n,))):
        raise ValueError(f"{what}: commitments must be a contiguous uint8 tensor [{n}, {DIGEST_BYTES}] or "
                         f"[{DIGEST_BYTES * n}] on the records' device")
    if ok is not None:
        ok = _out(ok, n, torch.uint8, first, f"{what} ok")
        if _overlaps(ok, packed):
            raise ValueError(f"{what}: ok overlaps packed")
    dev = _commit_device(what, first)
    if n == 0:
        return
    L = _native.need(_lib(), "dn_sha256_verify_records")
    bad, checked = _args.bad_flag(bad, dev)
    if c.data_ptr() & 3:  # the kernel loads dwords: one aligned device copy of a misaligned view
        c = c.clone()
    recs, ((p, nbytes, o),) = _args.aligned_wires([(packed, offsets)])
    _native.check(L.dn_sha256_verify_records(p, nbytes, o, n, c.data_ptr(), None if ok is None else ok.data_ptr(),
                                             bad.data_ptr(), _native.stream_ptr()))
    if checked:
        check_bad_commit(bad, what=what)


def check_bad_commit(bad, what: str = "verify_records_vec") -> None:
    """Raise if a deferred `verify_records_vec(..., bad=flag)` (or
    `commit_records_vec`: what="commit_records_vec") met records whose offsets
    leave their window (flag[0]) or records whose SHA-256 is not their
    commitment (flag[1]): one read-back of the two counts."""
    nbad, nmis = (int(c) for c in bad.tolist())
    if nbad or nmis:
        raise ValueError(f"{what}: {nbad} records whose offsets leave their window, "
                         f"{nmis} records whose SHA-256 is not their commitment")


# ------------------------------------------------------------------ wire frames
# One wire and its record lengths in one buffer (include/dn_shamir.h, "Share
# wire frames"):
#     [magic "DNSHREC1"][n u64][x u64][records_bytes u64][lens u8[n], zero-padded to 16][records]
FRAME_MAGIC = b"DNSHREC1"
FRAME_HEADER = 32


def _frame_lib():
    return _native.need(_lib(), "dn_m521_frame_open")


def frame_records_offset(n: int) -> int:
    """R(n) = 32 + 16 * ceil(n / 16): where the records of an n-record frame start."""
    return int(_frame_lib().dn_m521_frame_records_offset(n))


def frame_capacity(n: int, x: int) -> int:
    """Bytes a frame of n records of share x may take: R(n) + encoded_capacity(n, x)."""
    return int(_frame_lib().dn_m521_frame_capacity(n, x))


def _frame_out(t, cap: int, dev, what: str):
    """A frame buffer: the caller's (>= cap bytes, 16-byte aligned) or a fresh one."""
    import torch

    t = _out(t, cap, torch.uint8, dev, what)
    if t.data_ptr() & 15:
        raise ValueError(f"{what}: the buffer must be 16-byte aligned (the lengths are stored as 16-byte words)")
    return t


def _finish(L, offs, frames, xs, n: int) -> None:
    m = len(frames)
    vps = ctypes.c_void_p * m
    _native.check(L.dn_m521_frame_finish(vps(*[o.data_ptr() for o in offs]), vps(*[f.data_ptr() for f in frames]),
                                         (ctypes.c_uint64 * m)(*xs), m, n, _native.stream_ptr()))


def encode_share_frame(vec, n: int, x: int, *, trim: bool = True, out=None, offsets=None):
    """Share x of n elements (uint8 device tensor, tiled) -> (frame uint8, offsets int64[n+1]).

    `encode_share_vec` with its output inside a wire frame: the encoder writes
    the records at frame[R(n):] (R = frame_records_offset; nothing is copied),
    then one launch writes the lengths, the pad and the header
    (dn_m521_frame_finish).  The frame is what goes to `aes.encrypt_vec`;
    frame[R(n):] with `offsets` is a wire as it stands.
    out / offsets: caller buffers (>= frame_capacity(n, x) bytes, 16-byte
    aligned; >= n + 1 entries), else allocated.  trim=True cuts the frame to
    its length R(n) + offsets[n] (one read-back); trim=False returns the
    full-capacity tensor without synchronising (the length is in the header).
    Argument errors are raised before any device use."""
    import torch

    what = "encode_share_frame"
    n, x = int(n), int(x)
    if n < 0:
        raise ValueError(f"{what}: n must not be negative")
    if not _args.fits_u64(x):
        raise NotImplementedError(f"{what}: x must fit 64 bits")
    vb = field.vec_bytes(n)
    if not (isinstance(vec, torch.Tensor) and vec.dtype == torch.uint8 and vec.is_contiguous() and vec.numel() >= vb):
        raise ValueError(f"{what}: vec must be a contiguous uint8 tensor of >= {vb} bytes")
    dev = vec.device
    for name, t, dtype in (("out", out, torch.uint8), ("offsets", offsets, torch.int64)):
        if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.is_contiguous()
                                  and t.device == dev):
            raise ValueError(f"{what} {name}: expected a contiguous {dtype} tensor on {dev}")
    if dev.type != "cuda":
        _native.require_device()
        raise ValueError(f"{what}: vec must be on a HIP device (it is on {dev})")
    L = _frame_lib()
    R = int(L.dn_m521_frame_records_offset(n))
    cap = int(L.dn_m521_encoded_capacity(n, x))
    frame = _frame_out(out, R + cap, dev, f"{what} out")
    offsets = _out(offsets, n + 1, torch.int64, dev, f"{what} offsets")[: n + 1]
    if n:  # every entry is written by the encoder (offsets[n] by the last element)
        sb = int(L.dn_m521_codec_scratch_bytes(n))
        scratch = _scratch(dev, sb)
        _native.check(L.dn_m521_encode_shares(vec.data_ptr(), n, x, offsets.data_ptr(), frame.data_ptr() + R, cap,
                                              scratch.data_ptr(), sb, _native.stream_ptr()))
    else:
        offsets.zero_()
    _finish(L, [offsets], [frame], [x], n)
    if trim:
        frame = frame[: R + int(offsets[n].item())]
    return frame, offsets


def encode_frames_many(blocks, ns: Sequence[int], xs: Optional[Sequence[int]] = None, *,
                       rows: Optional[Sequence[int]] = None, trim: bool = True, outs=None, offsets=None
                       ) -> List[Tuple[object, object]]:
    """`encode_shares_many` into wire frames: for each x one frame holding the
    records of every tensor back to back and their lengths — three encoder
    launches for the records (written at frame[R(n_total):], nothing copied)
    and ONE dn_m521_frame_finish launch for the lengths and headers of all
    wires.  Arguments and errors are encode_shares_many's, raised before any
    device use, except:
    outs     per x a uint8 device tensor of >= frame_capacity(n_total, xs[i])
             bytes, 16-byte aligned.  Default: allocated
    trim     True cuts every frame to R(n_total) + its records' bytes with ONE
             read-back for all wires; False returns the full-capacity tensors
             without synchronising
    Returns one (frame, offsets[: n_total + 1]) per x; frame[R(n_total):] with
    the offsets is the wire encode_shares_many returns.  n_total == 0 gives
    header-only frames."""
    return _encode_list("encode_frames_many", _frame_lib, True, blocks, ns, xs, rows, trim, outs, offsets)


def _headers(frames, what: str):
    """(n, x) of every frame's header: one read-back for all frames."""
    import torch

    if any(f.numel() < FRAME_HEADER for f in frames):
        raise ValueError(f"{what}: a frame is shorter than its {FRAME_HEADER}-byte header")
    host = torch.stack([f[:FRAME_HEADER] for f in frames]).cpu().numpy()
    words = host.view("<u8")  # [m, 4]: magic, n, x, records_bytes
    return [(int(w[1]), int(w[2])) for w in words]


def open_frames(frames, n: Optional[int], xs: Optional[Sequence[int]], *, offsets=None, bad=None
                ) -> List[Tuple[object, object]]:
    """Wire frames -> [(packed, offsets int64[n + 1])], what the record calls
    (`decode_share_vec`, `resolve_records_vec`, `sum_records_vec`) take: one
    validated scan of the lengths, batched over all frames of the call (three
    launches per 64 frames, dn_m521_frame_open).  `packed` is the view
    frame[R(n):]; nothing is copied.

    frames   sequence of contiguous 1-D uint8 device tensors (one device), each
             cut to its length — `aes.decrypt_vec`'s result.  A frame that is
             not 16-byte aligned is copied once, as decode_share_vec copies a
             misaligned `packed`
    n        records per frame (all frames of a call share it); None reads it
             from the headers
    xs       the abscissa each frame should carry; None reads them from the
             headers.  Either None costs one read-back for all frames
    offsets  optional per frame an int64 device tensor of >= n + 1 entries
    bad      None: one read-back after the launches, ValueError naming both
             counts if a header is not (magic, n, xs[i], len(frame) - R(n)) or
             a frame's lengths do not sum to len(frame) - R(n).  An int32
             device tensor [2]: the two counts are ADDED to it and the call
             does not synchronise; `check_bad_frames(bad)` raises later
    Whatever the bytes say, the offsets are monotone and inside `packed`
    (offsets[e] = min(prefix, len(packed))), so they are safe to hand on.
    Argument errors are raised before any device use."""
    import torch

    what = "open_frames"
    frames = list(frames)
    if not frames:
        raise ValueError(f"{what}: no frames")
    first = frames[0]
    for f in frames:
        if not (isinstance(f, torch.Tensor) and f.dtype == torch.uint8 and f.dim() == 1 and f.is_contiguous()):
            raise ValueError(f"{what}: frames must be contiguous 1-D uint8 tensors")
        if f.device != first.device:
            raise ValueError(f"{what}: every frame must be on one device")
    m = len(frames)
    if n is not None:
        n = int(n)
        if n < 0:
            raise ValueError(f"{what}: n must not be negative")
    if xs is not None:
        xs = [int(x) for x in xs]
        if len(xs) != m:
            raise ValueError(f"{what}: {len(xs)} abscissas for {m} frames")
        if not all(_args.fits_u64(x) for x in xs):
            raise ValueError(f"{what}: x must fit 64 bits")
    if offsets is not None:
        offsets = list(offsets)
        if len(offsets) != m:
            raise ValueError(f"{what}: {len(offsets)} offsets for {m} frames")
        for o in offsets:
            if not (isinstance(o, torch.Tensor) and o.dtype == torch.int64 and o.dim() == 1 and o.is_contiguous()
                    and o.device == first.device):
                raise ValueError(f"{what}: offsets must be contiguous 1-D int64 tensors on the frames' device")
    _args.check_bad_flag(what, bad, first.device, "frames")
    L = _frame_lib()

    def sizes(n: int) -> int:
        """R(n), once every frame and offsets buffer is known to hold n records."""
        R = int(L.dn_m521_frame_records_offset(n))
        for i, f in enumerate(frames):
            if f.numel() < R:
                raise ValueError(f"{what}: frame {i} has {f.numel()} bytes, fewer than the {R} before its records")
            if offsets is not None and offsets[i].numel() < n + 1:
                raise ValueError(f"{what}: offsets must hold n + 1 = {n + 1} entries, got {offsets[i].numel()}")
        return R

    if n is not None:
        sizes(n)
    dev = _native.require_device()
    if first.device != dev:
        raise ValueError(f"{what}: frames must be on {dev}")
    if n is None or xs is None:
        heads = _headers(frames, what)
        if n is None:
            if len({h[0] for h in heads}) != 1:
                raise ValueError(f"{what}: the frames' headers carry different record counts: {[h[0] for h in heads]}")
            n = heads[0][0]
        if xs is None:
            xs = [h[1] for h in heads]
    R = sizes(n)
    # the kernels load 16-byte words: one aligned device copy of a misaligned view
    frames = [f.clone() if f.data_ptr() & 15 else f for f in frames]
    offs = [_out(None if offsets is None else offsets[i], n + 1, torch.int64, dev, f"{what} offsets[{i}]")[: n + 1]
            for i in range(m)]
    bad, checked = _args.bad_flag(bad, dev)
    sb = int(L.dn_m521_frame_scratch_bytes(n, m))
    scratch = _scratch(dev, sb)
    vps, u64s = ctypes.c_void_p * m, ctypes.c_uint64 * m
    _native.check(L.dn_m521_frame_open(vps(*[f.data_ptr() for f in frames]), u64s(*[f.numel() for f in frames]),
                                       u64s(*xs), m, n, vps(*[o.data_ptr() for o in offs]), bad.data_ptr(),
                                       scratch.data_ptr(), sb, _native.stream_ptr()))
    if checked:
        check_bad_frames(bad)
    return [(f[R:], o) for f, o in zip(frames, offs)]


def open_frame(frame, n: Optional[int], x: Optional[int], *, offsets=None, bad=None):
    """`open_frames` for one frame: (packed, offsets)."""
    return open_frames([frame], n, None if x is None else [x], offsets=None if offsets is None else [offsets],
                       bad=bad)[0]


def check_bad_frames(bad) -> None:
    """Raise if a deferred `open_frames(..., bad=flag)` met frames whose header
    is not what the caller expects (flag[0]) or whose lengths do not sum to
    their records' bytes (flag[1]): one read-back of the two counts."""
    nhead, nsum = (int(c) for c in bad.tolist())
    if nhead or nsum:
        raise ValueError(f"open_frames: {nhead} frames whose header is not (magic, n, x, records_bytes), "
                         f"{nsum} frames whose lengths do not sum to their records' bytes")


class FrameFields(NamedTuple):
    n: int
    x: int
    records_bytes: int
    lens: object  # numpy uint8[n]
    records: object  # numpy uint8[records_bytes]


def frame_fields_host(buf, n: Optional[int] = None, x: Optional[int] = None) -> FrameFields:
    """A host copy of a frame (bytes, numpy uint8 or a CPU tensor) parsed with
    numpy alone — for peers without a GPU and for tests.  Raises ValueError on
    the faults the device counts: a wrong magic, a record count or abscissa
    other than the expected `n` / `x` (where given), a records_bytes that is
    not len(buf) - R(n), lengths that do not sum to it."""
    import numpy as np

    what = "frame_fields_host"
    if hasattr(buf, "numpy"):
        buf = buf.numpy()
    a = np.frombuffer(bytes(buf), dtype=np.uint8) if isinstance(buf, (bytes, bytearray, memoryview)) \
        else np.ascontiguousarray(buf, dtype=np.uint8).reshape(-1)
    if a.size < FRAME_HEADER:
        raise ValueError(f"{what}: {a.size} bytes, fewer than the {FRAME_HEADER}-byte header")
    if a[:8].tobytes() != FRAME_MAGIC:
        raise ValueError(f"{what}: wrong magic {a[:8].tobytes()!r}")
    hn, hx, hbytes = (int(v) for v in a[8:FRAME_HEADER].view("<u8"))
    if n is not None and hn != n:
        raise ValueError(f"{what}: the header carries n = {hn}, expected {n}")
    if x is not None and hx != x:
        raise ValueError(f"{what}: the header carries x = {hx}, expected {x}")
    R = FRAME_HEADER + ((hn + 15) & ~15)
    if a.size < R:
        raise ValueError(f"{what}: {a.size} bytes, fewer than the {R} before the records of n = {hn}")
    if hbytes != a.size - R:
        raise ValueError(f"{what}: the header carries records_bytes = {hbytes}, the buffer holds {a.size - R}")
    lens = a[FRAME_HEADER:FRAME_HEADER + hn]
    total = int(lens.sum(dtype=np.uint64))
    if total != hbytes:
        raise ValueError(f"{what}: the lengths sum to {total}, not records_bytes = {hbytes}")
    return FrameFields(hn, hx, hbytes, lens, a[R:])
