"""The vector API's argument rules: what each call raises, and in which order.

One table, no device and no launch: `_native.require_device` answers
torch.device("cpu") and every `_native` launch function is replaced by one
that raises `Launched`, so a row that got past its checks fails.  A row is
(id, call); EXPECT holds its exception type and its exact, whole message.

* one row per check of the public vector methods that had no host row
  (make_shares_vec, make_shares_vec_prng, make_shares_vec_many,
  resolve_shares_vec, sum_shares_vec, encode_share_vec, decode_share_vec);
* precedence rows ("a>b"): for consecutive checks a, b of a method's source
  order, one call that violates both and must raise a's message — for the
  methods above and for resolve_shares_vec_many, resolve_records_vec,
  sum_records_vec, encode_share_frame, encode_shares_many, encode_frames_many,
  open_frames and the sum bindings.  Pairs that no call can violate together
  (an empty list and a wrong member of it; k == 1 and a duplicate) have no row;
* the "lacks dn_...: rebuild the native library" error of every optional entry
  point, against a library that hides it.

The expectations were taken from the package as it stood before the rules were
gathered in crypto/shamir/_args.py and the ctypes tables; the table passes
unchanged against either.  The last tests read the package's source: each rule's
message is written in one place, each dn_* symbol bound in one table.
"""
import ctypes
import glob
import os
import re

import pytest
import torch

from delta_node.crypto import shamir
from delta_node.crypto.aes import aes
from delta_node.crypto.shamir import _native, codec, field
from delta_node.utils import _mask_native, mimc7

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "delta-node_amd", "delta_node")

N = 4
VB = field.vec_bytes(N)  # one tile: 16896
U8, I32, I64 = torch.uint8, torch.int32, torch.int64
M127 = (1 << 127) - 1

LAUNCHES = ("split_u64", "split_fe", "split_prng", "mt_split_device", "mt_split_many_device",
            "mt_draw_coeffs_device", "reconstruct", "reconstruct_many", "reconstruct_records", "sum_vecs",
            "sum_records")
REAL = {name: getattr(_native, name) for name in LAUNCHES}  # the bindings' own count checks are rows too


class Launched(Exception):
    pass


def launched(*args, **kwargs):
    raise Launched


def S(t=3, **kw):
    return shamir.SecretShare(t, **kw)


def vals(n=N, dtype=I64):
    return torch.zeros(n, dtype=dtype)


def blk(rows=5, vb=VB, dtype=U8, **kw):
    return torch.zeros((rows, vb), dtype=dtype, **kw)


def vec(vb=VB, dtype=U8, **kw):
    return torch.zeros(vb, dtype=dtype, **kw)


def strided(numel, dtype=U8):
    return torch.zeros(2 * numel, dtype=dtype)[::2]


def skewed(numel, by=1):
    """A contiguous uint8 view whose address is `by` past a 64-byte boundary."""
    buf = torch.zeros(numel + 128, dtype=U8)
    return buf[(-buf.data_ptr()) % 64 + by:][:numel]


def wires(m, n=N, **kw):
    return [(torch.zeros(8 * n, dtype=U8, **kw), torch.zeros(n + 1, dtype=I64, **kw)) for _ in range(m)]


def wire(packed=None, offsets=None, n=N):
    p, o = wires(1, n)[0]
    return (p if packed is None else packed, o if offsets is None else offsets)


def frames(m, numel=64, **kw):
    return [torch.zeros(numel, dtype=U8, **kw) for _ in range(m)]


def flag(numel=2, dtype=I32, **kw):
    return torch.zeros(numel, dtype=dtype, **kw)


CAP = 1 << 10  # more than encoded_capacity(4, x) and frame_capacity(4, x) for any 64-bit x

ROWS = [
    # ---- make_shares_vec: m521, threshold, limits, values, out, coeffs
    ("msv m521", lambda: S(prime=M127).make_shares_vec(vals(), 5)),
    ("msv threshold", lambda: S(3).make_shares_vec(vals(), 2)),
    ("msv shares limit", lambda: S(3).make_shares_vec(vals(), 65536)),
    ("msv threshold limit", lambda: S(65).make_shares_vec(vals(), 70)),
    ("msv values", lambda: S(3).make_shares_vec(vals(dtype=torch.float32), 5)),
    ("msv out shape", lambda: S(3).make_shares_vec(vals(), 5, out=blk(4))),
    ("msv out dtype", lambda: S(3).make_shares_vec(vals(), 5, out=blk(dtype=torch.int8))),
    ("msv out strided", lambda: S(3).make_shares_vec(vals(), 5, out=blk(vb=2 * VB)[:, ::2])),
    ("msv out device", lambda: S(3).make_shares_vec(vals(), 5, out=blk(device="meta"))),
    ("msv out n=0", lambda: S(3).make_shares_vec(vals(0), 5, out=blk())),
    ("msv coeffs", lambda: S(3).make_shares_vec(vals(), 5, out=blk(), coeffs=blk(3))),
    ("msv m521>threshold", lambda: S(3, prime=M127).make_shares_vec(vals(), 2)),
    ("msv threshold>limits", lambda: S(70).make_shares_vec(vals(), 5)),
    ("msv limits>values", lambda: S(3).make_shares_vec(vals(dtype=torch.float32), 70000)),
    ("msv values>out", lambda: S(3).make_shares_vec(vals(dtype=torch.float32), 5, out=blk(4))),
    ("msv out>coeffs", lambda: S(3).make_shares_vec(vals(), 5, out=blk(4), coeffs=blk(3))),
    # ---- make_shares_vec_prng: m521, threshold, limits (threshold 8), values, out
    ("prng m521", lambda: S(prime=M127).make_shares_vec_prng(vals(), 5)),
    ("prng threshold", lambda: S(3).make_shares_vec_prng(vals(), 2)),
    ("prng shares limit", lambda: S(3).make_shares_vec_prng(vals(), 65536)),
    ("prng threshold limit", lambda: S(9).make_shares_vec_prng(vals(), 10)),
    ("prng values", lambda: S(3).make_shares_vec_prng(vals(dtype=torch.float64), 5)),
    ("prng out", lambda: S(3).make_shares_vec_prng(vals(), 5, out=blk(5, VB + 1))),
    ("prng out n=0", lambda: S(3).make_shares_vec_prng(vals(0), 5, out=blk())),
    ("prng m521>threshold", lambda: S(3, prime=M127).make_shares_vec_prng(vals(), 2)),
    ("prng threshold>limits", lambda: S(9).make_shares_vec_prng(vals(), 5)),
    ("prng limits>values", lambda: S(3).make_shares_vec_prng(vals(dtype=torch.float64), 70000)),
    ("prng values>out", lambda: S(3).make_shares_vec_prng(vals(dtype=torch.float64), 5, out=blk(4))),
    # ---- make_shares_vec_many: m521, threshold, limits, values, outs count, out
    ("many m521", lambda: S(prime=M127).make_shares_vec_many([vals()], 5)),
    ("many threshold", lambda: S(3).make_shares_vec_many([vals()], 2)),
    ("many shares limit", lambda: S(3).make_shares_vec_many([vals()], 65536)),
    ("many threshold limit", lambda: S(65).make_shares_vec_many([vals()], 70)),
    ("many values", lambda: S(3).make_shares_vec_many([vals(), vals(dtype=torch.float32)], 5, outs=[blk(), blk()])),
    ("many outs count", lambda: S(3).make_shares_vec_many([vals(), vals()], 5, outs=[blk()])),
    ("many out", lambda: S(3).make_shares_vec_many([vals(), vals(300)], 5, outs=[blk(), blk()])),
    ("many out n=0", lambda: S(3).make_shares_vec_many([vals(0)], 5, outs=[blk()])),
    ("many out dtype", lambda: S(3).make_shares_vec_many([vals()], 5, outs=[blk(dtype=torch.int8)])),
    ("many out device", lambda: S(3).make_shares_vec_many([vals()], 5, outs=[blk(device="meta")])),
    ("many m521>threshold", lambda: S(3, prime=M127).make_shares_vec_many([vals()], 2)),
    ("many threshold>limits", lambda: S(70).make_shares_vec_many([vals()], 5)),
    ("many limits>values", lambda: S(3).make_shares_vec_many([vals(dtype=torch.float32)], 70000)),
    ("many values>outs count", lambda: S(3).make_shares_vec_many([vals(dtype=torch.float32)], 5, outs=[])),
    ("many outs count>out", lambda: S(3).make_shares_vec_many([vals(), vals()], 5, outs=[blk(4)])),
    ("many first wrong out", lambda: S(3).make_shares_vec_many([vals(), vals(300), vals()], 5,
                                                                outs=[blk(), blk(4, 2 * VB), blk(3)])),
    # ---- resolve_shares_vec: m521, count, empty, few, distinct, k == 1, vectors, out
    ("rsv m521", lambda: S(prime=M127).resolve_shares_vec(blk(3), [1, 2, 3], N)),
    ("rsv count", lambda: S(3).resolve_shares_vec(blk(3), [1, 2], N)),
    ("rsv empty", lambda: S(3).resolve_shares_vec([], [], N)),
    ("rsv few", lambda: S(3).resolve_shares_vec(blk(2), [1, 2], N)),
    ("rsv distinct", lambda: S(3).resolve_shares_vec(blk(3), [1, 2, 1], N)),
    ("rsv k=1", lambda: S(1).resolve_shares_vec(blk(1), [1], N)),
    ("rsv vectors size", lambda: S(3).resolve_shares_vec([vec(), vec(), vec(VB - 1)], [1, 2, 3], N)),
    ("rsv vectors dtype", lambda: S(3).resolve_shares_vec(blk(3, dtype=torch.int8), [1, 2, 3], N)),
    ("rsv vectors strided", lambda: S(3).resolve_shares_vec([vec(), strided(VB), vec()], [1, 2, 3], N)),
    ("rsv vectors device", lambda: S(3).resolve_shares_vec(blk(3, device="meta"), [1, 2, 3], N)),
    ("rsv vectors n=0", lambda: S(3).resolve_shares_vec(blk(3), [1, 2, 3], 0)),
    ("rsv out", lambda: S(3).resolve_shares_vec(blk(3), [1, 2, 3], N, out="int32")),
    ("rsv m521>count", lambda: S(prime=M127).resolve_shares_vec(blk(3), [1, 2], N)),
    ("rsv count>empty", lambda: S(3).resolve_shares_vec(blk(1), [], N)),
    ("rsv few>distinct", lambda: S(3).resolve_shares_vec(blk(2), [1, 1], N)),
    ("rsv distinct>vectors", lambda: S(3).resolve_shares_vec(blk(3, VB + 1), [1, 2, 1], N)),
    ("rsv k=1>vectors", lambda: S(1).resolve_shares_vec(blk(1, VB + 1), [1], N)),
    ("rsv vectors>out", lambda: S(3).resolve_shares_vec(blk(3, VB + 1), [1, 2, 3], N, out="int32")),
    # ---- resolve_shares_vec_many
    ("rsvm m521>entries", lambda: S(prime=M127).resolve_shares_vec_many([blk(3)], [1, 2, 3], [N, N])),
    ("rsvm entries>count", lambda: S(3).resolve_shares_vec_many([blk(2)], [1, 2, 3], [N, N])),
    ("rsvm count>empty", lambda: S(3).resolve_shares_vec_many([blk(1)], [], [N])),
    ("rsvm empty", lambda: S(3).resolve_shares_vec_many([[]], [], [N])),
    ("rsvm few>distinct", lambda: S(3).resolve_shares_vec_many([blk(2)], [1, 1], [N])),
    ("rsvm distinct>out form", lambda: S(3).resolve_shares_vec_many([blk(3)], [1, 2, 1], [N], out="int32")),
    ("rsvm k=1>out form", lambda: S(1).resolve_shares_vec_many([blk(1)], [1], [N], out="int32")),
    ("rsvm out form>rows", lambda: S(3).resolve_shares_vec_many([blk(3, VB + 1)], [1, 2, 3], [N], out="int32")),
    ("rsvm rows>outs count", lambda: S(3).resolve_shares_vec_many([blk(3, VB + 1)], [1, 2, 3], [N], outs=[])),
    ("rsvm vectors>outs count", lambda: S(3).resolve_shares_vec_many([[vec(), vec(), vec(VB + 1)]], [1, 2, 3], [N],
                                                                      outs=[])),
    ("rsvm outs count>out", lambda: S(3).resolve_shares_vec_many([blk(3), blk(3)], [1, 2, 3], [N, N],
                                                                  outs=[vals(N + 1)])),
    ("rsvm out int64", lambda: S(3).resolve_shares_vec_many([blk(3)], [1, 2, 3], [N], outs=[vals(N + 1)])),
    ("rsvm out field", lambda: S(3).resolve_shares_vec_many([blk(3)], [1, 2, 3], [N], out="field", outs=[vals()])),
    # ---- resolve_records_vec
    ("rrv m521>pairs", lambda: S(prime=M127).resolve_records_vec([(vec(8),)] * 3, [1, 2, 3], N)),
    ("rrv pairs>count", lambda: S(3).resolve_records_vec([(vec(8),)] * 3, [1, 2], N)),
    ("rrv count>few", lambda: S(3).resolve_records_vec(wires(2), [1], N)),
    ("rrv few>distinct", lambda: S(3).resolve_records_vec(wires(2), [1, 1], N)),
    ("rrv distinct>out form", lambda: S(3).resolve_records_vec(wires(3), [1, 2, 1], N, out="int32")),
    ("rrv k=1>out form", lambda: S(1).resolve_records_vec(wires(1), [1], N, out="int32")),
    ("rrv no wires>out form", lambda: S(3).resolve_records_vec([], None, N, out="int32")),
    ("rrv out form>n", lambda: S(3).resolve_records_vec(wires(3), [1, 2, 3], -1, out="int32")),
    ("rrv n>packed", lambda: S(3).resolve_records_vec(wires(2) + [wire(packed=vec(32, torch.int8))], [1, 2, 3], -1)),
    ("rrv packed>offsets", lambda: S(3).resolve_records_vec(
        wires(2) + [wire(packed=vec(32, torch.int8), offsets=vals(N + 1, I32))], [1, 2, 3], N)),
    ("rrv offsets>device", lambda: S(3).resolve_records_vec(
        wires(2) + [wire(offsets=torch.zeros(N + 1, dtype=I32, device="meta"))], [1, 2, 3], N)),
    ("rrv device>entries", lambda: S(3).resolve_records_vec(
        wires(2) + [wire(offsets=torch.zeros(N, dtype=I64, device="meta"))], [1, 2, 3], N)),
    ("rrv first wrong wire", lambda: S(3).resolve_records_vec(
        [wire(), wire(offsets=vals(N)), wire(packed=vec(32, torch.int8))], [1, 2, 3], N)),
    ("rrv entries>bad", lambda: S(3).resolve_records_vec(wires(2) + [wire(offsets=vals(N))], [1, 2, 3], N,
                                                         bad=flag(1))),
    ("rrv bad>first record", lambda: S(3).resolve_records_vec(wires(3, n=0), None, 0, bad=flag(1))),
    ("rrv first record>device", lambda: S(3).resolve_records_vec(wires(3, n=0, device="meta"), None, 0)),
    ("rrv device>readable", lambda: S(3).resolve_records_vec(wires(3, device="meta"), None, N)),
    ("rrv readable", lambda: S(3).resolve_records_vec(wires(3), None, N)),
    ("rrv read xs distinct", lambda: S(2).resolve_records_vec(
        [wire(offsets=torch.tensor([0, 8, 16, 24, 32]))] * 2, None, N)),
    # ---- sum_shares_vec
    ("ssv m521>no blocks", lambda: S(prime=M127).sum_shares_vec([])),
    ("ssv no blocks", lambda: S(3).sum_shares_vec([])),
    ("ssv dtype>shape", lambda: S(3).sum_shares_vec([vec(), vec(2 * VB, torch.int8)])),
    ("ssv shape>contiguous", lambda: S(3).sum_shares_vec([vec(), strided(2 * VB)])),
    ("ssv contiguous>tiles", lambda: S(3).sum_shares_vec([strided(100), strided(100)])),
    ("ssv first wrong block", lambda: S(3).sum_shares_vec([vec(), strided(VB), vec(dtype=torch.int8)])),
    ("ssv tiles>signs count", lambda: S(3).sum_shares_vec([vec(100), vec(100)], signs=[1])),
    ("ssv signs count>signs", lambda: S(3).sum_shares_vec([vec(), vec()], signs=[True])),
    ("ssv signs>out", lambda: S(3).sum_shares_vec([vec(), vec()], signs=[1, 1.0], out=vec(VB + 1))),
    ("ssv out>device", lambda: S(3).sum_shares_vec([vec(device="meta")] * 2, out=vec())),
    ("ssv device", lambda: S(3).sum_shares_vec([vec(device="meta")] * 2, signs=[1, -1], out=vec(device="meta"))),
    # ---- sum_records_vec
    ("srv m521>pairs", lambda: S(prime=M127).sum_records_vec([(vec(8),)], 1, N)),
    ("srv pairs>n", lambda: S(3).sum_records_vec([(vec(8),)], 1, -1)),
    ("srv no records>n", lambda: S(3).sum_records_vec([], 1, -1)),
    ("srv n>packed", lambda: S(3).sum_records_vec([wire(packed=vec(32, torch.int8))], 1, -1)),
    ("srv packed>offsets", lambda: S(3).sum_records_vec([wire(packed=strided(32), offsets=strided(N + 1, I64))], 1, N)),
    ("srv offsets>device", lambda: S(3).sum_records_vec(
        wires(1) + [wire(offsets=torch.zeros(N + 1, dtype=I32, device="meta"))], 1, N)),
    ("srv device>entries", lambda: S(3).sum_records_vec(
        wires(1) + [wire(offsets=torch.zeros(N, dtype=I64, device="meta"))], 1, N)),
    ("srv entries>x integer", lambda: S(3).sum_records_vec([wire(offsets=vals(N))], True, N)),
    ("srv x integer>signs count", lambda: S(3).sum_records_vec(wires(2), 1.0, N, signs=[1])),
    ("srv x fits>signs count", lambda: S(3).sum_records_vec(wires(2), 1 << 64, N, signs=[1])),
    ("srv first record>signs count", lambda: S(3).sum_records_vec(wires(2, n=0), None, 0, signs=[1])),
    ("srv signs count>signs", lambda: S(3).sum_records_vec(wires(2), 1, N, signs=[0])),
    ("srv signs>acc", lambda: S(3).sum_records_vec(wires(2), 1, N, signs=[1, 2], acc=vec(VB + 1))),
    ("srv acc>out", lambda: S(3).sum_records_vec(wires(2), 1, N, acc=vec(VB + 1), out=vec(VB - 1))),
    ("srv out>bad", lambda: S(3).sum_records_vec(wires(2), 1, N, out=vec(VB - 1), bad=flag(3))),
    ("srv bad>device", lambda: S(3).sum_records_vec(wires(2, device="meta"), 1, N, bad=flag())),
    ("srv device>readable", lambda: S(3).sum_records_vec(wires(2, device="meta"), None, N)),
    ("srv readable", lambda: S(3).sum_records_vec(wires(2), None, N)),
    ("srv read xs differ", lambda: S(3).sum_records_vec(
        [wire(offsets=torch.tensor([0, 8, 16, 24, 32])),
         wire(packed=torch.tensor([1, 7] + [0] * 30, dtype=U8), offsets=torch.tensor([0, 8, 16, 24, 32]))], None, N)),
    # ---- the sum bindings' own counts
    ("sum_vecs flags", lambda: REAL["sum_vecs"]([4096, 8192, 12288], [True, False], 4096, 1)),
    ("sum_records flags>x", lambda: REAL["sum_records"]([(4096, 8, 8192)] * 3, 1 << 64, [True], None, None, n=1)),
    ("sum_records x", lambda: REAL["sum_records"]([(4096, 8, 8192)] * 3, -1, None, None, None, n=1)),
    ("reconstruct_records counts", lambda: REAL["reconstruct_records"]([(4096, 8, 8192)] * 3, [1, 2],
                                                                       _native.ones_weights(3), None, n=1)),
    # ---- encode_share_vec: x, out, alignment, offsets
    ("esv x", lambda: codec.encode_share_vec(vec(), N, 1 << 64)),
    ("esv out small", lambda: codec.encode_share_vec(vec(), N, 5, out=vec(8))),
    ("esv out dtype", lambda: codec.encode_share_vec(vec(), N, 5, out=vec(CAP, torch.int8))),
    ("esv out device", lambda: codec.encode_share_vec(vec(), N, 5, out=vec(CAP, device="meta"))),
    ("esv out n=0", lambda: codec.encode_share_vec(vec(0), 0, 5, out=vec(0))),
    ("esv aligned", lambda: codec.encode_share_vec(vec(), N, 5, out=skewed(CAP, 2))),
    ("esv offsets", lambda: codec.encode_share_vec(vec(), N, 5, out=vec(CAP), offsets=vals(N))),
    ("esv offsets n=0", lambda: codec.encode_share_vec(vec(0), 0, 5, out=vec(CAP), offsets=vals(0))),
    ("esv x>out", lambda: codec.encode_share_vec(vec(), N, -1, out=vec(8))),
    ("esv out>aligned", lambda: codec.encode_share_vec(vec(), N, 5, out=skewed(8, 1))),
    ("esv aligned>offsets", lambda: codec.encode_share_vec(vec(), N, 5, out=skewed(CAP, 3), offsets=vals(N))),
    # ---- decode_share_vec: out, xs, bad
    ("dsv out", lambda: codec.decode_share_vec(*wire(), N, out=vec(VB - 1))),
    ("dsv out n=0", lambda: codec.decode_share_vec(*wire(n=0), 0, out=vec(0, torch.int8))),
    ("dsv xs", lambda: codec.decode_share_vec(*wire(), N, out=vec(), xs=vals(N - 1))),
    ("dsv xs n=0", lambda: codec.decode_share_vec(*wire(n=0), 0, xs=vals(0))),
    ("dsv bad dtype", lambda: codec.decode_share_vec(*wire(), N, bad=flag(1, I64))),
    ("dsv bad device", lambda: codec.decode_share_vec(*wire(), N, bad=flag(1, device="meta"))),
    ("dsv bad list", lambda: codec.decode_share_vec(*wire(), N, bad=[0])),
    ("dsv out>xs", lambda: codec.decode_share_vec(*wire(), N, out=vec(VB - 1), xs=vals(N - 1))),
    ("dsv xs>bad", lambda: codec.decode_share_vec(*wire(), N, xs=vals(N - 1), bad=flag(1, I64))),
    # ---- encode_share_frame
    ("esf n>x", lambda: codec.encode_share_frame(vec(), -1, 1 << 64)),
    ("esf x>vec", lambda: codec.encode_share_frame(vec(VB - 1), N, -1)),
    ("esf vec>out", lambda: codec.encode_share_frame(vec(VB - 1), N, 5, out=vec(CAP, torch.int8))),
    ("esf out>offsets", lambda: codec.encode_share_frame(vec(), N, 5, out=strided(CAP), offsets=vals(N + 1, I32))),
    ("esf offsets>device", lambda: codec.encode_share_frame(vec(), N, 5, offsets=vals(N + 1, I32))),
    ("esf device", lambda: codec.encode_share_frame(vec(), N, 5, out=vec(8), offsets=vals(1))),
    # ---- open_frames
    ("of no frames>n", lambda: codec.open_frames([], -1, None)),
    ("of form>device", lambda: codec.open_frames([vec(64), vec(64, torch.int8, device="meta")], N, None)),
    ("of device>n", lambda: codec.open_frames([vec(64), vec(64, device="meta")], -1, None)),
    ("of n>xs count", lambda: codec.open_frames(frames(2), -1, [1])),
    ("of xs count>x", lambda: codec.open_frames(frames(2), N, [1 << 64])),
    ("of x>offsets count", lambda: codec.open_frames(frames(2), N, [1, -1], offsets=[vals(N + 1)])),
    ("of offsets count>offsets", lambda: codec.open_frames(frames(2), N, [1, 2], offsets=[vals(N + 1, I32)])),
    ("of offsets>bad", lambda: codec.open_frames(frames(2), N, [1, 2], offsets=[vals(N + 1), vals(N + 1, I32)],
                                                 bad=flag(1))),
    ("of bad>frame bytes", lambda: codec.open_frames(frames(2, 40), N, [1, 2], bad=flag(2, I64))),
    ("of frame bytes>entries", lambda: codec.open_frames([vec(40), vec(64)], N, [1, 2], offsets=[vals(N), vals(N)])),
    ("of entries>device", lambda: codec.open_frames(frames(2, device="meta"), N, [1, 2],
                                                    offsets=[torch.zeros(N, dtype=I64, device="meta")] * 2)),
    ("of device>header", lambda: codec.open_frames(frames(2, 16, device="meta"), None, None)),
    ("of header", lambda: codec.open_frames(frames(2, 16), None, None)),
    ("of header counts", lambda: codec.open_frames([torch.tensor([0] * 8 + [4] + [0] * 55, dtype=U8), vec(64)],
                                                   None, None)),
]

# encode_shares_many / encode_frames_many: one argument walk, two names
for _name, _f in (("esm", codec.encode_shares_many), ("efm", codec.encode_frames_many)):
    ROWS += [
        (f"{_name} count>negative", lambda f=_f: f([vec()], [N, -1])),
        (f"{_name} negative>block", lambda f=_f: f([vec(VB + 1), vec()], [N, -1])),
        (f"{_name} block>rows without xs", lambda f=_f: f([vec(VB + 1)], [N], rows=[0])),
        (f"{_name} first wrong block", lambda f=_f: f([blk(), blk(4), vec(VB + 1)], [N, N, N])),
        (f"{_name} rows without xs", lambda f=_f: f([blk()], [N], rows=[0], outs=[])),
        (f"{_name} x>rows count", lambda f=_f: f([blk()], [N], [1, 1 << 64], rows=[0])),
        (f"{_name} rows count>rows", lambda f=_f: f([blk()], [N], [1, 2], rows=[5])),
        (f"{_name} rows>outs count", lambda f=_f: f([blk()], [N], [1, 2], rows=[0, 5], outs=[])),
        (f"{_name} outs count>offsets count", lambda f=_f: f([blk()], [N], [1, 2], outs=[], offsets=[])),
        (f"{_name} offsets count>device", lambda f=_f: f([blk()], [N], [1, 2], offsets=[])),
        (f"{_name} device", lambda f=_f: f([blk(device="meta")], [N])),
        (f"{_name} out small>aligned", lambda f=_f: f([], [], [1], outs=[skewed(0, 1)])),
        (f"{_name} aligned>offsets", lambda f=_f: f([], [], [1], outs=[skewed(CAP, 4)[1:]], offsets=[vals(0)])),
        (f"{_name} offsets", lambda f=_f: f([], [], [1], outs=[skewed(CAP, 0)], offsets=[vals(1, I32)])),
    ]

EXPECT = {
    "msv m521": ("NotImplementedError", "the vector (GPU) path is GF(2^521 - 1) only; the byte API takes any prime"),
    "msv threshold": ("ValueError", "threshold should be little equal than shares"),
    "msv shares limit": ("NotImplementedError", "make_shares_vec: at most 65535 shares and threshold 64"),
    "msv threshold limit": ("NotImplementedError", "make_shares_vec: at most 65535 shares and threshold 64"),
    "msv values": ("TypeError", "make_shares_vec: values must be an int64 tensor"),
    "msv out shape": ("ValueError", "make_shares_vec: out must be contiguous uint8 [5, 16896] on cpu"),
    "msv out dtype": ("ValueError", "make_shares_vec: out must be contiguous uint8 [5, 16896] on cpu"),
    "msv out strided": ("ValueError", "make_shares_vec: out must be contiguous uint8 [5, 16896] on cpu"),
    "msv out device": ("ValueError", "make_shares_vec: out must be contiguous uint8 [5, 16896] on cpu"),
    "msv out n=0": ("ValueError", "make_shares_vec: out must be contiguous uint8 [5, 0] on cpu"),
    "msv coeffs": ("ValueError", "make_shares_vec: coeffs must be uint8 [2, 16896] on cpu"),
    "msv m521>threshold": ("NotImplementedError",
        "the vector (GPU) path is GF(2^521 - 1) only; the byte API takes any prime"),
    "msv threshold>limits": ("ValueError", "threshold should be little equal than shares"),
    "msv limits>values": ("NotImplementedError", "make_shares_vec: at most 65535 shares and threshold 64"),
    "msv values>out": ("TypeError", "make_shares_vec: values must be an int64 tensor"),
    "msv out>coeffs": ("ValueError", "make_shares_vec: out must be contiguous uint8 [5, 16896] on cpu"),
    "prng m521": ("NotImplementedError", "the vector (GPU) path is GF(2^521 - 1) only; the byte API takes any prime"),
    "prng threshold": ("ValueError", "threshold should be little equal than shares"),
    "prng shares limit": ("NotImplementedError", "make_shares_vec_prng: at most 65535 shares and threshold 8"),
    "prng threshold limit": ("NotImplementedError", "make_shares_vec_prng: at most 65535 shares and threshold 8"),
    "prng values": ("TypeError", "make_shares_vec_prng: values must be an int64 tensor"),
    "prng out": ("ValueError", "make_shares_vec_prng: out must be contiguous uint8 [5, 16896] on cpu"),
    "prng out n=0": ("ValueError", "make_shares_vec_prng: out must be contiguous uint8 [5, 0] on cpu"),
    "prng m521>threshold": ("NotImplementedError",
        "the vector (GPU) path is GF(2^521 - 1) only; the byte API takes any prime"),
    "prng threshold>limits": ("ValueError", "threshold should be little equal than shares"),
    "prng limits>values": ("NotImplementedError", "make_shares_vec_prng: at most 65535 shares and threshold 8"),
    "prng values>out": ("TypeError", "make_shares_vec_prng: values must be an int64 tensor"),
    "many m521": ("NotImplementedError", "the vector (GPU) path is GF(2^521 - 1) only; the byte API takes any prime"),
    "many threshold": ("ValueError", "threshold should be little equal than shares"),
    "many shares limit": ("NotImplementedError", "make_shares_vec_many: at most 65535 shares and threshold 64"),
    "many threshold limit": ("NotImplementedError", "make_shares_vec_many: at most 65535 shares and threshold 64"),
    "many values": ("TypeError", "make_shares_vec_many: values must be an int64 tensor"),
    "many outs count": ("ValueError", "make_shares_vec_many: 1 outs for 2 tensors"),
    "many out": ("ValueError", "make_shares_vec_many: out must be contiguous uint8 [5, 33792] on cpu"),
    "many out n=0": ("ValueError", "make_shares_vec_many: out must be contiguous uint8 [5, 0] on cpu"),
    "many out dtype": ("ValueError", "make_shares_vec_many: out must be contiguous uint8 [5, 16896] on cpu"),
    "many out device": ("ValueError", "make_shares_vec_many: out must be contiguous uint8 [5, 16896] on cpu"),
    "many m521>threshold": ("NotImplementedError",
        "the vector (GPU) path is GF(2^521 - 1) only; the byte API takes any prime"),
    "many threshold>limits": ("ValueError", "threshold should be little equal than shares"),
    "many limits>values": ("NotImplementedError", "make_shares_vec_many: at most 65535 shares and threshold 64"),
    "many values>outs count": ("TypeError", "make_shares_vec_many: values must be an int64 tensor"),
    "many outs count>out": ("ValueError", "make_shares_vec_many: 1 outs for 2 tensors"),
    "many first wrong out": ("ValueError", "make_shares_vec_many: out must be contiguous uint8 [5, 33792] on cpu"),
    "rsv m521": ("NotImplementedError", "the vector (GPU) path is GF(2^521 - 1) only; the byte API takes any prime"),
    "rsv count": ("ValueError", "resolve_shares_vec: one abscissa per share vector"),
    "rsv empty": ("ValueError", "not enough values to unpack (expected 2, got 0)"),
    "rsv few": ("ValueError", "need at least 3 shares"),
    "rsv distinct": ("ValueError", "shares must be distinct"),
    "rsv k=1": ("TypeError", "reduce() of empty iterable with no initial value"),
    "rsv vectors size": ("ValueError", "resolve_shares_vec: share vectors must be contiguous uint8 [16896] on cpu"),
    "rsv vectors dtype": ("ValueError", "resolve_shares_vec: share vectors must be contiguous uint8 [16896] on cpu"),
    "rsv vectors strided": ("ValueError", "resolve_shares_vec: share vectors must be contiguous uint8 [16896] on cpu"),
    "rsv vectors device": ("ValueError", "resolve_shares_vec: share vectors must be contiguous uint8 [16896] on cpu"),
    "rsv vectors n=0": ("ValueError", "resolve_shares_vec: share vectors must be contiguous uint8 [0] on cpu"),
    "rsv out": ("ValueError", "resolve_shares_vec: out must be \"int64\" or \"field\""),
    "rsv m521>count": ("NotImplementedError",
        "the vector (GPU) path is GF(2^521 - 1) only; the byte API takes any prime"),
    "rsv count>empty": ("ValueError", "resolve_shares_vec: one abscissa per share vector"),
    "rsv few>distinct": ("ValueError", "need at least 3 shares"),
    "rsv distinct>vectors": ("ValueError", "shares must be distinct"),
    "rsv k=1>vectors": ("TypeError", "reduce() of empty iterable with no initial value"),
    "rsv vectors>out": ("ValueError", "resolve_shares_vec: share vectors must be contiguous uint8 [16896] on cpu"),
    "rsvm m521>entries": ("NotImplementedError",
        "the vector (GPU) path is GF(2^521 - 1) only; the byte API takes any prime"),
    "rsvm entries>count": ("ValueError", "resolve_shares_vec_many: 1 share entries for 2 tensors"),
    "rsvm count>empty": ("ValueError", "resolve_shares_vec: one abscissa per share vector"),
    "rsvm empty": ("ValueError", "not enough values to unpack (expected 2, got 0)"),
    "rsvm few>distinct": ("ValueError", "need at least 3 shares"),
    "rsvm distinct>out form": ("ValueError", "shares must be distinct"),
    "rsvm k=1>out form": ("TypeError", "reduce() of empty iterable with no initial value"),
    "rsvm out form>rows": ("ValueError", "resolve_shares_vec_many: out must be \"int64\" or \"field\""),
    "rsvm rows>outs count": ("ValueError",
        "resolve_shares_vec_many: share rows must be contiguous uint8 [3, 16896] on cpu"),
    "rsvm vectors>outs count": ("ValueError",
        "resolve_shares_vec_many: share vectors must be contiguous uint8 [16896] on cpu"),
    "rsvm outs count>out": ("ValueError", "resolve_shares_vec_many: 1 outs for 2 tensors"),
    "rsvm out int64": ("ValueError", "resolve_shares_vec_many: out must be contiguous int64 [4] on cpu"),
    "rsvm out field": ("ValueError", "resolve_shares_vec_many: out must be contiguous field [16896] on cpu"),
    "rrv m521>pairs": ("NotImplementedError",
        "the vector (GPU) path is GF(2^521 - 1) only; the byte API takes any prime"),
    "rrv pairs>count": ("ValueError", "resolve_records_vec: records must be (packed, offsets) pairs"),
    "rrv count>few": ("ValueError", "resolve_records_vec: one abscissa per wire"),
    "rrv few>distinct": ("ValueError", "need at least 3 shares"),
    "rrv distinct>out form": ("ValueError", "shares must be distinct"),
    "rrv k=1>out form": ("TypeError", "reduce() of empty iterable with no initial value"),
    "rrv no wires>out form": ("ValueError", "not enough values to unpack (expected 2, got 0)"),
    "rrv out form>n": ("ValueError", "resolve_records_vec: out must be \"int64\" or \"field\""),
    "rrv n>packed": ("ValueError", "resolve_records_vec: n must not be negative"),
    "rrv packed>offsets": ("ValueError", "resolve_records_vec: packed records must be contiguous 1-D uint8 tensors"),
    "rrv offsets>device": ("ValueError", "resolve_records_vec: offsets must be contiguous 1-D int64 tensors"),
    "rrv device>entries": ("ValueError", "resolve_records_vec: every wire's records and offsets must be on one device"),
    "rrv first wrong wire": ("ValueError", "resolve_records_vec: offsets must hold n + 1 = 5 entries, got 4"),
    "rrv entries>bad": ("ValueError", "resolve_records_vec: offsets must hold n + 1 = 5 entries, got 4"),
    "rrv bad>first record": ("ValueError",
        "resolve_records_vec: bad must be a contiguous int32 tensor [2] on the records' device"),
    "rrv first record>device": ("ValueError",
        "resolve_records_vec: xs=None needs a first record to read each abscissa from"),
    "rrv device>readable": ("ValueError", "resolve_records_vec: records must be on cpu"),
    "rrv readable": ("ValueError", "resolve_records_vec: the first record of wire 0 has no readable x"),
    "rrv read xs distinct": ("ValueError", "shares must be distinct"),
    "ssv m521>no blocks": ("NotImplementedError",
        "the vector (GPU) path is GF(2^521 - 1) only; the byte API takes any prime"),
    "ssv no blocks": ("ValueError", "sum_shares_vec: no blocks"),
    "ssv dtype>shape": ("ValueError", "sum_shares_vec: blocks must be uint8 tensors"),
    "ssv shape>contiguous": ("ValueError",
        "sum_shares_vec: blocks must share one shape and device, got (33792,) on cpu next to (16896,) on cpu"),
    "ssv contiguous>tiles": ("ValueError", "sum_shares_vec: blocks must be contiguous"),
    "ssv first wrong block": ("ValueError", "sum_shares_vec: blocks must be contiguous"),
    "ssv tiles>signs count": ("ValueError", "sum_shares_vec: blocks must be whole 16896-byte tiles, got 100 bytes"),
    "ssv signs count>signs": ("ValueError", "sum_shares_vec: 1 signs for 2 blocks"),
    "ssv signs>out": ("ValueError", "sum_shares_vec: signs must be +1 or -1"),
    "ssv out>device": ("ValueError", "sum_shares_vec: out must be contiguous uint8 (16896,) on meta"),
    "ssv device": ("ValueError", "sum_shares_vec: blocks must be on cpu"),
    "srv m521>pairs": ("NotImplementedError",
        "the vector (GPU) path is GF(2^521 - 1) only; the byte API takes any prime"),
    "srv pairs>n": ("ValueError", "sum_records_vec: records must be (packed, offsets) pairs"),
    "srv no records>n": ("ValueError", "sum_records_vec: no records"),
    "srv n>packed": ("ValueError", "sum_records_vec: n must not be negative"),
    "srv packed>offsets": ("ValueError", "sum_records_vec: packed records must be contiguous 1-D uint8 tensors"),
    "srv offsets>device": ("ValueError", "sum_records_vec: offsets must be contiguous 1-D int64 tensors"),
    "srv device>entries": ("ValueError", "sum_records_vec: every wire's records and offsets must be on one device"),
    "srv entries>x integer": ("ValueError", "sum_records_vec: offsets must hold n + 1 = 5 entries, got 4"),
    "srv x integer>signs count": ("ValueError", "sum_records_vec: x must be an integer or None"),
    "srv x fits>signs count": ("ValueError", "sum_records_vec: x must fit 64 bits"),
    "srv first record>signs count": ("ValueError",
        "sum_records_vec: x=None needs a first record to read the abscissa from"),
    "srv signs count>signs": ("ValueError", "sum_records_vec: 1 signs for 2 wires"),
    "srv signs>acc": ("ValueError", "sum_records_vec: signs must be +1 or -1"),
    "srv acc>out": ("ValueError",
        "sum_records_vec: acc must be a contiguous uint8 tensor [16896] on the records' device"),
    "srv out>bad": ("ValueError",
        "sum_records_vec: out must be a contiguous uint8 tensor [16896] on the records' device"),
    "srv bad>device": ("ValueError",
        "sum_records_vec: bad must be a contiguous int32 tensor [2] on the records' device"),
    "srv device>readable": ("ValueError", "sum_records_vec: records must be on cpu"),
    "srv readable": ("ValueError", "sum_records_vec: the first record of wire 0 has no readable x"),
    "srv read xs differ": ("ValueError", "sum_records_vec: the wires' first records carry different abscissas: [0, 7]"),
    "sum_vecs flags": ("ValueError", "sum_vecs: one negate flag per input"),
    "sum_records flags>x": ("ValueError", "sum_records: one negate flag per wire"),
    "sum_records x": ("ValueError", "sum_records: x must fit 64 bits"),
    "reconstruct_records counts": ("ValueError", "reconstruct_records: one wire and one abscissa per weight"),
    "esv x": ("NotImplementedError", "encode_share_vec: x must fit 64 bits"),
    "esv out small": ("ValueError",
        "encode_share_vec out: expected a contiguous torch.uint8 tensor of >= 272 elements on cpu"),
    "esv out dtype": ("ValueError",
        "encode_share_vec out: expected a contiguous torch.uint8 tensor of >= 272 elements on cpu"),
    "esv out device": ("ValueError",
        "encode_share_vec out: expected a contiguous torch.uint8 tensor of >= 272 elements on cpu"),
    "esv out n=0": ("ValueError",
        "encode_share_vec out: expected a contiguous torch.uint8 tensor of >= 1 elements on cpu"),
    "esv aligned": ("ValueError",
        "encode_share_vec out: the buffer must be 4-byte aligned (the encoder stores dwords)"),
    "esv offsets": ("ValueError",
        "encode_share_vec offsets: expected a contiguous torch.int64 tensor of >= 5 elements on cpu"),
    "esv offsets n=0": ("ValueError",
        "encode_share_vec offsets: expected a contiguous torch.int64 tensor of >= 1 elements on cpu"),
    "esv x>out": ("NotImplementedError", "encode_share_vec: x must fit 64 bits"),
    "esv out>aligned": ("ValueError",
        "encode_share_vec out: expected a contiguous torch.uint8 tensor of >= 272 elements on cpu"),
    "esv aligned>offsets": ("ValueError",
        "encode_share_vec out: the buffer must be 4-byte aligned (the encoder stores dwords)"),
    "dsv out": ("ValueError",
        "decode_share_vec out: expected a contiguous torch.uint8 tensor of >= 16896 elements on cpu"),
    "dsv out n=0": ("ValueError",
        "decode_share_vec out: expected a contiguous torch.uint8 tensor of >= 0 elements on cpu"),
    "dsv xs": ("ValueError", "decode_share_vec xs: expected a contiguous torch.int64 tensor of >= 4 elements on cpu"),
    "dsv xs n=0": ("ValueError",
        "decode_share_vec xs: expected a contiguous torch.int64 tensor of >= 1 elements on cpu"),
    "dsv bad dtype": ("ValueError", "decode_share_vec: bad must be an int32 tensor on the packed records' device"),
    "dsv bad device": ("ValueError", "decode_share_vec: bad must be an int32 tensor on the packed records' device"),
    "dsv bad list": ("ValueError", "decode_share_vec: bad must be an int32 tensor on the packed records' device"),
    "dsv out>xs": ("ValueError",
        "decode_share_vec out: expected a contiguous torch.uint8 tensor of >= 16896 elements on cpu"),
    "dsv xs>bad": ("ValueError",
        "decode_share_vec xs: expected a contiguous torch.int64 tensor of >= 4 elements on cpu"),
    "esf n>x": ("ValueError", "encode_share_frame: n must not be negative"),
    "esf x>vec": ("NotImplementedError", "encode_share_frame: x must fit 64 bits"),
    "esf vec>out": ("ValueError", "encode_share_frame: vec must be a contiguous uint8 tensor of >= 16896 bytes"),
    "esf out>offsets": ("ValueError", "encode_share_frame out: expected a contiguous torch.uint8 tensor on cpu"),
    "esf offsets>device": ("ValueError", "encode_share_frame offsets: expected a contiguous torch.int64 tensor on cpu"),
    "esf device": ("ValueError", "encode_share_frame: vec must be on a HIP device (it is on cpu)"),
    "of no frames>n": ("ValueError", "open_frames: no frames"),
    "of form>device": ("ValueError", "open_frames: frames must be contiguous 1-D uint8 tensors"),
    "of device>n": ("ValueError", "open_frames: every frame must be on one device"),
    "of n>xs count": ("ValueError", "open_frames: n must not be negative"),
    "of xs count>x": ("ValueError", "open_frames: 1 abscissas for 2 frames"),
    "of x>offsets count": ("ValueError", "open_frames: x must fit 64 bits"),
    "of offsets count>offsets": ("ValueError", "open_frames: 1 offsets for 2 frames"),
    "of offsets>bad": ("ValueError", "open_frames: offsets must be contiguous 1-D int64 tensors on the frames' device"),
    "of bad>frame bytes": ("ValueError",
        "open_frames: bad must be a contiguous int32 tensor [2] on the frames' device"),
    "of frame bytes>entries": ("ValueError", "open_frames: frame 0 has 40 bytes, fewer than the 48 before its records"),
    "of entries>device": ("ValueError", "open_frames: offsets must hold n + 1 = 5 entries, got 4"),
    "of device>header": ("ValueError", "open_frames: frames must be on cpu"),
    "of header": ("ValueError", "open_frames: a frame is shorter than its 32-byte header"),
    "of header counts": ("ValueError", "open_frames: the frames' headers carry different record counts: [4, 0]"),
    "esm count>negative": ("ValueError", "encode_shares_many: 1 blocks for 2 sizes"),
    "esm negative>block": ("ValueError", "encode_shares_many: negative element count"),
    "esm block>rows without xs": ("ValueError",
        "encode_shares_many: block 0 must be a contiguous uint8 tensor [S, 16896] or [16896]"),
    "esm first wrong block": ("ValueError", "encode_shares_many: block 1 has 4 rows on cpu, block 0 has 5 on cpu"),
    "esm rows without xs": ("ValueError", "encode_shares_many: rows without xs"),
    "esm x>rows count": ("NotImplementedError", "encode_shares_many: x must fit 64 bits"),
    "esm rows count>rows": ("ValueError", "encode_shares_many: 1 rows for 2 abscissas"),
    "esm rows>outs count": ("ValueError", "encode_shares_many: rows must lie in [0, 5): the blocks have 5 share rows"),
    "esm outs count>offsets count": ("ValueError", "encode_shares_many: 0 outs for 2 abscissas"),
    "esm offsets count>device": ("ValueError", "encode_shares_many: 0 offsets for 2 abscissas"),
    "esm device": ("ValueError", "encode_shares_many: the blocks must be on a HIP device (they are on meta)"),
    "esm out small>aligned": ("ValueError",
        "encode_shares_many outs[0]: expected a contiguous torch.uint8 tensor of >= 1 elements on cpu"),
    "esm aligned>offsets": ("ValueError",
        "encode_shares_many outs[0]: the buffer must be 4-byte aligned (the encoder stores dwords)"),
    "esm offsets": ("ValueError",
        "encode_shares_many offsets[0]: expected a contiguous torch.int64 tensor of >= 1 elements on cpu"),
    "efm count>negative": ("ValueError", "encode_frames_many: 1 blocks for 2 sizes"),
    "efm negative>block": ("ValueError", "encode_frames_many: negative element count"),
    "efm block>rows without xs": ("ValueError",
        "encode_frames_many: block 0 must be a contiguous uint8 tensor [S, 16896] or [16896]"),
    "efm first wrong block": ("ValueError", "encode_frames_many: block 1 has 4 rows on cpu, block 0 has 5 on cpu"),
    "efm rows without xs": ("ValueError", "encode_frames_many: rows without xs"),
    "efm x>rows count": ("NotImplementedError", "encode_frames_many: x must fit 64 bits"),
    "efm rows count>rows": ("ValueError", "encode_frames_many: 1 rows for 2 abscissas"),
    "efm rows>outs count": ("ValueError", "encode_frames_many: rows must lie in [0, 5): the blocks have 5 share rows"),
    "efm outs count>offsets count": ("ValueError", "encode_frames_many: 0 outs for 2 abscissas"),
    "efm offsets count>device": ("ValueError", "encode_frames_many: 0 offsets for 2 abscissas"),
    "efm device": ("ValueError", "encode_frames_many: the blocks must be on a HIP device (they are on meta)"),
    "efm out small>aligned": ("ValueError",
        "encode_frames_many outs[0]: expected a contiguous torch.uint8 tensor of >= 32 elements on cpu"),
    "efm aligned>offsets": ("ValueError",
        "encode_frames_many outs[0]: the buffer must be 16-byte aligned (the lengths are stored as 16-byte "
        "words)"),
    "efm offsets": ("ValueError",
        "encode_frames_many offsets[0]: expected a contiguous torch.int64 tensor of >= 1 elements on cpu"),
}


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_native, "require_device", lambda: torch.device("cpu"))
    for name in LAUNCHES:
        monkeypatch.setattr(_native, name, launched)


def outcome(call):
    try:
        call()
    except Launched:
        return ("launched", "")
    except Exception as e:  # noqa: BLE001 - the table names the type it expects
        return (type(e).__name__, str(e))
    return ("returned", "")


def test_every_row_has_its_expectation():
    ids = [row[0] for row in ROWS]
    assert len(set(ids)) == len(ids)
    assert sorted(ids) == sorted(EXPECT)


def test_each_call_raises_its_first_failing_checks_message(no_device):
    got = {name: outcome(call) for name, call in ROWS}
    wrong = {name: (got[name], EXPECT[name]) for name in got if got[name] != EXPECT[name]}
    assert not wrong, wrong


# ------------------------------------------------------------------ optional entry points
class Without:
    """A loaded library as one built from an older revision shows it: without some symbols."""

    def __init__(self, lib, *hidden):
        self.__dict__.update(_lib=lib, _hidden=hidden)

    def __getattr__(self, name):
        if name in self._hidden:
            raise AttributeError(name)
        return getattr(self._lib, name)


OPTIONAL = [
    ("dn_m521_reconstruct_many", lambda: REAL["reconstruct_many"]([N], [4096] * 3, _native.ones_weights(3), "cpu")),
    ("dn_m521_sum_vecs", lambda: REAL["sum_vecs"]([4096, 8192], None, 4096, 1)),
    ("dn_m521_reconstruct_records", lambda: REAL["reconstruct_records"]([(4096, 8, 8192)] * 3, [1, 2, 3],
                                                                        _native.ones_weights(3), None, n=1)),
    ("dn_m521_sum_records", lambda: REAL["sum_records"]([(4096, 8, 8192)], 1, None, None, None, n=1)),
    ("dn_mt19937_split_many_device", lambda: REAL["mt_split_many_device"](None, None, [(N, 4096)], 3, 5)),
    ("dn_m521_encode_shares_many", lambda: codec.encode_shares_many([], [], [1])),
    ("dn_m521_frame_open", lambda: codec.frame_records_offset(N)),
    ("dn_m521_frame_open", lambda: codec.frame_capacity(N, 1)),
    ("dn_m521_frame_open", lambda: codec.encode_frames_many([], [], [1])),
    ("dn_m521_frame_open", lambda: codec.open_frames(frames(2), N, [1, 2])),
]


@pytest.mark.parametrize("symbol, call", OPTIONAL, ids=[f"{s}-{i}" for i, (s, _) in enumerate(OPTIONAL)])
def test_a_library_without_an_optional_entry_point_says_so(symbol, call, no_device, monkeypatch):
    old = Without(_native.lib(), symbol)
    monkeypatch.setattr(_native, "lib", lambda: old)
    monkeypatch.setenv("DN_SHAMIR_LIB", "/old/libdn_shamir.so")
    assert outcome(call) == ("RuntimeError", f"/old/libdn_shamir.so lacks {symbol}: rebuild the native library")


def test_a_library_without_the_optional_entry_points_still_binds(monkeypatch):
    optional = ("dn_m521_encode_many_scratch_bytes", "dn_m521_encode_shares_many", "dn_m521_frame_records_offset",
                "dn_m521_frame_capacity", "dn_m521_frame_finish", "dn_m521_frame_scratch_bytes", "dn_m521_frame_open")
    old = Without(_native.lib(), "_dn_codec_bound", *optional)  # (not bound yet, as a library just loaded)
    monkeypatch.setattr(_native, "lib", lambda: old)
    assert codec._lib() is old
    assert codec.encoded_capacity(N, 1) == int(_native.lib().dn_m521_encoded_capacity(N, 1)) > 0


def test_a_library_swapped_in_is_bound_again():
    with _native.library(_native.lib_path()) as other:
        assert other is not None and _native.lib() is other
        for get, name in ((codec._lib, "dn_m521_encoded_capacity"), (aes._lib, "dn_aes_encrypt_len"),
                          (_mask_native.lib, "dn_pcg64_advance"), (mimc7._lib, "dn_mimc7_hash")):
            assert get() is other
            assert getattr(other, name).argtypes, name
        assert other.dn_m521_vec_bytes.restype is ctypes.c_uint64
        assert codec.encoded_capacity(N, 1 << 63) > (1 << 5)  # (a 64-bit argument arrives whole)
    assert _native.lib() is not other


# ------------------------------------------------------------------ the device draws' state hand-over
class Stub:
    """The loaded library with some entry points replaced by Python functions."""

    def __init__(self, lib, **entry):
        self.__dict__.update(_lib=lib, **entry)

    def __getattr__(self, name):
        return getattr(self._lib, name)


class AsDevice:
    """A CPU tensor that answers is_cuda: what a binding looks at before it hands addresses on."""

    is_cuda = True

    def __init__(self, t):
        self.t = t

    def __getattr__(self, name):
        return getattr(self.t, name)


DRAWS = [
    ("dn_mt19937_draw_coeffs_device", lambda rng: REAL["mt_draw_coeffs_device"](rng, N, 2, AsDevice(blk(2)))),
    ("dn_mt19937_split_device", lambda rng: REAL["mt_split_device"](rng, AsDevice(vals()), AsDevice(blk()), N, 3, 5)),
    ("dn_mt19937_split_many_device", lambda rng: REAL["mt_split_many_device"](rng, AsDevice(vals()), [(N, 4096)], 3,
                                                                              5)),
]


@pytest.mark.parametrize("in_place", [True, False], ids=["in place", "marshalled"])
@pytest.mark.parametrize("symbol, draw", DRAWS, ids=[s for s, _ in DRAWS])
def test_a_device_draw_changes_the_generator_only_when_it_succeeds(symbol, draw, in_place, monkeypatch):
    """False (a retry code) and an exception leave `rng` as it was; success
    leaves it as the entry point wrote it — whether the state is taken in place
    or marshalled (an interpreter whose layout did not check out)."""
    import random

    if in_place:
        assert _native._mt_layout(), "this interpreter's random.Random layout was expected to check out"
    else:
        monkeypatch.setattr(_native, "_MT_LAYOUT", False)
    rc = [_native.DN_OK]

    def entry(state, index, *rest):
        if rc[0] == _native.DN_OK or not in_place:  # (the real entry points write the state only on success)
            ctypes.c_int32.from_address(index).value = 7
            ctypes.c_uint32.from_address(state).value = 0xC0FFEE
        return rc[0]

    stub = Stub(_native.lib(), dn_mt19937_split_supported=lambda *a: 1, dn_mt19937_split_many_supported=lambda *a: 1,
                dn_mt19937_device_scratch_bytes=lambda *a: 64, dn_mt19937_split_many_scratch_bytes=lambda *a: 64,
                **{symbol: entry})
    monkeypatch.setattr(_native, "lib", lambda: stub)
    monkeypatch.setattr(_native, "stream_ptr", lambda: 0)
    rng = random.Random(1234)
    before = rng.getstate()
    for code in (_native.DN_ERR_RETRY, _native.DN_ERR_UNSUPPORTED):
        rc[0] = code
        assert draw(rng) is False
        assert rng.getstate() == before
    rc[0] = _native.DN_ERR_HIP
    with pytest.raises(RuntimeError, match="^dn_shamir error -5"):
        draw(rng)
    assert rng.getstate() == before
    rc[0] = _native.DN_OK
    assert draw(rng) is True
    after = rng.getstate()
    assert (after[0], after[2]) == (before[0], before[2])
    assert after[1] == (0xC0FFEE,) + before[1][1:624] + (7,)


# ------------------------------------------------------------------ one definition
def _sources():
    out = {}
    for path in sorted(glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True)):
        with open(path) as f:
            out[os.path.relpath(path, PKG)] = f.read()
    return out


# (the signs rule as the template the Shamir methods share: utils/mask.py has a rule of its own in the same words)
@pytest.mark.parametrize("fragment", ["shares must be distinct", "packed records must be contiguous 1-D uint8",
                                      "{what}: signs must be +1 or -1", "bad must be a contiguous int32 tensor [2]",
                                      "lacks {name}: rebuild the native library", "must be 4-byte aligned"])
def test_each_rules_message_is_written_once(fragment):
    where = {f: text.count(fragment) for f, text in _sources().items() if fragment in text}
    assert len(where) == 1 and list(where.values()) == [1], (fragment, where)


def test_each_symbol_is_bound_in_one_table():
    bound = []
    for text in _sources().values():
        bound += re.findall(r'^    "(dn_\w+)": \(', text, flags=re.M)
    assert len(bound) == len(set(bound)), sorted(s for s in set(bound) if bound.count(s) > 1)
    assert sorted(bound) == sorted(_native.EXPORTS + codec.EXPORTS + aes.EXPORTS + _mask_native.EXPORTS
                                   + mimc7.EXPORTS)
    # ... and one statement assigns them
    assigns = {f: text.count(".argtypes") for f, text in _sources().items() if ".argtypes" in text}
    assert assigns == {os.path.join("crypto", "shamir", "_native.py"): 1}, assigns
