"""Shapes, predicates and exact expected values for the wire path — the share
envelope (csrc/aes_envelope.hip), the record codec (csrc/codec_m521.hip) and
the ChaCha counter of the PRNG split.  A helper for test_wire_edges_host.py,
test_gpu_aes_edges.py, test_gpu_codec_edges.py and test_gpu_prng.py (no tests,
no torch).

Every expectation comes from oracle/ (C AES, C ChaCha, py_shamir), Python's
base64 / bytes.fromhex, numpy or Python integers, never from the library under
test, and every comparison is bit for bit.  The unit arithmetic below restates
how the envelope kernels cut a message into thread units, so that a test can
assert the premise it needs (a full wave, a second grid-stride pass, a window
inside one aligned chunk) from the sizes it uses instead of trusting a
hard-coded number.
"""
from __future__ import annotations

import base64
import re
from typing import Callable, List, Sequence, Tuple

import numpy as np

from oracle import c_oracle

# ------------------------------------------------------------------ envelope: unit arithmetic
WAVE = 64
ENC_UNIT = 48          # message bytes (nonce || ciphertext) per encrypt unit
TEXT_UNIT = 64         # base64 characters per decrypt unit (128 hex digits)
GROUP = 1024           # threads of one envelope workgroup; one workgroup per CU


def enc_units(n: int) -> int:
    """Thread units of encrypt for n plaintext bytes: ceil((n + 16) / 48)."""
    return (n + 16 + ENC_UNIT - 1) // ENC_UNIT


def text_chars(n: int) -> int:
    """base64 characters of the envelope of n plaintext bytes."""
    return 4 * ((n + 16 + 2) // 3)


def text_units(n: int) -> int:
    """Thread units of decrypt: ceil(chars / 64)."""
    return (text_chars(n) + TEXT_UNIT - 1) // TEXT_UNIT


def text_len(n: int, hex_: bool) -> int:
    """Bytes of the text the kernels write / read (without "0x")."""
    return 2 * text_chars(n) if hex_ else text_chars(n)


def plain_capacity(n_text: int, hex_: bool) -> int:
    """Plaintext bytes a text of n_text bytes can hold at most; 0: not canonical by its length."""
    if hex_:
        if n_text & 1:
            return 0
        n_text //= 2
    if n_text < 24 or n_text & 3:
        return 0
    return n_text // 4 * 3 - 16


def n_for_units(u: int, ragged: int) -> int:
    """Plaintext length whose envelope has u units, the last holding `ragged`
    (1..48) of its 48 message bytes; 48 makes the last unit a whole one."""
    assert u >= 1 and 1 <= ragged <= ENC_UNIT
    n = ENC_UNIT * (u - 1) + ragged - 16
    assert n >= 0 and enc_units(n) == text_units(n) == u
    return n


def pad_chars(n: int) -> int:
    """'=' characters at the end of the envelope of n plaintext bytes."""
    return (3 - (n + 16) % 3) % 3


def enc_whole(n: int, g: int) -> bool:
    """encrypt_kernel's fast path: unit g holds 48 message bytes and no nonce byte."""
    return g != 0 and ENC_UNIT * (g + 1) <= n + 16


def enc_wave_full(n: int, k: int) -> bool:
    """Units 64k .. 64k + 63 (one wave: thread t of a pass takes unit t) are all whole."""
    return all(enc_whole(n, g) for g in (WAVE * k, WAVE * k + WAVE - 1)) and WAVE * k + WAVE - 1 < enc_units(n)


def dec_whole(units: int, g: int) -> bool:
    """The decrypt kernels' fast path: every unit but the first (nonce) and the last (padding)."""
    return 1 <= g <= units - 2


def dec_wave_full(units: int, k: int) -> bool:
    """decrypt_fused_kernel: thread t of a pass takes unit 1 + t, so wave k holds units 1 + 64k .. 64k + 64."""
    return dec_whole(units, 1 + WAVE * k) and dec_whole(units, WAVE * k + WAVE)


def dec2_wave_full(units: int, k: int) -> bool:
    """decode_kernel (the two-pass decrypt): thread t takes unit t, wave k holds units 64k .. 64k + 63."""
    return dec_whole(units, WAVE * k) and dec_whole(units, WAVE * k + WAVE - 1)


def locate(unit: int, stride: int, first_unit: int = 0) -> Tuple[int, int, int, int]:
    """(unit, pass, wave, lane) of the thread that handles `unit` when thread t
    of pass p takes unit first_unit + t + p * stride."""
    t = unit - first_unit
    return unit, t // stride, (t % stride) // WAVE, t % WAVE


# ------------------------------------------------------------------ envelope: references
_B64 = re.compile(rb"[A-Za-z0-9+/]*={0,2}")
_HEX = re.compile(rb"[0-9a-fA-F]*")


def canonical(text: bytes, hex_: bool) -> bool:
    """The strict predicate behind the kernels' `bad` flag (and the length test
    of dn_aes_decrypt_capacity): hex — even length, hex digits only, no "0x";
    base64 — alphabet characters then at most two '=', at least 24 characters,
    a multiple of 4."""
    if hex_:
        if len(text) & 1 or not _HEX.fullmatch(text):
            return False
        text = bytes.fromhex(text.decode("ascii"))
    return len(text) >= 24 and len(text) % 4 == 0 and _B64.fullmatch(text) is not None


def want_text(key: bytes, nonce: bytes, data: bytes, hex_: bool = False) -> bytes:
    """aes.encrypt's text (aes.py:8-14) with the oracle cipher; hex_: its hex digits (no "0x")."""
    b = base64.b64encode(nonce + c_oracle.aes_ctr(key, nonce, data))
    return b.hex().encode() if hex_ else b


def ref_decrypt(key: bytes, text: bytes, hex_: bool = False) -> bytes:
    """The receiver's path: hex_to_bytes (hex.py:29-41) then aes.decrypt (aes.py:17-23)."""
    if hex_:
        s = text.decode("ascii")
        text = bytes.fromhex(s[2:] if s.startswith("0x") else s)
    raw = base64.b64decode(text)
    if len(raw[:16]) != 16:
        raise ValueError("Invalid nonce size")
    return c_oracle.aes_ctr(key, raw[:16], raw[16:])


def rand_bytes(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def nonce_wrapping_at(block: int) -> bytes:
    """The nonce whose 128-bit counter wraps to 0 at keystream block `block`."""
    return ((1 << 128) - block).to_bytes(16, "big")


# byte classification: one 67-unit text — slow unit 0, one full coalesced wave
# (units 1..64), one whole unit read per lane (65), the slow last unit (66)
CLASS_UNITS = 67
CLASS_RAGGED = {"==": 4, "=": 5, "": 6}   # message bytes of the last unit -> padding of the text
CLASS_COAL_UNIT, CLASS_LONE_UNIT = 20, 65


def class_n(pad: str) -> int:
    n = n_for_units(CLASS_UNITS, CLASS_RAGGED[pad])
    assert pad_chars(n) == len(pad)
    return n


def class_positions(pad: str, hex_: bool) -> List[int]:
    """Byte positions of the text (without "0x") at which every byte value is tried."""
    n = class_n(pad)
    chars, units = text_chars(n), text_units(n)
    assert units == CLASS_UNITS and dec_wave_full(units, 0) and not dec_wave_full(units, 1)
    assert dec_whole(units, CLASS_LONE_UNIT) and CLASS_LONE_UNIT > WAVE
    last = TEXT_UNIT * (units - 1)
    assert chars - last >= 4 + len(pad)
    if hex_:
        pos = [128 * CLASS_COAL_UNIT + o for o in (40, 41, 42, 43)]      # digit offsets 0..3 (mod 4)
        pos += [128 * CLASS_LONE_UNIT + o for o in (16, 37, 70, 107)]    # the same four, other words
        pos += [10, 2 * (chars - 3) + 1]                                 # a nonce character, the last before the padding
        pos += [2 * (chars - 2), 2 * (chars - 2) + 1, 2 * (chars - 1), 2 * (chars - 1) + 1]
        assert [p % 4 for p in pos[:8]] == [0, 1, 2, 3, 0, 1, 2, 3]
    else:
        pos = [64 * CLASS_COAL_UNIT + o for o in (20, 21, 22, 23)]       # character offsets 0..3 (mod 4)
        pos += [64 * CLASS_LONE_UNIT + 33, 5, last + 1, chars - 2, chars - 1]
    assert len(set(pos)) == len(pos) and max(pos) < text_len(n, hex_)
    return pos


def substitute(text: bytes, pos: int, value: int) -> bytes:
    return text[:pos] + bytes([value]) + text[pos + 1:]


CLASS_KEY, CLASS_NONCE = bytes(range(32)), bytes(range(200, 216))


def class_texts() -> List[Tuple[str, bool, bytes, List[int]]]:
    """(label, hex, canonical text, positions) of the byte-classification table:
    base64 texts with two, one and no '=', and the hex of the first."""
    out = []
    for pad in ("==", "=", ""):
        data = rand_bytes(class_n(pad), 700 + len(pad))
        text = want_text(CLASS_KEY, CLASS_NONCE, data)
        assert text.endswith(pad.encode()) and not text[:len(text) - len(pad)].endswith(b"=")
        out.append(("base64" + pad, False, text, class_positions(pad, False)))
    hx = out[0][2].hex().encode()
    out.append(("hex", True, hx, class_positions("==", True)))
    return out


# sizes of the canonical-text test: the envelope suite's sizes, the encrypt
# twin of 6128 / 6129, and decrypt waves one unit short of full, full, and full + 1
BASE_SIZES = [0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 95, 96, 97, 127, 128, 129,
              191, 192, 1000, 3071, 3072, 3073, 6128, 6129, 12345, 98288]
CANON_UNITS = [65, 66, 67, 129, 130, 131]
CANON_SIZES = BASE_SIZES + [6127] + [n_for_units(u, 7 + 5 * i) for i, u in enumerate(CANON_UNITS)]
EDGE_DEC_UNITS = [65, 66, 67, 129, 130, 131]       # fused decrypt: 65-67; the two-pass decode: 129-131
EDGE_ENC_TOTALS = [6143, 6144, 6145]               # n + 16 around 48 * 128
SKEWS = [0, 1, 2, 15]


def two_pass_units(stride: int) -> int:
    """Units of the whole-message test: two full strides, two full waves and 7."""
    return 2 * stride + 2 * WAVE + 7


# ------------------------------------------------------------------ codec: limbs, tiles, records
LIMBS, TILE, TILE_BYTES = 17, 256, 66 * 256
SCAN_BLOCK = 1024            # elements per block total (lengths_scan_kernel)
SCAN_STAGE = 8192            # block totals per pass of scan_blocks_kernel
MAX_RECORD = 1 + 8 + 66
DEC_WINDOW_LIMIT = 64 * MAX_RECORD + 8 + 12   # decode_kernel: Bend - A4 at most this on the LDS path
P = (1 << 521) - 1


def vec_bytes(n: int) -> int:
    return ((n + TILE - 1) // TILE) * TILE_BYTES


def ints_to_limbs(vals: Sequence[int]) -> np.ndarray:
    buf = b"".join(int(v).to_bytes(4 * LIMBS, "little") for v in vals)
    return np.frombuffer(buf, dtype="<u4").reshape(len(vals), LIMBS).astype(np.uint32)


def limbs_to_ints(limbs: np.ndarray) -> List[int]:
    raw = np.ascontiguousarray(limbs, dtype="<u4").reshape(-1, LIMBS).tobytes()
    return [int.from_bytes(raw[i:i + 4 * LIMBS], "little") for i in range(0, len(raw), 4 * LIMBS)]


def x_bytes(x: int) -> bytes:
    return x.to_bytes((x.bit_length() + 7) // 8, "big")


def be_image(limbs: np.ndarray) -> np.ndarray:
    """uint32 [k, 17] -> uint8 [k, 68]: each value's 68 big-endian bytes."""
    limbs = np.asarray(limbs, dtype=np.uint32).reshape(-1, LIMBS)
    return np.ascontiguousarray(limbs[:, ::-1]).astype(">u4").view(np.uint8).reshape(-1, 4 * LIMBS)


def y_lengths(limbs: np.ndarray) -> np.ndarray:
    """Minimal big-endian byte length of each value (0 -> 0)."""
    nz = be_image(limbs) != 0
    return np.where(nz.any(axis=1), 4 * LIMBS - nz.argmax(axis=1), 0).astype(np.int64)


def build_records(x: int, limbs: np.ndarray, n: int = None, index: np.ndarray = None):
    """The packed `_share_to_bytes((x, y_e))` records of a vector and their
    offsets[n + 1], vectorised: (uint8 array, int64 array).  limbs: uint32
    [k, 17]; with `index` (increasing element numbers) they are the values of
    those elements of an n-element vector that is zero elsewhere."""
    img = be_image(limbs)
    k = img.shape[0]
    if index is None:
        n, index = k, np.arange(k, dtype=np.int64)
    index = np.asarray(index, dtype=np.int64)
    assert index.shape == (k,) and (k == 0 or (index[0] >= 0 and index[-1] < n and (np.diff(index) > 0).all()))
    ylen_k = y_lengths(limbs)
    head = bytes([len(x_bytes(x))]) + x_bytes(x)
    reclen = np.full(n, len(head), dtype=np.int64)
    reclen[index] += ylen_k
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(reclen, out=offsets[1:])
    packed = np.zeros(int(offsets[n]), dtype=np.uint8)
    for j, b in enumerate(head):
        packed[offsets[:n] + j] = b
    ystart = offsets[index] + len(head)
    first = 4 * LIMBS - ylen_k            # image column of each value's first significant byte
    for c in range(4 * LIMBS):
        sel = np.nonzero(first <= c)[0]
        if sel.size:
            packed[ystart[sel] + (c - first[sel])] = img[sel, c]
    return packed, offsets


def tiles_of(limbs: np.ndarray) -> np.ndarray:
    """field.limbs_to_vec restated: uint32 [k, 17] (k elements from a tile
    boundary on) -> the uint8 bytes of their ceil(k / 256) tiles: per tile
    uint32 lo[16][256] (limb i of element w at lo[i][w]) then uint16 hi[256]."""
    limbs = np.asarray(limbs, dtype=np.uint32).reshape(-1, LIMBS)
    k = limbs.shape[0]
    nt = (k + TILE - 1) // TILE
    lo = np.zeros((nt, 16, TILE), dtype="<u4")
    hi = np.zeros((nt, TILE), dtype="<u2")
    e = np.arange(k)
    for i in range(16):
        lo[e // TILE, i, e % TILE] = limbs[:, i]
    hi[e // TILE, e % TILE] = limbs[:, 16]
    out = np.empty((nt, TILE_BYTES), dtype=np.uint8)
    out[:, :64 * TILE] = lo.reshape(nt, -1).view(np.uint8)
    out[:, 64 * TILE:] = hi.view(np.uint8)
    return out.reshape(-1)


def fill_tiles(put: Callable[[int, np.ndarray], None], limbs: np.ndarray, chunk_tiles: int = 512) -> None:
    """Fill a tiled vector tile-wise: put(byte offset, uint8 array) receives the
    bytes of `chunk_tiles` tiles at a time (a device tensor's slice copy)."""
    limbs = np.asarray(limbs, dtype=np.uint32).reshape(-1, LIMBS)
    step = chunk_tiles * TILE
    for e0 in range(0, limbs.shape[0], step):
        put(e0 // TILE * TILE_BYTES, tiles_of(limbs[e0:e0 + step]))


def scatter_tiles(index: np.ndarray, limbs: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(byte positions int64 [66 k], byte values uint8 [66 k]) of elements
    `index` of a tiled vector: what a sparse fill of a zeroed vector stores."""
    index = np.asarray(index, dtype=np.int64)
    limbs = np.asarray(limbs, dtype=np.uint32).reshape(-1, LIMBS)
    base, w = index // TILE * TILE_BYTES, index % TILE
    pos, val = [], []
    for i in range(16):
        for b in range(4):
            pos.append(base + 4 * (i * TILE + w) + b)
            val.append((limbs[:, i] >> (8 * b)).astype(np.uint8))
    for b in range(2):
        pos.append(base + 64 * TILE + 2 * w + b)
        val.append((limbs[:, 16] >> (8 * b)).astype(np.uint8))
    return np.concatenate(pos), np.concatenate(val)


def ragged_limbs(n: int, seed: int) -> np.ndarray:
    """n values below p of every byte length 0..66 (uniform lengths), uint32 [n, 17]."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (n, 4 * LIMBS), dtype=np.uint8)   # little-endian bytes
    blen = rng.integers(0, 67, n)
    img[np.arange(4 * LIMBS)[None, :] >= blen[:, None]] = 0
    img[:, 65] &= 1                                              # 521 bits
    img[:, 0] &= 0xFE                                            # never p itself
    return img.view("<u4").astype(np.uint32)


# the value plan of the two-pass scan test
SCAN2_N = SCAN_STAGE * SCAN_BLOCK + SCAN_BLOCK + 1     # 8194 block totals: the second pass scans two
SCAN2_EDGES = (1, 511, 512, 513, 8191, 8192, 8193)
SPARSE_STEP = 1021


def sparse_values(n: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(index int64 [k], byte lengths int64 [k], limbs uint32 [k, 17]) of the
    non-zero elements of an n-element vector: every 1021st element a 1-3-byte
    value; the elements on both sides of the scan-block edges 1024 j
    (j in SCAN2_EDGES) and the last element alternately a 66-byte value (top
    limb set) and a 64-byte one (top limb zero: the kernel's y_len_low)."""
    plan = {}
    for e in range(0, n, SPARSE_STEP):
        b = 1 + (e // SPARSE_STEP) % 3
        plan[e] = (b, ((0x9E3779B97F4A7C15 * (e + 1)) % (1 << (8 * b))) | (1 << (8 * b - 8)))
    edge = sorted({e for j in SCAN2_EDGES for e in (SCAN_BLOCK * j - 1, SCAN_BLOCK * j) if 0 <= e < n} | {n - 1})
    for i, e in enumerate(edge):
        b = 66 if i % 2 == 0 else 64
        v = pow(3, 1000 + e, P) | (1 << 520)
        plan[e] = (b, v if b == 66 else (v & ((1 << 512) - 1)) | (1 << 511))
    index = np.array(sorted(plan), dtype=np.int64)
    nbytes = np.array([plan[int(e)][0] for e in index], dtype=np.int64)
    limbs = ints_to_limbs([plan[int(e)][1] for e in index])
    return index, nbytes, limbs


# ------------------------------------------------------------------ codec: window arithmetic
def encode_window(offsets: np.ndarray, e0: int, n: int, al: int) -> Tuple[int, int, bool]:
    """encode_kernel's wave of elements e0 .. e0 + 63: its byte range [A, B)
    and whether the whole range sits inside one aligned chunk (`a4 > b4`) for
    the al-byte store path (16 or 4)."""
    A, B = int(offsets[e0]), int(offsets[min(e0 + WAVE, n)])
    return A, B, (A + al - 1) // al * al > B // al * al


def decode_window(offsets: np.ndarray, e0: int, n: int, al: int) -> int:
    """decode_kernel's Bend - A4 for the wave of records e0 .. e0 + 63 on the
    al-byte staging path: at most DEC_WINDOW_LIMIT -> LDS path, else byte-serial."""
    A, B = int(offsets[e0]), int(offsets[min(e0 + WAVE, n)])
    return B - A // al * al


def pack_records(recs: Sequence[bytes], first_offset: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """Hand-built records back to back from byte `first_offset` on: (uint8 array, int64 offsets)."""
    offs = np.cumsum([first_offset] + [len(r) for r in recs]).astype(np.int64)
    return np.frombuffer(bytes(first_offset) + b"".join(recs), dtype=np.uint8).copy(), offs


# ------------------------------------------------------------------ ChaCha counter
def prng_offset_below_2_32(t: int) -> int:
    """The 256-aligned elem_offset one tile below the element whose first
    coefficient index i = g (t - 1) reaches 2^32."""
    return (1 << 32) // (t - 1) // TILE * TILE - TILE


def prng_index_range(off: int, n: int, t: int) -> Tuple[int, int]:
    """First and last coefficient index i = g (t - 1) + (j - 1) of elements off .. off + n - 1."""
    return off * (t - 1), (off + n - 1) * (t - 1) + (t - 2)
