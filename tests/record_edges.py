"""The record-reading kernels (csrc/recon_records.hip, csrc/sum_records.hip,
and the frames of csrc/codec_frame.hip that feed them) as a Python model:
the contract for untrusted offsets, exact expected values, the accesses the
contract implies, and the wires that put a window on every edge of the
staging.  A helper for test_record_edges_host.py and
test_gpu_record_edges.py (no tests, no torch).

Nothing here calls the library under test.  The parse is written from the
rules of csrc/wire_parse.hpp, not from its code path: per wave of 64 records
the window [A, Bend) is staged in LDS iff Bend >= A, Bend <= in_bytes and
Bend - A4 <= LIMIT (A4: A rounded down to the wire's alignment, 16 or 4); on
that path a record is good only inside the window (off[e] >= A, off[e + 1] >
off[e], off[e + 1] <= Bend), on the byte-serial path only inside the wire
(off[e] < off[e + 1] <= in_bytes).  Then, on both: the header byte is at most
8, header and x fit the record, y is the rest without its leading zero bytes
and has at most 68 significant bytes; y is not reduced.  A bad record is
y = 0 and counts once; a good one whose x is not the expected one counts in
the second counter and its y is used.

LIMIT and MAX_RECORD are wire_edges.py's (test_wire_geom_host.py ties them to
csrc/wire_geom.hpp); the other geometry constants are restated below and
test_record_edges_host.py compares them with tests/host/wire_geom_check.cpp.
"""
from __future__ import annotations

import functools
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

import wire_edges as we

P = we.P
WAVE, TILE = we.WAVE, we.TILE
MAX_RECORD = we.MAX_RECORD
LIMIT = we.DEC_WINDOW_LIMIT
WIN_PAD = 16                                                  # kWinPad
DEC_WINDOW = 64 * MAX_RECORD + 8                              # kDecWindow
ROW_WORDS = ((DEC_WINDOW + 16 + 2 * WIN_PAD) // 4 + 3) & ~3   # kDecRowWords
STAGE_Q = (LIMIT // 16 + 63) // 64                            # kStageQ: 16-byte rows per lane
STAGE_W = (LIMIT // 4 + 63) // 64                             # kStageW: 4-byte rows per lane
LIMBS = 17                                                    # limb loads of one LDS parse
U64 = (1 << 64) - 1
BAD = (False, 0, 0)


def stage_rows(align: int) -> int:
    return STAGE_Q if align == 16 else STAGE_W


def align_of(shift: int) -> int:
    """The staging width of a wire whose first byte sits `shift` bytes past a 16-byte boundary."""
    assert shift % 4 == 0
    return 16 if shift % 16 == 0 else 4


# ------------------------------------------------------------------ the contract
class Window(NamedTuple):
    e0: int
    eN: int
    A: int
    Bend: int
    A4: int
    lds: bool


def windows(offsets: Sequence[int], in_bytes: int, n: int, align: int) -> List[Window]:
    out = []
    for e0 in range(0, n, WAVE):
        eN = min(e0 + WAVE, n)
        A, Bend = int(offsets[e0]) & U64, int(offsets[eN]) & U64
        A4 = A - A % align
        out.append(Window(e0, eN, A, Bend, A4, Bend >= A and Bend <= in_bytes and Bend - A4 <= LIMIT))
    return out


def parse_record(packed: bytes, o: int, end: int) -> Tuple[bool, int, int]:
    """Record [o, end) of the wire, 0 <= o < end <= len(packed): (ok, x, y)."""
    xlen = packed[o]
    if xlen > 8 or o + 1 + xlen > end:
        return BAD
    y = packed[o + 1 + xlen:end].lstrip(b"\0")
    if len(y) > 68:
        return BAD
    return True, int.from_bytes(packed[o + 1:o + 1 + xlen], "big"), int.from_bytes(y, "big")


def record_in_window(w: Window, oe: int, ee: int, in_bytes: int) -> bool:
    if w.lds:
        return oe >= w.A and ee > oe and ee <= w.Bend
    return oe < ee <= in_bytes


def parse_wire(packed: bytes, offsets: Sequence[int], in_bytes: int, n: int, align: int
               ) -> List[Tuple[bool, int, int]]:
    packed = bytes(packed)
    assert in_bytes <= len(packed)
    out = []
    for w in windows(offsets, in_bytes, n, align):
        for e in range(w.e0, w.eN):
            oe, ee = int(offsets[e]) & U64, int(offsets[e + 1]) & U64
            out.append(parse_record(packed, oe, ee) if record_in_window(w, oe, ee, in_bytes) else BAD)
    return out


# ------------------------------------------------------------------ wires
class Wire:
    """One wire as the tests upload it: the bytes, the offsets table, the
    abscissa its records should carry, the shift of its first byte past a
    16-byte boundary, and the facts its builder claims."""

    def __init__(self, packed, offsets, x: int, shift: int = 0, facts: Optional[dict] = None, want=None):
        self.packed = np.frombuffer(bytes(packed), dtype=np.uint8).copy()
        self.offsets = np.asarray(offsets, dtype=np.int64).copy()
        self.x, self.shift = x, shift
        self.n = self.offsets.size - 1
        self.facts = facts or {}
        self.want = want            # per record the (x, y) the builder meant, None where it meant a bad record
        self._parsed: Dict[int, list] = {}
        self._bounds: Dict[int, list] = {}

    @property
    def in_bytes(self) -> int:
        return int(self.packed.size)

    def parsed(self, align: Optional[int] = None):
        align = align or align_of(self.shift)
        if align not in self._parsed:
            self._parsed[align] = parse_wire(self.packed.tobytes(), self.offsets.tolist(), self.in_bytes, self.n, align)
        return self._parsed[align]

    def with_offsets(self, offsets, facts=None) -> "Wire":
        return Wire(self.packed, offsets, self.x, self.shift, facts)

    def windows(self, align: Optional[int] = None) -> List[Window]:
        return windows(self.offsets.tolist(), self.in_bytes, self.n, align or align_of(self.shift))

    def checked(self, align: Optional[int] = None) -> List[dict]:
        """assert_in_bounds, once per staging width: the report of the accesses."""
        align = align or align_of(self.shift)
        if align not in self._bounds:
            self._bounds[align] = assert_in_bounds(self, align)
        return self._bounds[align]


def y_bytes(v: int) -> bytes:
    return v.to_bytes((v.bit_length() + 7) // 8, "big")


def rec(x: int, y: int, pad: int = 0) -> bytes:
    """The record of (x, y) with `pad` zero bytes in front of y."""
    xb = we.x_bytes(x)
    return bytes([len(xb)]) + xb + bytes(pad) + y_bytes(y)


def from_records(recs: Sequence[bytes], x: int, shift: int = 0, facts=None, want=None, slack: bytes = b"") -> Wire:
    offs = np.cumsum([0] + [len(r) for r in recs]).astype(np.int64)
    return Wire(b"".join(recs) + slack, offs, x, shift, facts, want)


def ordinary_wire(x: int, n: int, seed: int, shift: int = 0) -> Wire:
    """n minimal records of every y length 0..66 (wire_edges.ragged_limbs)."""
    ys = we.limbs_to_ints(we.ragged_limbs(n, seed))
    return from_records([rec(x, y) for y in ys], x, shift, want=[(x, y) for y in ys])


# ------------------------------------------------------------------ expectations
def counts(parsed, x: int) -> Tuple[int, int]:
    return sum(not ok for ok, _, _ in parsed), sum(ok and px != (x & U64) for ok, px, _ in parsed)


def lagrange_at_zero(xs: Sequence[int]) -> List[int]:
    lam = []
    for i, xi in enumerate(xs):
        num = den = 1
        for j, xj in enumerate(xs):
            if j != i:
                num, den = num * xj % P, den * (xj - xi) % P
        lam.append(num * pow(den, -1, P) % P)
    return lam


def want_resolve(wires: Sequence[Wire], xs: Sequence[int], n: int, aligns: Optional[Sequence[int]] = None) -> dict:
    """sum lambda_i y_i mod p per element: the field results, their low 64 bits
    as int64, the count of results from 2^64 on, and the two record counts."""
    aligns = aligns or [None] * len(wires)
    parsed = [w.parsed(a)[:n] for w, a in zip(wires, aligns)]
    lam = lagrange_at_zero(xs)
    fld = [sum(l * p[e][2] for l, p in zip(lam, parsed)) % P for e in range(n)]
    i64 = [(v & U64) - ((v & U64) >> 63 << 64) for v in fld]
    cs = [counts(p, x) for p, x in zip(parsed, xs)]
    return dict(field=fld, i64=i64, overflow=sum(v >> 64 != 0 for v in fld), bad=sum(c[0] for c in cs),
                mis=sum(c[1] for c in cs))


def want_sum(wires: Sequence[Wire], x: int, n: int, signs: Optional[Sequence[int]] = None,
             acc: Optional[Sequence[int]] = None, aligns: Optional[Sequence[int]] = None) -> dict:
    """(acc + sum +-y_i) mod p per element, canonical, and the two record counts."""
    aligns = aligns or [None] * len(wires)
    signs = signs or [1] * len(wires)
    parsed = [w.parsed(a)[:n] for w, a in zip(wires, aligns)]
    fld = [((acc[e] if acc is not None else 0) + sum(s * p[e][2] for s, p in zip(signs, parsed))) % P
           for e in range(n)]
    cs = [counts(p, x) for p in parsed]
    return dict(field=fld, bad=sum(c[0] for c in cs), mis=sum(c[1] for c in cs))


# ------------------------------------------------------------------ the access model
def accesses(packed: bytes, offsets: Sequence[int], in_bytes: int, n: int, align: int) -> List[dict]:
    """Per wave what the contract implies a kernel touches: `glob`, the global
    byte ranges [lo, hi) of the wire (the staging loads from A4 to the aligned
    end, the tail bytes, the records read byte-serially); `lds_write` and
    `lds_read`, the lowest and one past the highest LDS byte relative to window
    byte 0; `rows`, the staging rows j in use, `last_row_lanes`, the lanes of
    the highest one, `tail`, the lanes that carry a tail byte, and `unstaged`,
    the loads that no row of the register file holds."""
    out = []
    for w in windows(offsets, in_bytes, n, align):
        info = dict(window=w, glob=[], lds_write=None, lds_read=None, rows=0, last_row_lanes=0, tail=0, unstaged=0,
                    max_offset_index=w.eN)
        if w.lds:
            Bq = w.Bend - w.Bend % align
            units = (Bq - w.A4) // align
            if units:
                info["glob"].append((w.A4, Bq))
            info["rows"] = -(-units // WAVE)
            info["last_row_lanes"] = units - WAVE * (info["rows"] - 1) if units else 0
            info["unstaged"] = max(0, units - WAVE * stage_rows(align))
            info["tail"] = min(w.Bend - Bq, WAVE)
            if w.Bend > Bq:
                info["glob"].append((Bq, w.Bend))
            if w.Bend > w.A4:
                info["lds_write"] = (0, w.Bend - w.A4)
            lo = hi = None
            for e in range(w.e0, w.eN):
                oe, ee = int(offsets[e]) & U64, int(offsets[e + 1]) & U64
                if not record_in_window(w, oe, ee, in_bytes):
                    continue
                o, end = oe - w.A4, ee - w.A4
                touched = [(o, o + 1)]
                xlen = packed[oe]
                if xlen <= 8 and o + 1 + xlen <= end:
                    touched.append((o + 1, o + 1 + xlen))
                    ys, ok = o + 1 + xlen, True
                    while end - ys > 68:
                        touched.append((ys, ys + 1))
                        if packed[w.A4 + ys]:
                            ok = False
                            break
                        ys += 1
                    if ok:
                        for i in range(LIMBS):
                            d = max(end - 4 * (i + 1), -4) >> 2      # the dword pair of limb i, clamped at byte -4
                            touched.append((4 * d, 4 * d + 8))
                for a, b in touched:
                    lo, hi = (a if lo is None else min(lo, a)), (b if hi is None else max(hi, b))
            if lo is not None:
                info["lds_read"] = (lo, hi)
        else:
            for e in range(w.e0, w.eN):
                oe, ee = int(offsets[e]) & U64, int(offsets[e + 1]) & U64
                if record_in_window(w, oe, ee, in_bytes):
                    info["glob"].append((oe, ee))
        out.append(info)
    return out


def assert_in_bounds(wire: Wire, align: Optional[int] = None) -> List[dict]:
    """Every global range inside [0, in_bytes), every LDS byte inside the padded
    slice, every staged load in a row of the register file; returns the report."""
    align = align or align_of(wire.shift)
    rep = accesses(wire.packed.tobytes(), wire.offsets.tolist(), wire.in_bytes, wire.n, align)
    lds_lo, lds_hi = -WIN_PAD, 4 * ROW_WORDS - WIN_PAD
    for info in rep:
        w = info["window"]
        assert info["max_offset_index"] <= wire.n, w
        for lo, hi in info["glob"]:
            assert 0 <= lo <= hi <= wire.in_bytes, (w, lo, hi, wire.in_bytes)
        if w.lds:
            assert w.A4 % align == 0 and info["unstaged"] == 0 and info["rows"] <= stage_rows(align), (w, info)
        for key in ("lds_write", "lds_read"):
            if info[key] is not None:
                assert lds_lo <= info[key][0] and info[key][1] <= lds_hi, (w, key, info[key])
    return rep


# ------------------------------------------------------------------ builder: the window limit
X8 = (0xF1 << 56) + 0x0102030405
TAIL_DELTAS = {16: (-5, -3), 4: (-3, -1)}   # window sizes LIMIT + delta that end on 15, 1 (mod 16) and 1, 3 (mod 4)


def full_record(x: int, y: int, pad: int = 0) -> bytes:
    """A record of MAX_RECORD + pad bytes: y as 66 bytes behind as many zero bytes as the x header leaves."""
    xb = we.x_bytes(x)
    return bytes([len(xb)]) + xb + bytes(8 - len(xb) + pad) + y.to_bytes(66, "big")


@functools.lru_cache(maxsize=None)
def limit_wire(amod: int, delta: int, align: int, x: int = X8) -> Wire:
    """test_decode_window_limit's construction: four waves of 75-byte records;
    leading zero bytes in one record of wave 1 bring its Bend - A4 to
    LIMIT + delta, with its first byte at `amod` (mod 16)."""
    ys = [y | (1 << 520) for y in we.limbs_to_ints(we.ragged_limbs(256, 100 + amod))]
    pad = [0] * 256
    pad[9] = amod
    pad[64 + 17] = LIMIT + delta - 64 * MAX_RECORD - amod % align
    assert pad[64 + 17] >= 0
    shift = 0 if align == 16 else 4
    facts = dict(wave=1, size=LIMIT + delta, lds=delta <= 0, amod=amod)
    return from_records([full_record(x, y, p) for y, p in zip(ys, pad)], x, shift, facts, [(x, y) for y in ys])


# (amod, delta, align) of the limit cases, and of the set whose windows end on 1 and 15 (mod 16), 1 and 3 (mod 4)
LIMIT_CASES = [(amod, delta, align) for align in (16, 4) for delta in (-1, 0, 1) for amod in (0, 1, 15)]
TAIL_CASES = [(amod, delta, align) for align in (16, 4) for delta in TAIL_DELTAS[align] for amod in (0, 1, 15)
              if (amod, delta, align) not in LIMIT_CASES]   # (LIMIT - 1 on the narrow path is a limit case already)


# ------------------------------------------------------------------ builder: the last staging row
@functools.lru_cache(maxsize=None)
def row_edge_wire(align: int, x: int = X8) -> Wire:
    """Wave 0: a window of exactly (rows - 1) * 64 loads (the last staging row
    unused); wave 1: one load more (the last row used by lane 0 alone); then 20
    ordinary records.  18 * 256 and 18 * 256 + 4 bytes on the narrow path,
    4 * 1024 and 4 * 1024 + 16 on the wide one."""
    full = (stage_rows(align) - 1) * WAVE * align
    rng = np.random.default_rng(align)
    head = 1 + len(we.x_bytes(x))
    recs, want = [], []
    for total in (full, full + align):
        base, extra = divmod(total, WAVE)
        for i in range(WAVE):
            room = base + (i < extra) - head
            ylen = min(room, 64)
            assert ylen >= 1
            y = int.from_bytes(rng.integers(1, 256, ylen, dtype=np.uint8).tobytes(), "big")
            recs.append(rec(x, y, room - ylen))
            want.append((x, y))
    for y in we.limbs_to_ints(we.ragged_limbs(20, 7 + align)):
        recs.append(rec(x, y))
        want.append((x, y))
    facts = dict(sizes=(full, full + align), rows=(stage_rows(align) - 1, stage_rows(align)))
    return from_records(recs, x, 0 if align == 16 else 4, facts, want)


# ------------------------------------------------------------------ builder: window sequences
SEQ = ("largest", "tiny", "serial", "empty", "largest")
SPECIALS = ("one-byte", "header-only", "y68")
SEQ_N = 256 + 20
Y68 = (1 << 544) - 1 - (0xABCDEF << 200)     # a 68-byte y above 2^521


def special_record(kind: str, x: int) -> Tuple[bytes, Tuple[int, int]]:
    if kind == "one-byte":
        return bytes([0]), (0, 0)
    if kind == "header-only":
        return rec(x, 0), (x, 0)
    return rec(x, Y68), (x, Y68)


def sequence_wires(xs: Sequence[int] = (1, 2, 3, 4, 5), shifts: Sequence[int] = (0, 4, 8, 12, 0)) -> List[Wire]:
    return list(_sequence_wires(tuple(xs), tuple(shifts)))


@functools.lru_cache(maxsize=None)
def _sequence_wires(xs, shifts):
    """Five wires over 276 elements.  Wave w of wire i holds a window of kind
    SEQ[(i + w) % 5]: wave 0 meets, wire after wire, the largest LDS window
    (Bend - A4 = LIMIT), 64 two-byte records, a byte-serial window, an empty one
    (Bend = A: 64 bad records) and the largest again; waves 1 to 3 of the same
    workgroup meet rotations of that sequence.  The largest and the byte-serial
    windows begin and end with a one-byte record, a header-only record or a
    68-byte y, in turn; the last, partial wave holds ordinary records."""
    assert len(xs) == len(shifts) == 5
    out = []
    for i, (x, shift) in enumerate(zip(xs, shifts)):
        align = align_of(shift)
        ys = iter(y | (1 << 520) for y in we.limbs_to_ints(we.ragged_limbs(4 * WAVE, 900 + i)))
        recs, want, kinds, ends = [], [], [], {}
        pos = 0
        for w in range(4):
            kind = SEQ[(i + w) % 5]
            kinds.append(kind)
            wave: List[Tuple[bytes, Optional[Tuple[int, int]]]] = []
            if kind == "empty":
                wave = [(b"", None)] * WAVE
            elif kind == "tiny":
                for lane in range(WAVE):
                    if lane % 2 == 0 and x < 256:
                        wave.append((bytes([1, x]), (x, 0)))
                    else:
                        wave.append((bytes([0, 1 + 3 * lane]), (0, 1 + 3 * lane)))
            else:
                turn = i if kind == "serial" else i + w   # every special begins and ends a window of both kinds
                first, last = SPECIALS[turn % 3], SPECIALS[(turn + 2) % 3]
                ends[w] = (first, last)
                pad = 30 if kind == "serial" else 0
                body = []
                for _ in range(WAVE - 2):
                    y = next(ys)
                    body.append((rec(x, y, pad), (x, y)))
                wave = [special_record(first, x)] + body + [special_record(last, x)]
                size = pos % align + sum(len(r) for r, _ in wave)
                if kind == "largest":  # zero bytes in front of one y bring Bend - A4 to LIMIT exactly
                    fill = LIMIT - size
                    assert fill >= 0
                    r, (rx, ry) = wave[29]
                    wave[29] = (rec(rx, ry, fill), (rx, ry))
                else:
                    assert size > LIMIT
            recs += [r for r, _ in wave]
            want += [v for _, v in wave]
            pos += sum(len(r) for r, _ in wave)
        for y in we.limbs_to_ints(we.ragged_limbs(SEQ_N - 4 * WAVE, 950 + i)):
            recs.append(rec(x, y))
            want.append((x, y))
        out.append(from_records(recs, x, shift, dict(kinds=kinds, ends=ends), want))
    return tuple(out)


# ------------------------------------------------------------------ builder: hostile offsets
HOSTILE_N = 4 * WAVE + 20
HOSTILE_X = 3
HOSTILE_SLACK = 5000


@functools.lru_cache(maxsize=None)
def hostile_offsets(align: int) -> Dict[str, Wire]:
    """Offset tables over one good wire (276 ordinary records and 5000 bytes
    that belong to no record), each with its fault in a full wave (wave 1) and
    in the last, partial wave (elements 256..275).  The model classifies every
    record; `facts` names the records the table is about."""
    n, full, part = HOSTILE_N, WAVE, 4 * WAVE
    slack = np.random.default_rng(77).integers(0, 256, HOSTILE_SLACK, dtype=np.uint8).tobytes()
    ys = we.limbs_to_ints(we.ragged_limbs(n, 4242))
    for e in (2 * full - 2, 2 * full - 1, n - 2, n - 1):   # short: a stretched record still parses
        ys[e] = 0x0102 + e
    pads = [0] * n
    for e0 in (full, part):
        # a 3-byte record ends the wave before, two short ones begin this one, and zero bytes in front of an
        # earlier y bring off[e0] to 3 (mod 16): the record [A - 3, off[e0 + 2]) starts at window byte 0 and
        # would parse if only its start were not below A
        ys[e0 - 1], ys[e0], ys[e0 + 1] = 0x41 + e0 % 16, 0x0102 + e0, 0x0304 + e0
        start = sum(len(rec(HOSTILE_X, y, p)) for y, p in zip(ys[:e0], pads[:e0]))
        pads[e0 - 10] = (3 - start) % 16
    good = from_records([rec(HOSTILE_X, y, p) for y, p in zip(ys, pads)], HOSTILE_X, 0 if align == 16 else 4,
                        slack=slack, want=[(HOSTILE_X, y) for y in ys])
    o = good.offsets.tolist()
    size = good.in_bytes

    def table(name, edits, **facts):
        t = list(o)
        for idx, value in edits:
            t[idx] = value
        return name, good.with_offsets(t, facts)

    def a4(e0):
        return o[e0] - o[e0] % align

    tables = [
        ("good", good),
        # a record that starts below its window's A (and so one that ends before it starts)
        table("start-below-A", [(full + 1, o[full] - 3), (part + 1, o[part] - 3)], at=(full + 1, part + 1)),
        # a record that ends one byte above Bend, inside the wire, in LDS windows (it would parse otherwise)
        table("end-above-Bend", [(2 * full - 1, o[2 * full] + 1), (n - 1, o[n] + 1)], at=(2 * full - 2, n - 2)),
        # off[eN] < off[e0]: byte-serial windows whose records end above Bend and parse
        table("eN-below-e0", [(2 * full, o[full] - 1), (n, o[part] - 1)], serial=(full, part)),
        table("eN-past-in-bytes", [(2 * full, size + 1000), (n, size + 5)], serial=(full, part)),
        table("equal-runs", [(e, o[full + 6]) for e in range(full + 6, full + 17)]
              + [(e, o[part + 12]) for e in range(part + 12, part + 16)], empty=(full + 6, part + 12)),
        # a window of exactly LIMIT + 1 bytes made by the offsets alone
        table("limit-plus-1", [(2 * full, a4(full) + LIMIT + 1), (n, a4(part) + LIMIT + 1)], serial=(full, part)),
    ]
    assert a4(part) + LIMIT + 1 <= size
    return dict(tables)


# ------------------------------------------------------------------ builder: frames
FRAME_MAGIC = b"DNSHREC1"
FRAME_N = 4096 + 300
FRAME_BLOCK = 4096


def frame_records_offset(n: int) -> int:
    return 32 + 16 * ((n + 15) // 16)


class Frame(NamedTuple):
    kind: str
    frame: np.ndarray      # uint8: the bytes as they arrive
    cap: int               # len(frame) - R(n): the size of the `packed` view
    offsets: np.ndarray    # int64 [n + 1]: min(cumsum of the lengths, cap)
    bad: Tuple[int, int]   # (the header is not what is expected, the lengths do not sum to cap)
    x: int


def make_frame(kind: str, n: int, x: int, lens: np.ndarray, records: bytes, header_total: Optional[int] = None,
               pad_fill: int = 0) -> Frame:
    R = frame_records_offset(n)
    cap = len(records)
    total = cap if header_total is None else header_total
    head = FRAME_MAGIC + np.array([n, x, total], dtype="<u8").tobytes()
    buf = head + lens.astype(np.uint8).tobytes() + bytes([pad_fill]) * (R - 32 - n) + records
    prefix = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens.astype(np.int64), out=prefix[1:])
    return Frame(kind, np.frombuffer(buf, dtype=np.uint8).copy(), cap, np.minimum(prefix, cap),
                 (int(total != cap), int(int(prefix[n]) != cap)), x)


def frame_wire(f: Frame, shift: int = 0) -> Wire:
    """The (packed, offsets) pair a frame must open to (a frame's records start on a 16-byte boundary)."""
    n = f.offsets.size - 1
    return Wire(f.frame[frame_records_offset(n):], f.offsets, f.x, shift)


@functools.lru_cache(maxsize=None)
def good_frame(n: int, x: int, seed: int) -> Frame:
    w = ordinary_wire(x, n, seed)
    return make_frame("good", n, x, np.diff(w.offsets), w.packed.tobytes())


@functools.lru_cache(maxsize=None)
def corrupt_frames(n: int = FRAME_N, x: int = 3) -> Dict[str, Frame]:
    """One corrupted field at a time (the kinds of test_gpu_frames.py's
    test_one_corrupted_field_at_a_time that leave the header's n and x alone)
    and the frames whose every window is byte-serial or empty, each with the
    offsets it must open to."""
    w = ordinary_wire(x, n, 4243)
    lens = np.diff(w.offsets)
    lens_at10 = int(lens[10])
    assert 1 <= lens_at10 <= 254
    records = w.packed.tobytes()
    out = {}

    def add(kind, lens_, records_, **kw):
        out[kind] = make_frame(kind, n, x, np.asarray(lens_), records_, **kw)

    def changed(e, d):
        l2 = lens.copy()
        l2[e] += d
        assert 0 <= l2[e] <= 255
        return l2

    add("len+1", changed(10, 1), records)
    add("len-1", changed(10, -1), records)
    add("all255short", np.full(n, 255), records[:1000])
    add("truncated", lens, records[:-100], header_total=len(records))
    add("records_bytes", lens, records, header_total=len(records) + 1)
    rng = np.random.default_rng(9)
    ys = [int(v) | (1 << 520) for v in we.limbs_to_ints(we.ragged_limbs(n, 4244))]
    long_recs = b"".join(rec(x, y, 255 - 2 - 66) if e % 3 else rng.integers(0, 256, 255, dtype=np.uint8).tobytes()
                         for e, y in enumerate(ys))
    add("all255full", np.full(n, 255), long_recs)          # every wave byte-serial
    add("all0", np.zeros(n, dtype=np.int64), records[:48])  # every window empty
    add("pad-nonzero", lens, records, pad_fill=0xFF)
    assert n > FRAME_BLOCK and (frame_records_offset(n) - 32 - n) > 0
    add("block-last+1", changed(FRAME_BLOCK - 1, 1), records)
    add("block-first-1", changed(FRAME_BLOCK, -1 if lens[FRAME_BLOCK] else 1), records)
    return out
