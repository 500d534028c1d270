"""The share commitment kernel (csrc/commit_sha256.hip) as a Python model:
which records of a wire with untrusted offsets are hashable, the digest each
must get, and the wires that put every padding class on every byte phase of
both staging paths.  A helper for test_commit_host.py and test_gpu_commit.py
(no tests, no torch).

Nothing here calls the library under test.  The rule is include/dn_commit.h's,
written over record_edges.windows: per wave of 64 records the window [A, Bend)
is usable iff Bend >= A and Bend <= in_bytes; record e is hashable iff its
window is usable, off[e] >= A, off[e + 1] >= off[e] and off[e + 1] <= Bend.
A hashable record's digest is hashlib.sha256 of its bytes (the reference's
calc_commitment); any other record is 32 zero bytes and counts once.  Whether
the window is staged in LDS (record_edges.Window.lds) decides the path the
kernel takes, never the result.
"""
from __future__ import annotations

import functools
import hashlib
from typing import List, Sequence, Tuple

import numpy as np

import record_edges as re

ZERO = bytes(32)
U64 = re.U64
LENGTHS = 131                  # record lengths 0..130: one, two and three blocks
N_PHASE = 2 * LENGTHS          # 262 records: four full waves and a partial one
LONG = 5000                    # a record of 79 blocks


def sha(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


def blocks_of(length: int) -> int:
    return (length + 9 + 63) // 64


def want(packed: bytes, offsets: Sequence[int], in_bytes: int, n: int, align: int) -> List[Tuple[bool, bytes]]:
    """Per record (hashable, digest)."""
    packed = bytes(packed)
    assert in_bytes <= len(packed)
    out = []
    for w in re.windows(offsets, in_bytes, n, align):
        usable = w.Bend >= w.A and w.Bend <= in_bytes
        for e in range(w.e0, w.eN):
            oe, ee = int(offsets[e]) & U64, int(offsets[e + 1]) & U64
            if usable and oe >= w.A and ee >= oe and ee <= w.Bend:
                out.append((True, sha(packed[oe:ee])))
            else:
                out.append((False, ZERO))
    return out


def want_wire(w: re.Wire, align: int = None) -> List[Tuple[bool, bytes]]:
    return want(w.packed.tobytes(), w.offsets.tolist(), w.in_bytes, w.n, align or re.align_of(w.shift))


def digests_of(wanted) -> np.ndarray:
    return np.frombuffer(b"".join(d for _, d in wanted), dtype=np.uint8).reshape(len(wanted), 32).copy()


def serial_windows(w: re.Wire, align: int = None) -> List[int]:
    """The waves whose window is usable but not staged in LDS."""
    return [i for i, win in enumerate(w.windows(align)) if not win.lds and win.A <= win.Bend <= w.in_bytes]


# ------------------------------------------------------------------ wires
def _bytes(length: int, rng) -> bytes:
    return rng.integers(0, 256, length, dtype=np.uint8).tobytes()


def phase_lengths() -> List[int]:
    """Even e: e / 2, odd e: 130 - e // 2.  Every length 0..130 occurs twice,
    every pair sums to 130, so every full window holds 32 * 130 = 4160 bytes
    and record starts fall on every byte phase."""
    return [e // 2 if e % 2 == 0 else LENGTHS - 1 - e // 2 for e in range(N_PHASE)]


@functools.lru_cache(maxsize=None)
def phase_wire(shift: int) -> re.Wire:
    rng = np.random.default_rng(2024)
    return re.from_records([_bytes(length, rng) for length in phase_lengths()], 0, shift)


@functools.lru_cache(maxsize=None)
def sorted_wire(shift: int) -> re.Wire:
    """The same lengths ascending: waves 2 and 3 hold 5088 and 7136 bytes."""
    rng = np.random.default_rng(2025)
    return re.from_records([_bytes(length, rng) for length in sorted(phase_lengths())], 0, shift)


@functools.lru_cache(maxsize=None)
def long_wire(shift: int) -> re.Wire:
    """One record of 5000 bytes at lane 17 beside 63 short ones, then 10 more records."""
    rng = np.random.default_rng(2026)
    lengths = [(7 * i) % 60 for i in range(64)] + [55, 56, 63, 64, 65, 119, 120, 0, 1, 75]
    lengths[17] = LONG
    return re.from_records([_bytes(length, rng) for length in lengths], 0, shift)
