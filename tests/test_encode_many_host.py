"""encode_shares_many on the host side (no kernel launches).

* the function and the two C entry points exist and are listed in
  codec.EXPORTS; every argument error fires before any device use;
* dn_m521_encode_many_scratch_bytes grows with the tiles and with the rows;
* the C entry point validates as dn_m521_encode_shares and
  dn_m521_reconstruct_many do, before any device call;
* the arithmetic that turns (segment table, global tile) into (segment, local
  tile, live words, global element index) (csrc/enc_plan.hpp, shared with the
  kernels) and a CPU model of the three launches are checked against a
  per-element map by a stand-alone program (tests/host/enc_plan_check.cpp)
  built with AddressSanitizer and UndefinedBehaviorSanitizer — the one place
  where a mistake would read outside a block or write a neighbour's bytes,
  rehearsed before any GPU run.
"""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

from delta_node.crypto.shamir import _native, codec, field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dn_m521_encode_many_scratch_bytes", "dn_m521_encode_shares_many")


def test_function_and_entry_points_exist():
    assert callable(getattr(codec, "encode_shares_many"))
    L = codec._lib()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in codec.EXPORTS
    header = open(os.path.join(ROOT, "include", "dn_shamir.h")).read()
    for name in NAMES:
        assert name + "(" in header
    assert "shamir.py:28-33" in codec.encode_shares_many.__doc__
    assert "encode_shares_many" in codec.__doc__


def _blocks(ns, S=5):
    return [torch.zeros((S, field.vec_bytes(n)), dtype=torch.uint8) for n in ns]


def test_argument_errors_fire_before_any_device_use():
    many = codec.encode_shares_many
    ns = [4, 0, 300]
    with pytest.raises(ValueError, match="^encode_shares_many: 3 blocks for 2 sizes$"):
        many(_blocks(ns), ns[:2])
    with pytest.raises(ValueError, match="negative element count"):
        many(_blocks([4]), [-4])
    with pytest.raises(ValueError, match="block 2 must be a contiguous uint8 tensor"):
        many(_blocks([4, 0, 256]), ns)  # one tile for a two-tile tensor
    with pytest.raises(ValueError, match="block 0 must be a contiguous uint8 tensor"):
        many([b.to(torch.int8) if k == 0 else b for k, b in enumerate(_blocks(ns))], ns)
    with pytest.raises(ValueError, match="block 1 must be a contiguous uint8 tensor"):
        many([torch.zeros((5, 2 * field.vec_bytes(n)), dtype=torch.uint8)[:, ::2] if k == 1 else b
              for k, (b, n) in enumerate(zip(_blocks([4, 4, 300]), [4, 4, 300]))], [4, 4, 300])
    with pytest.raises(ValueError, match="block 0 must be a contiguous uint8 tensor"):
        many([torch.zeros((1, 5, field.vec_bytes(4)), dtype=torch.uint8)], [4])
    with pytest.raises(ValueError, match="block 1 has 3 rows"):
        many([_blocks([4])[0], _blocks([300], S=3)[0]], [4, 300])
    with pytest.raises(ValueError, match="block 1 has 1 rows"):  # a 1-D block counts as S = 1
        many([_blocks([4])[0], torch.zeros(field.vec_bytes(300), dtype=torch.uint8)], [4, 300])
    with pytest.raises(NotImplementedError, match="x must fit 64 bits"):
        many(_blocks(ns), ns, [1, 1 << 64], rows=[0, 1])
    with pytest.raises(NotImplementedError, match="x must fit 64 bits"):
        many(_blocks(ns), ns, [-1], rows=[0])
    with pytest.raises(ValueError, match="rows must lie in \\[0, 5\\)"):
        many(_blocks(ns), ns, [6])  # the default row of x = 6 is past the blocks' 5 rows
    with pytest.raises(ValueError, match="rows must lie in \\[0, 5\\)"):
        many(_blocks(ns), ns, [1, 2], rows=[0, 5])
    with pytest.raises(ValueError, match="1 rows for 2 abscissas"):
        many(_blocks(ns), ns, [1, 2], rows=[0])
    with pytest.raises(ValueError, match="rows without xs"):
        many(_blocks(ns), ns, rows=[0])
    with pytest.raises(ValueError, match="1 outs for 2 abscissas"):
        many(_blocks(ns), ns, [1, 2], outs=[torch.zeros(8, dtype=torch.uint8)])
    with pytest.raises(ValueError, match="3 offsets for 2 abscissas"):
        many(_blocks(ns), ns, [1, 2], offsets=[torch.zeros(8, dtype=torch.int64)] * 3)
    with pytest.raises(ValueError, match="must be on a HIP device"):
        many(_blocks(ns), ns)  # valid arguments, host tensors: refused, nothing computed on the host
    assert many(_blocks(ns), ns, []) == []  # no abscissa: no wire, no device


def test_scratch_bytes_grow_with_tiles_and_rows():
    sb = codec._lib().dn_m521_encode_many_scratch_bytes
    for segs in (1, 127, 65536):
        for tiles in (1, 53, 65536):
            for rows in (1, 5, 17):
                # the table's entries (tile range, element range, n, base, pitch) and 8 bytes per (tile, wire)
                assert sb(segs, tiles, rows) >= 40 * (segs + 1) + 8 * tiles * rows
                assert sb(segs, tiles + 1, rows) > sb(segs, tiles, rows)
                assert sb(segs, tiles, rows + 1) > sb(segs, tiles, rows)
                assert sb(segs + 1, tiles, rows) > sb(segs, tiles, rows)
    assert sb(127, 65536, 5) < 4 * (1 << 20)  # 2^24 elements x 5 wires: MBs, not the 335 MB of a per-element prefix


def test_entry_point_validates_before_any_device_call():
    """A list without elements: DN_OK without touching a pointer.  Null
    pointers, a misaligned out, a capacity below dn_m521_encoded_capacity and
    more than 65536 tensors: DN_ERR_ARG (the pointers given are host memory or
    small integers — none is dereferenced on the way)."""
    L = codec._lib()
    u64, vp, u32 = ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32
    enc = L.dn_m521_encode_shares_many
    OK, ARG = _native.DN_OK, _native.DN_ERR_ARG
    zeros = (u64 * 3)(0, 0, 0)
    assert enc(zeros, None, None, 3, None, None, None, None, None, 5, None, None, 0, None) == OK
    assert enc(None, None, None, 0, None, None, None, None, None, 5, None, None, 0, None) == OK
    assert enc(zeros, None, None, 65537, None, None, None, None, None, 5, None, None, 0, None) == ARG
    assert "65536" in _native.last_error()
    assert enc(None, None, None, 2, None, None, None, None, None, 5, None, None, 0, None) == ARG

    ns = (u64 * 2)(300, 5)
    n_total, tiles = 305, 3
    blocks, pitches = (vp * 2)(0x1000, 0x100000), (u64 * 2)(field.vec_bytes(300), field.vec_bytes(5))
    rows, xs = (u32 * 2)(0, 1), (u64 * 2)(1, 300)
    offs, outs = (vp * 2)(0x2000, 0x3000), (vp * 2)(0x4000, 0x5004)
    caps = (u64 * 2)(L.dn_m521_encoded_capacity(n_total, 1), L.dn_m521_encoded_capacity(n_total, 300))
    sb = L.dn_m521_encode_many_scratch_bytes(2, tiles, 2)
    totals, scratch = vp(0x6000), vp(0x7000)

    def call(**kw):
        a = dict(ns=ns, blocks=blocks, pitches=pitches, nseg=2, rows=rows, xs=xs, offs=offs, outs=outs, caps=caps,
                 m=2, totals=totals, scratch=scratch, sb=sb)
        a.update(kw)
        return enc(a["ns"], a["blocks"], a["pitches"], a["nseg"], a["rows"], a["xs"], a["offs"], a["outs"], a["caps"],
                   a["m"], a["totals"], a["scratch"], a["sb"], None)

    assert call(m=0) == OK  # no wire: nothing to do
    for null in ("blocks", "pitches", "rows", "xs", "offs", "outs", "caps", "totals", "scratch"):
        assert call(**{null: None}) == ARG, null
        assert "null pointer" in _native.last_error()
    assert call(blocks=(vp * 2)(0x1000, None)) == ARG and "null block of tensor 1" in _native.last_error()
    assert call(blocks=(vp * 2)(0x1002, 0x100000)) == ARG and "4-byte aligned" in _native.last_error()
    assert call(offs=(vp * 2)(0x2000, None)) == ARG and "wire 1" in _native.last_error()
    assert call(outs=(vp * 2)(0x4000, None)) == ARG and "wire 1" in _native.last_error()
    assert call(outs=(vp * 2)(0x4000, 0x5002)) == ARG and "out of wire 1 must be 4-byte aligned" in _native.last_error()
    assert call(caps=(u64 * 2)(caps[0], caps[1] - 1)) == ARG and "capacity" in _native.last_error()
    # the capacity is that of the whole list under the wire's own x (x = 300: two x bytes)
    assert call(caps=(u64 * 2)(caps[0], L.dn_m521_encoded_capacity(n_total, 1))) == ARG
    assert call(sb=sb - 1) == ARG and "scratch too small" in _native.last_error()
    assert call(ns=(u64 * 2)(300, (1 << 40) + 1)) == ARG and "too long" in _native.last_error()


def test_tile_plan_and_launch_model_against_per_element_map(tmp_path):
    """Every global tile of the ragged test list (several header lengths and
    rows) and of 1000 seeded random tables (sizes 0..700): each global element
    visited exactly once at its own (segment, local tile, word) and global
    index, no word at or past n_k live, the cursor equal to the binary search,
    and the byte ranges a CPU model of the three launches assigns to the tiles'
    waves disjoint and tiling [0, total) — by a stand-alone program under
    ASan + UBSan (not loaded into this process)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path / "enc_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "delta-node_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "enc_plan_check.cpp"), "-o", exe]
    # the sanitizer runtimes linked statically where the compiler can (the
    # program then runs whatever else the environment loads into processes)
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok"
