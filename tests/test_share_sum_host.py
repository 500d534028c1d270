"""sum_shares_vec on the host side (no kernel launches).

* the method, the binding and the C entry point exist, and the symbol is
  listed in _native.EXPORTS;
* every argument error of the method fires before any device use (CPU
  tensors, no HIP device needed);
* dn_m521_sum_vecs validates before any device call: n_tiles == 0 is DN_OK
  and touches no pointer; m == 0, a null pointer, 2^32 tiles, a partial
  overlap with `out` and more aliases of `out` than one launch holds are
  DN_ERR_ARG;
* the logic that spreads m inputs over chained launches of
  DN_M521_SUM_GROUP inputs (csrc/sum_plan.hpp, shared with the entry point)
  is replayed on a model of memory by a stand-alone program
  (tests/host/sum_plan_check.cpp) built with AddressSanitizer and
  UndefinedBehaviorSanitizer and run as a subprocess.
"""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from delta_node.crypto import shamir
from delta_node.crypto.shamir import _native, field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TB = field.TILE_BYTES


def sum_group() -> int:
    """DN_M521_SUM_GROUP as include/dn_shamir.h defines it (its one definition)."""
    with open(os.path.join(ROOT, "include", "dn_shamir.h")) as f:
        found = re.findall(r"^#define\s+DN_M521_SUM_GROUP\s+(\d+)\s*$", f.read(), flags=re.M)
    assert len(found) == 1, found
    return int(found[0])


def test_method_binding_and_entry_point_exist():
    assert callable(getattr(shamir.SecretShare, "sum_shares_vec"))
    assert callable(_native.sum_vecs)
    assert hasattr(_native.lib(), "dn_m521_sum_vecs")
    assert "dn_m521_sum_vecs" in _native.EXPORTS
    assert "dn_m521_sum_vecs" in _native.exported_symbols()
    g = sum_group()
    assert g >= 32 and g % 32 == 0  # the sign words of the kernel arguments


def _blocks(m, tiles=1):
    return [torch.zeros(tiles * TB, dtype=torch.uint8) for _ in range(m)]


def test_argument_errors_fire_before_any_device_use(monkeypatch):
    def no_device():
        raise AssertionError("sum_shares_vec reached the device before its argument checks")

    monkeypatch.setattr(_native, "require_device", no_device)
    monkeypatch.setattr(_native, "sum_vecs", lambda *a, **k: no_device())
    ss = shamir.SecretShare(3)
    s = ss.sum_shares_vec
    with pytest.raises(NotImplementedError, match="GF\\(2\\^521 - 1\\) only"):
        shamir.SecretShare(3, prime=(1 << 127) - 1).sum_shares_vec([])  # _require_m521 comes first
    with pytest.raises(ValueError, match="^sum_shares_vec: no blocks$"):
        s([])
    with pytest.raises(ValueError, match="^sum_shares_vec: no blocks$"):
        s(torch.zeros((0, TB), dtype=torch.uint8))
    with pytest.raises(ValueError, match="sum_shares_vec: blocks must share one shape and device"):
        s(_blocks(2) + _blocks(1, tiles=2))
    with pytest.raises(ValueError, match="sum_shares_vec: blocks must share one shape and device"):
        s([torch.zeros(2 * TB, dtype=torch.uint8), torch.zeros((2, TB), dtype=torch.uint8)])
    with pytest.raises(ValueError, match="^sum_shares_vec: blocks must be uint8 tensors$"):
        s([torch.zeros(TB, dtype=torch.uint8), torch.zeros(TB, dtype=torch.int8)])
    with pytest.raises(ValueError, match="^sum_shares_vec: blocks must be uint8 tensors$"):
        s([torch.zeros(TB, dtype=torch.uint8), bytes(TB)])
    with pytest.raises(ValueError, match="^sum_shares_vec: blocks must be contiguous$"):
        s([torch.zeros(TB, dtype=torch.uint8), torch.zeros(2 * TB, dtype=torch.uint8)[::2]])
    with pytest.raises(ValueError, match="sum_shares_vec: blocks must be whole 16896-byte tiles, got 16895 bytes"):
        s([torch.zeros(TB - 1, dtype=torch.uint8)] * 2)
    with pytest.raises(ValueError, match="sum_shares_vec: blocks must be whole 16896-byte tiles"):
        s(torch.zeros(5, dtype=torch.uint8))  # a 1-D tensor unbinds into scalars
    for bad in ([1, 0, 1], [1, 2, 1], [1, -1, 1.0], [1, True, 1], [1, None, -1]):
        with pytest.raises(ValueError, match="^sum_shares_vec: signs must be \\+1 or -1$"):
            s(_blocks(3), signs=bad)
    with pytest.raises(ValueError, match="^sum_shares_vec: 2 signs for 3 blocks$"):
        s(_blocks(3), signs=[1, -1])
    for bad_out in (torch.zeros(2 * TB, dtype=torch.uint8), torch.zeros(TB, dtype=torch.int8),
                    torch.zeros(2 * TB, dtype=torch.uint8)[::2], torch.zeros((1, TB), dtype=torch.uint8), bytearray(TB)):
        with pytest.raises(ValueError, match="sum_shares_vec: out must be contiguous uint8 \\(16896,\\)"):
            s(_blocks(3), out=bad_out)


def test_the_device_is_required_only_after_the_checks(monkeypatch):
    """Valid CPU arguments get as far as the device requirement, and no further."""
    class Reached(Exception):
        pass

    def reached():
        raise Reached

    monkeypatch.setattr(_native, "require_device", reached)
    monkeypatch.setattr(_native, "sum_vecs", lambda *a, **k: pytest.fail("launched"))
    blocks = _blocks(3)
    with pytest.raises(Reached):
        shamir.SecretShare(3).sum_shares_vec(blocks, signs=[1, -1, 1], out=blocks[1])
    with pytest.raises(Reached):
        shamir.SecretShare(1).sum_shares_vec(torch.zeros((4, 2, TB), dtype=torch.uint8))


def test_binding_checks_its_flags():
    with pytest.raises(ValueError, match="one negate flag per input"):
        _native.sum_vecs([4096, 8192], [True], 4096, 1)


def test_entry_point_validates_before_any_device_call():
    L = _native.lib()
    f = L.dn_m521_sum_vecs
    G = sum_group()
    OK, ARG = _native.DN_OK, _native.DN_ERR_ARG
    vp = ctypes.c_void_p
    base = 0x7F0000000000  # never dereferenced: every call below returns before a launch

    def arr(*ptrs):
        return (vp * len(ptrs))(*ptrs)

    # n_tiles == 0: DN_OK whatever else is passed, no pointer touched
    assert f(None, None, 0, None, 0, None) == OK
    assert f(None, None, 5, None, 0, None) == OK
    assert f(arr(None, None), None, 2, None, 0, None) == OK
    # m == 0, null pointers, 2^32 tiles
    assert f(arr(base), None, 0, base + (1 << 30), 1, None) == ARG
    assert "no input" in _native.last_error()
    assert f(None, None, 1, base, 1, None) == ARG
    assert f(arr(base), None, 1, None, 1, None) == ARG
    assert f(arr(base, None), None, 2, base + (1 << 30), 1, None) == ARG
    assert "null input 1" in _native.last_error()
    assert f(arr(base), None, 1, base, 1 << 32, None) == ARG
    assert "2^32" in _native.last_error()
    # a range that overlaps out without being equal to it, from either side; one tile and three
    for tiles, delta in [(1, 1), (1, TB - 1), (3, TB), (3, 3 * TB - 1)]:
        for sign in (1, -1):
            assert f(arr(base + (1 << 30), base + sign * delta), None, 2, base, tiles, None) == ARG, (tiles, delta)
            assert "overlaps out" in _native.last_error()
    # more inputs equal to out than one launch holds
    assert f(arr(*([base] * (G + 1))), None, G + 1, base, 1, None) == ARG
    assert str(G) in _native.last_error()


def test_launch_plan_replayed_on_a_memory_model(tmp_path):
    """m = 1 .. 3 GROUP + 2, out aliasing nothing, input 0, a middle-group
    input, the last input, repeated addresses: every input consumed once with
    its sign, aliases in launch 1, later launches take out first and positive,
    no launch above GROUP, partial overlaps refused — by a stand-alone program
    under ASan + UBSan (not loaded into this process)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path / "sum_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "delta-node_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "host", "sum_plan_check.cpp"), "-o", exe]
    # the sanitizer runtimes linked statically where the compiler can (the
    # program then runs whatever else the environment loads into processes)
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok"
