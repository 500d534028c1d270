"""resolve_shares_vec_many on the host side (no kernel launches).

* the method and the two C entry points exist and are listed in
  _native.EXPORTS; the reference's argument errors fire before any device use;
* dn_m521_reconstruct_many_scratch_bytes grows with the segments and with k;
* the arithmetic that turns (segment table, global tile) into (segment, local
  tile, live lanes, output offsets) (csrc/recon_plan.hpp, shared with the
  kernel) is checked against a per-element map by a stand-alone program
  (tests/host/recon_plan_check.cpp) built with AddressSanitizer and
  UndefinedBehaviorSanitizer — the one place where a mistake would read or
  write outside a block, rehearsed before any GPU run.
"""
import os
import shutil
import subprocess

import pytest
import torch

from delta_node.crypto import shamir
from delta_node.crypto.shamir import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_method_and_entry_points_exist():
    assert callable(getattr(shamir.SecretShare, "resolve_shares_vec_many"))
    L = _native.lib()
    for name in ("dn_m521_reconstruct_many_scratch_bytes", "dn_m521_reconstruct_many"):
        assert hasattr(L, name), name
        assert name in _native.EXPORTS
    assert callable(_native.reconstruct_many)


def _vecs(k, n=4):
    return [torch.zeros(_native.vec_bytes(n), dtype=torch.uint8) for _ in range(k)]


def test_argument_errors_fire_before_any_device_use():
    ss = shamir.SecretShare(3)
    many = ss.resolve_shares_vec_many
    with pytest.raises(ValueError, match="one abscissa per share vector"):
        many([_vecs(3), _vecs(2)], [1, 2, 3], [4, 4])
    with pytest.raises(ValueError, match="one abscissa per share vector"):
        many([torch.zeros(2, _native.vec_bytes(4), dtype=torch.uint8)], [1, 2, 3], [4])
    with pytest.raises(ValueError, match="^not enough values to unpack \\(expected 2, got 0\\)$"):
        many([[], []], [], [4, 4])
    with pytest.raises(ValueError, match="^need at least 3 shares$"):
        many([_vecs(2)], [1, 2], [4])
    with pytest.raises(ValueError, match="^shares must be distinct$"):
        many([_vecs(3)], [1, 2, 2], [4])
    with pytest.raises(TypeError, match="^reduce\\(\\) of empty iterable with no initial value$"):
        shamir.SecretShare(1).resolve_shares_vec_many([_vecs(1)], [7], [4])
    with pytest.raises(NotImplementedError, match="GF\\(2\\^521 - 1\\) only"):
        shamir.SecretShare(3, prime=(1 << 127) - 1).resolve_shares_vec_many([_vecs(3)], [1, 2, 3], [4])
    with pytest.raises(ValueError, match="^resolve_shares_vec_many: 1 share entries for 2 tensors$"):
        many([_vecs(3)], [1, 2, 3], [4, 4])
    with pytest.raises(ValueError, match='^resolve_shares_vec_many: out must be "int64" or "field"$'):
        many([_vecs(3)], [1, 2, 3], [4], out="bytes")


def test_the_checks_are_those_of_resolve_shares_vec():
    """Same exception type and message from both methods for each reference check."""
    ss = shamir.SecretShare(3)
    for k, xs in [(2, [1, 2]), (3, [1, 2, 2]), (3, [1, 2]), (0, [])]:
        with pytest.raises(ValueError) as one:
            ss.resolve_shares_vec(_vecs(k), xs, 4)
        with pytest.raises(ValueError) as many:
            ss.resolve_shares_vec_many([_vecs(k)], xs, [4])
        assert str(one.value) == str(many.value)
    s1 = shamir.SecretShare(1)
    with pytest.raises(TypeError) as one:
        s1.resolve_shares_vec(_vecs(1), [7], 4)
    with pytest.raises(TypeError) as many:
        s1.resolve_shares_vec_many([_vecs(1)], [7], [4])
    assert str(one.value) == str(many.value)


def test_scratch_bytes_grow_with_segments_and_k():
    L = _native.lib()
    sb = L.dn_m521_reconstruct_many_scratch_bytes
    for k in (2, 3, 16):
        for segs in (1, 17, 127, 65536):
            # the table's entries (tile range, n, three pointers) and k row addresses per segment
            assert sb(segs, k) >= 40 * (segs + 1) + 8 * k * segs
            assert sb(segs + 1, k) > sb(segs, k)
            assert sb(segs, k + 1) > sb(segs, k)


def test_entry_point_validates_before_any_device_call():
    """No vector with elements: DN_OK without touching a pointer; a malformed
    descriptor and more than 65536 vectors are refused as dn_m521_reconstruct does."""
    import ctypes

    L = _native.lib()
    w = _native.lagrange([1, 3, 5], 3)
    ns = (ctypes.c_uint64 * 3)(0, 0, 0)
    assert L.dn_m521_reconstruct_many(ns, None, None, None, None, 3, ctypes.byref(w), None, 0, None) == _native.DN_OK
    assert L.dn_m521_reconstruct_many(None, None, None, None, None, 0, ctypes.byref(w), None, 0, None) == _native.DN_OK
    assert (L.dn_m521_reconstruct_many(ns, None, None, None, None, 65537, ctypes.byref(w), None, 0, None)
            == _native.DN_ERR_ARG)
    assert "65536" in _native.last_error()
    bad = _native.lagrange([1, 3, 5], 3)
    bad.k = 17
    assert (L.dn_m521_reconstruct_many(ns, None, None, None, None, 3, ctypes.byref(bad), None, 0, None)
            == _native.DN_ERR_UNSUPPORTED)
    bad.k, bad.a_limbs = 3, 5
    assert (L.dn_m521_reconstruct_many(ns, None, None, None, None, 3, ctypes.byref(bad), None, 0, None)
            == _native.DN_ERR_ARG)
    one = (ctypes.c_uint64 * 1)(5)
    assert (L.dn_m521_reconstruct_many(one, None, None, None, None, 1, ctypes.byref(w), None, 0, None)
            == _native.DN_ERR_ARG)  # elements, but no share vectors


def test_tile_plan_against_per_element_map(tmp_path):
    """Every global tile and every wave-sched quarter of the ragged test list
    and of 1000 seeded random tables (sizes 0..700): each element visited
    exactly once, at its own (segment, local tile, word); no lane at or past
    n_k; the cursor equal to the binary search — by a stand-alone program under
    ASan + UBSan (not loaded into this process)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path / "recon_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "delta-node_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "recon_plan_check.cpp"), "-o", exe]
    # the sanitizer runtimes linked statically where the compiler can (the
    # program then runs whatever else the environment loads into processes)
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok"
