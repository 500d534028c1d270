"""make_shares_vec_many on the host side (no kernel launches).

* the method and the three C entry points exist, and the reference's argument
  error fires before any device work;
* dn_mt19937_split_many_supported agrees with dn_mt19937_split_supported on
  the tensors' total, and refuses more than 65536 segments;
* the arithmetic that places a group's 64 elements in a list of share blocks
  (csrc/seg_plan.hpp, shared with the kernel) is checked against a per-element
  map by a stand-alone program (tests/host/many_plan_check.cpp) built with
  AddressSanitizer and UndefinedBehaviorSanitizer — the one place where a
  mistake would write outside a block, rehearsed before any GPU run.
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
    assert callable(getattr(shamir.SecretShare, "make_shares_vec_many"))
    L = _native.lib()
    for name in ("dn_mt19937_split_many_scratch_bytes", "dn_mt19937_split_many_supported",
                 "dn_mt19937_split_many_device"):
        assert hasattr(L, name), name
        assert name in _native.EXPORTS


def test_threshold_above_shares_raises_before_any_device_use():
    ss = shamir.SecretShare(3)
    with pytest.raises(ValueError, match="^threshold should be little equal than shares$"):
        ss.make_shares_vec_many([torch.arange(4, dtype=torch.int64), torch.arange(9, dtype=torch.int64)], 2)
    with pytest.raises(NotImplementedError, match="65535 shares and threshold 64"):
        ss.make_shares_vec_many([torch.arange(4, dtype=torch.int64)], 65536)
    with pytest.raises(NotImplementedError, match="65535 shares and threshold 64"):
        shamir.SecretShare(65).make_shares_vec_many([torch.arange(4, dtype=torch.int64)], 70)
    with pytest.raises(NotImplementedError, match="GF\\(2\\^521 - 1\\) only"):
        shamir.SecretShare(3, prime=(1 << 127) - 1).make_shares_vec_many([torch.arange(4, dtype=torch.int64)], 5)


@pytest.mark.parametrize("n_total,t,n", [(0, 3, 5), (1, 3, 5), (8861, 3, 5), (8861, 3, 7), (8861, 2, 3), (1704, 5, 9),
                                         (1 << 24, 3, 5), (1 << 40, 3, 5), (1000, 4, 5), (1000, 3, 2), (1000, 1, 1),
                                         (1000, 3, 65535), (1000, 5, 2000)])
def test_many_supported_agrees_with_split_supported(n_total, t, n):
    L = _native.lib()
    want = L.dn_mt19937_split_supported(n_total, t, n)
    for segments in (0, 1, 16, 65536):
        assert L.dn_mt19937_split_many_supported(n_total, t, n, segments) == want, segments


def test_many_supported_refuses_more_than_65536_segments():
    L = _native.lib()
    assert L.dn_mt19937_split_many_supported(1 << 20, 3, 5, 65536) == 1
    assert L.dn_mt19937_split_many_supported(1 << 20, 3, 5, 65537) == 0
    assert L.dn_mt19937_split_many_supported(1 << 20, 3, 5, 1 << 40) == 0


def test_many_scratch_holds_the_draw_and_the_segment_table():
    L = _native.lib()
    for n_total, tm1, segs in [(8861, 2, 16), (1 << 20, 2, 127), (1704, 4, 12)]:
        draw = L.dn_mt19937_device_scratch_bytes(n_total, tm1)
        assert L.dn_mt19937_split_many_scratch_bytes(n_total, tm1, segs) >= draw + 24 * (segs + 1)


def test_store_plan_against_per_element_map(tmp_path):
    """Every group of the ragged test list and of 1000 seeded random tables
    (sizes 0..700): each element stored exactly once, at its own (segment,
    tile, word); lane ranges disjoint; descriptors inside their rows — by a
    stand-alone program under ASan + UBSan (not loaded into this process)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path / "many_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "delta-node_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "many_plan_check.cpp"), "-o", exe]
    # the sanitizer runtimes linked statically where the compiler can (the
    # program then runs whatever else the environment loads into processes)
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok"
