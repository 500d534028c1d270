"""The share wire geometry (csrc/wire_geom.hpp) on the host side.

* a stand-alone program (tests/host/wire_geom_check.cpp) static_asserts the
  relations between the constants and prints their values; the values are what
  the Python tests assume: wire_edges.decode_window predicts which waves take
  the byte-serial path from DEC_WINDOW_LIMIT and MAX_RECORD
  (test_gpu_resolve_records.py, test_gpu_sum_records.py, test_gpu_codec_edges.py
  rely on it), and the frame tests build their edge lists from the scan shape
  and the frame block;
* every one of the constants, and every shared parse / emit / scan function,
  is defined in exactly one file under csrc/ — a kernel that restated one
  would no longer follow a fix made in the header.
"""
import glob
import os
import re
import shutil
import subprocess

import pytest

import test_frames_host
import wire_edges as we

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "delta-node_amd", "csrc")

GEOM = ("kMaxRecord", "kWinPad", "kDecWindow", "kWinLimit", "kDecRowWords", "kEncRowWords", "kStageQ", "kStageW",
        "kStageRegs", "kScanThreads", "kScanRun", "kScanStage", "kScanLdsWords")
FUNCS = ("win_of", "stage_load", "stage_store", "stage_direct", "parse_lds", "parse_global", "lds_order", "limb_bytes",
         "y_len", "lds_put_bytes", "lay_y", "flush_window", "scan_slot", "scan_block_totals", "scan_passes",
         "scan_count")


@pytest.fixture(scope="module")
def geom(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path_factory.mktemp("wire_geom") / "wire_geom_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC,
                            os.path.join(ROOT, "tests", "host", "wire_geom_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    return {name: int(value) for name, value in (line.split() for line in run.stdout.splitlines())}


def test_window_geometry_is_what_the_edge_suites_assume(geom):
    assert geom["kMaxRecord"] == we.MAX_RECORD == 1 + 8 + 66
    assert geom["kDecWindow"] == 64 * we.MAX_RECORD + 8
    assert geom["kWinLimit"] == we.DEC_WINDOW_LIMIT == 64 * we.MAX_RECORD + 8 + 12
    assert geom["kWinPad"] == 16
    assert geom["kMaxRecord"] <= 255  # a frame's u8 holds every record length


def test_scan_shape_is_what_the_frame_suites_assume(geom):
    assert (geom["kScanThreads"], geom["kScanRun"], geom["kScanStage"]) == (1024, 8, 8192)
    assert geom["kScanLdsWords"] == 8192 + 1024
    # the literals test_frames_host.py and test_gpu_frames.py read by text
    assert geom["kFrameBlock"] == test_frames_host.plan_constant("kFrameBlock")
    assert geom["kFrameWord"] == test_frames_host.plan_constant("kFrameWord")
    assert geom["kScanThreads"] == test_frames_host.plan_constant("kFrameScanThreads")
    assert geom["kScanRun"] == test_frames_host.plan_constant("kFrameScanRun")


def _sources():
    out = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if path.endswith((".hip", ".hpp", ".cpp", ".inc")):
            with open(path) as f:
                out[os.path.basename(path)] = f.read()
    return out


def test_every_constant_and_shared_function_is_defined_once():
    src = _sources()
    for name in GEOM:
        where = [f for f, text in src.items() if re.search(r"\bconstexpr\s+\w+\s+" + name + r"\s*=", text)]
        assert where == ["wire_geom.hpp"], (name, where)
    for name in FUNCS:
        # a definition or declaration: a return type, the name, an opening parenthesis, at the start of a statement
        pat = re.compile(r"^[ \t]*(?:template\s*<[^>]*>\s*)?(?:(?:__device__|__host__|__forceinline__|__noinline__|"
                         r"static|inline|constexpr|DN_WIRE_HD)\s+)+[\w:<>]+[\s*&]+" + name + r"\s*\(", flags=re.M)
        where = [f for f, text in src.items() if pat.search(text)]
        assert len(where) == 1 and where[0] in ("wire_geom.hpp", "wire_parse.hpp", "wire_emit.hpp"), (name, where)
    # the old names of the same things are gone
    for text in src.values():
        assert not re.search(r"\bkFrameMaxRecord\b|\bparse_record_global\b", text)
