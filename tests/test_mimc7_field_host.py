"""The device arithmetic of the MiMC7 kernels, rehearsed on the host.

csrc/mimc7_field.hpp is the text the kernels compile (limb helpers, mont_mul,
mont_sqr, hash_m, arr_step, float_to_field).  A stand-alone program
(tests/host/mimc7_field_check.cpp) built with AddressSanitizer and
UndefinedBehaviorSanitizer — not loaded into this process — runs it over the
edge pools of tests/mimc7_edges.py, and every result is compared with Python
integers (oracle/py_mimc7.py), bit for bit:

* mul, sqr (of a lazy, unreduced sum, as in a hash round), hash and arr_step
  over pool x pool;
* raw_mul / raw_sqr on operands of the lazy form up to 3q - 1: a b R^-1 mod q,
  canonical, every column accumulator below 2^63 (asserted by the program);
* float_to_field over both float pools, at the reference's precisions 8 and
  21, and the values it must refuse.

The host chain (csrc/host_mimc7.cpp, a different conversion: exact for every
finite double) runs the same float pools against the oracle.
"""
import ctypes
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import mimc7_edges as me
from oracle import py_mimc7 as om

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = om.Q
RINV = pow(me.R, -1, Q)


@pytest.fixture(scope="module")
def field_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path_factory.mktemp("mimc7_field") / "mimc7_field_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "delta-node_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "mimc7_field_check.cpp"), "-o", exe]
    # the sanitizer runtimes linked statically where the compiler can (the
    # program then runs whatever else the environment loads into processes)
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr

    def run(lines):
        res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=110)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
        out = res.stdout.split()
        assert len(out) == len(lines)
        return out

    return run


def check(run, lines, want):
    got = run(lines)
    bad = [(ln, g, w) for ln, g, w in zip(lines, got, want) if g != w]
    assert not bad, f"{len(bad)} of {len(lines)} differ; first: {bad[:3]}"


def hx(v: int) -> str:
    return format(v, "064x")


def test_pool_is_what_the_tests_rely_on():
    pool = me.field_pool()
    assert len(pool) == len(set(pool)) and all(0 <= v < Q for v in pool)
    for v in [0, Q - 1, Q // 2, Q // 2 + 1, me.R % Q, me.R * me.R % Q, (1 << 29) - 1, 1 << 29, (1 << 32) - 1, 1 << 233,
              Q - (1 << 233) - 1, me.limb_ones(7), om.CTS[12], Q - om.CTS[12]]:
        assert v in pool, v
    assert len(me.merkle_partners()) == 16
    # round sums r + k + c_i that land exactly on 0 and on q are among the pairs
    assert all((Q - c) in pool for c in om.CTS if c)
    for scale in (1e8, 1e21, 1.0, 1e22):  # the coverage conditions are asserted inside
        assert len(me.float_pool(scale)) > 2000
        bad = me.bad_floats(scale)
        assert len(bad) == 6 and abs(me.product(me.good_neighbour(scale), scale)) < me.LIMIT


@pytest.mark.parametrize("op", ["mul", "sqr", "hash", "arr_step"])
def test_field_ops_pool_squared(field_check, op):
    pool = me.field_pool()
    want_of = {"mul": lambda a, b: a * b % Q, "sqr": lambda a, b: (a + b) * (a + b) % Q,
               "hash": lambda a, b: om.mimc7_hash(a, b) % Q, "arr_step": lambda a, b: om.mimc7_hash_arr([b], a)}[op]
    hexes = [hx(v) for v in pool]
    lines = [f"{op} {ha} {hb}" for ha in hexes for hb in hexes]
    want = [hx(want_of(a, b)) for a in pool for b in pool]
    check(field_check, lines, want)


def test_raw_products_of_lazy_operands(field_check):
    """Operands anywhere in [0, 3q): the result is a b R^-1 mod q, canonical, and
    no column accumulator reaches 2^63 (the program exits non-zero otherwise)."""
    pool = me.raw_pool()
    assert max(pool) == 3 * Q - 1
    hexes = [hx(v) for v in pool]
    lines = [f"raw_mul {ha} {hb}" for ha in hexes for hb in hexes] + [f"raw_sqr {ha}" for ha in hexes]
    want = [hx(a * b * RINV % Q) for a in pool for b in pool] + [hx(a * a * RINV % Q) for a in pool]
    check(field_check, lines, want)


def f2f_line(v: float, p: int) -> str:
    return f"f2f {struct.unpack('<Q', struct.pack('<d', v))[0]:016x} {p}"


@pytest.mark.parametrize("precision", [8, 21, 0, 22])
def test_float_to_field_pool_and_refusals(field_check, precision):
    scale = float(10 ** precision)
    pool, bad, good = me.float_pool(scale), me.bad_floats(scale), me.good_neighbour(scale)
    vals = pool + [good, -good]
    lines = [f2f_line(v, precision) for v in vals] + [f2f_line(v, precision) for v in bad]
    want = [hx(me.expected_field(v, precision)) for v in vals] + ["bad"] * len(bad)
    check(field_check, lines, want)


def test_host_chain_accepts_and_matches_on_both_float_pools():
    """calc_weight_commitment's host conversion is exact for every finite
    double: the pools and the finite members the device refuses."""
    from delta_node.crypto.shamir import _native
    from delta_node.utils import calc_weight_commitment, mimc7

    for scale in (1e8, 1e21):
        w = me.float_pool(scale) + [me.good_neighbour(scale)]
        w += [v for v in me.bad_floats(scale) if math.isfinite(v) and math.isfinite(me.product(v, 1e8))]
        assert calc_weight_commitment(w) == om.weight_commitment(w), scale
        for lo in range(0, len(w), 257):  # in chunks, so that a failure is localised
            part = w[lo:lo + 257]
            assert calc_weight_commitment(part) == om.weight_commitment(part), (scale, lo)
    # the label precision through the C entry point (the wrapper's is always 8)
    p = 21
    w = me.float_pool(1e21) + [v for v in me.bad_floats(1e21) if math.isfinite(me.product(v, 1e21))]
    arr = np.ascontiguousarray(w, dtype=np.float64)
    out = (ctypes.c_uint32 * 8)()
    _native.check(mimc7._lib().dn_mimc7_weight_commitment_host(arr.ctypes.data, arr.size, p, ctypes.addressof(out)))
    assert int.from_bytes(bytes(out), "little") == om.mimc7_hash_arr([om.float2int(float(v), p) for v in w], 2)
