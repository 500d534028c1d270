"""csrc/m521_device.hpp and csrc/chacha_device.hpp, operation by operation,
on the host.

The two headers are the arithmetic every Shamir kernel compiles.  Here they
compile unchanged for the host against a small stand-in for
<hip/hip_runtime.h> (tests/host/hip_shim), inside a stand-alone program
(tests/host/opcheck_host.cpp over csrc/opcheck_ops.hpp) built with
AddressSanitizer and UndefinedBehaviorSanitizer and run as a child process.
Every case comes from tests/device_ops.py and every result is compared with
Python integers there, bit for bit.  test_gpu_device_ops.py runs the same
sections on the device.

What only this file can do: prng_retry (odds 2^-520 in a real draw), a
carry ripple of every length, every odd divisor below 2^16, all 31 x 521
rotations, and store_reduced with the wave's ballot forced either way.
"""
import os
import shutil
import subprocess
import time

import pytest

import device_ops as do
import field_edges as fe
from field_edges import P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """Build the checker, run every section through it once: name -> out bytes."""
    cxx = os.environ.get("HOSTCXX") or "/opt/rocm/llvm/bin/clang++"
    if not (os.path.isfile(cxx) or shutil.which(cxx)):
        cxx = shutil.which("clang++")
    assert cxx, "no clang++ (the headers use __builtin_addc / __builtin_subc)"
    tmp = tmp_path_factory.mktemp("opcheck")
    exe = str(tmp / "opcheck_host")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "tests", "host", "hip_shim"), "-I", os.path.join(ROOT, "delta-node_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "opcheck_host.cpp"), "-o", exe]
    # the sanitizer runtimes linked statically where the compiler can (the
    # program then runs whatever else the environment loads into processes)
    build = subprocess.run(cmd + ["-static-libsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]

    secs = list(do.sections())
    secs += [do.sec_store_reduced("store_reduced", flags=1), do.sec_store_reduced("store_reduced_at", flags=1)]
    cases, out = str(tmp / "cases.bin"), str(tmp / "results.bin")
    with open(cases, "wb") as f:
        for s in secs:
            f.write(s.header())
            f.write(s.records)
    t0 = time.perf_counter()
    res = subprocess.run([exe, cases, out], capture_output=True, text=True, timeout=300)
    dt = time.perf_counter() - t0
    print(f"opcheck_host: {res.stdout.strip()} in {dt:.1f} s")
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert res.stdout.split()[-2:] == ["out_of_descriptor", "0"], res.stdout
    got, o = {}, 0
    with open(out, "rb") as f:
        blob = f.read()
    os.remove(cases)
    os.remove(out)
    for s in secs:
        nb = 4 * s.ow * len(s.cases)
        got[s.name] = (s, blob[o:o + nb])
        o += nb
    assert o == len(blob)
    return got


# ------------------------------------------------------------------ the census, from Python alone
def test_lazy_values_reach_every_rare_branch():
    vals = do.lazy_values()
    c = do.census(vals)
    for name in fe.PREDICATES:
        assert c[name] >= 16, (name, c[name])
    assert all(c["ripple"][k] >= 2 for k in range(1, 17)), c["ripple"]
    # limb 16 at 0x1FF under a carry of every length, 16 included (the carry then sets bit 521)
    for k in range(1, 17):
        assert any(do.ripple_len(v) == k and (v >> 512) & 0x1FF == 0x1FF for v in vals), k
    for m in (1, 2, 3, 1 << 22, (1 << 23) - 1):
        assert m * P in vals
    for v in [(1 << 544) - 1, P - 1, P, P + 1, (1 << 521) + (1 << 23) - 1, 0] + fe.edge_values():
        assert v in vals


def test_store_reduced_layout_has_every_kind_of_wave():
    lay = do.store_reduced_layout()
    c = do.wave_census(lay)
    assert c["none"] >= 2 and c["all"] >= 2 and c["only0"] == 1 and c["only63"] == 1 and c["only_mid"] == 1, c
    assert sorted(v for v, _ in lay) == sorted(do.lazy_values())
    assert {w for _, w in lay} >= set(do.W_SET)


def test_sweeps_are_complete():
    rot = do.section("rotr521").cases
    assert {(e, k) for e in range(1, 32) for k in range(521)} <= {(e, v.bit_length() - 1) for v, e in rot
                                                                  if v and v & (v - 1) == 0}
    div = do.section("exact_div_small-sweep").cases
    assert {d for _, d in div} == set(range(3, 65536, 2))
    per_d = {}
    for r, d in div:
        per_d.setdefault(d, []).append(r)
    assert all(len(rs) == 8 and {0, 1, d, P - d, P - 1} <= set(rs) and rs[5] % d == 0 for d, rs in per_d.items())
    ds = do.descriptor_divisors()
    assert {3, 15, 5, 7, 45, 315} <= set(ds) and all(3 <= d < 65536 and d & 1 for d in ds)
    # the divisor of every abscissa set the rest of the suite uses is among them
    for xs in ([1, 2, 3], [1, 3, 5], [2, 4, 5, 7], list(range(1, 9)), list(range(1, 17))):
        w = fe.desc_from_xs(xs)
        if w.has_inv == 2:
            assert w.d in ds, xs
    counts = {}
    for _, d in do.section("exact_div_small-descriptors").cases:
        counts[d] = counts.get(d, 0) + 1
    assert counts == {d: do.DIV_RANDOM_R for d in ds}
    mods = {d for _, d in do.section("mod_small").cases}
    assert set(do.MOD_D) <= mods
    assert {T: fe.fd_max_n(T) for T in range(2, 8)} == {2: 65535, 3: 2892, 4: 198, 5: 48, 6: 18, 7: 7}
    assert [c[1] for c in do.section("mul_small_add").cases if c[1] in do.MSA_X]


def test_retry_draws_are_accepted_and_the_boundary_is_met():
    """Each expected redraw is itself accepted (so attempt 0 is the one the
    device must return); second and later attempts stay unreachable."""
    sec = do.section("prng_retry")
    assert len(sec.cases) == 3 * 2 * len(do.RETRY_I)
    assert all(c[4] < P - 1 for c in sec.cases)
    rej = do.section("prng_rejected").cases
    assert P - 2 in rej and P - 1 in rej and P in rej


def test_record_widths_are_the_headers():
    """device_ops.OPS restates csrc/opcheck_ops.hpp: ids in enum order."""
    src = open(os.path.join(ROOT, "delta-node_amd", "csrc", "opcheck_ops.hpp")).read()
    enum = src[src.index("enum Op"):src.index("kOpCount")]
    names = [t.split("=")[0].strip() for t in enum[enum.index("{") + 1:].replace("\n", " ").split(",") if t.strip()]
    assert len(names) == len(do.OPS) and [i for i, _, _ in do.OPS.values()] == list(range(len(names)))
    assert set(do.section_names()) == {s.name for s in do.sections()}
    assert {s.op for s in do.sections()} == set(do.OPS)


# ------------------------------------------------------------------ the checker's results
@pytest.mark.parametrize("name", do.section_names() + ["store_reduced+ballot", "store_reduced_at+ballot"])
def test_host_op(results, name):
    sec, out = results[name]
    sec.check(out)


def test_forced_ballot_stores_the_same_value(results):
    """store_reduced with another lane rare: the same bytes in the tile, and D
    reduced in place where the lane alone would have left it."""
    for op in ("store_reduced", "store_reduced_at"):
        (sec, off), (_, on) = results[op], results[op + "+ballot"]
        ob = 4 * sec.ow
        changed = 0
        for i, (D, _) in enumerate(sec.cases):
            a, b = off[i * ob:(i + 1) * ob], on[i * ob:(i + 1) * ob]
            assert a[:do.TILE_BYTES] == b[:do.TILE_BYTES], (op, i)
            assert do.fe_at(b, do.TILE_WORDS) == D % P
            changed += do.fe_at(a, do.TILE_WORDS) != do.fe_at(b, do.TILE_WORDS)
        assert changed >= 16, changed
