"""Share commitments on the host side (no kernel launches).

* csrc/sha256_core.hpp — the text commit_sha256.hip compiles: rounds, rolling
  schedule, block count, padded-word rule — in a stand-alone program
  (tests/host/sha256_check.cpp) built with AddressSanitizer and
  UndefinedBehaviorSanitizer, not loaded into this process, against hashlib:
  FIPS 180-4's short vectors, every length 0..200, 5000 and 2^16 + 1 bytes;
* the model of tests/commit_edges.py holds what the GPU tests rely on;
* the two entry points are declared, exported and bound in codec's table;
* every argument error of commit_records_vec / verify_records_vec fires before
  any device use, valid CPU arguments reach the device requirement and go no
  further, and without a HIP device the calls raise (no CPU fallback);
* dn_sha256_commit_records / dn_sha256_verify_records validate before any
  device call.
"""
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import commit_edges as ce
import record_edges as re
from delta_node.crypto.shamir import _native, codec
from delta_node.utils import calc_commitment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8, I32, I64 = torch.uint8, torch.int32, torch.int64


# ------------------------------------------------------------------ the sanitised host program
@pytest.fixture(scope="module")
def sha_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path_factory.mktemp("sha256") / "sha256_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "delta-node_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "sha256_check.cpp"), "-o", exe]
    # the sanitizer runtimes linked statically where the compiler can (the
    # program then runs whatever else the environment loads into processes)
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr

    def run(messages):
        res = subprocess.run([exe], input="".join(m.hex() + "\n" for m in messages), capture_output=True, text=True,
                             timeout=110)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
        out = res.stdout.split()
        assert len(out) == len(messages)
        return out

    return run


def check(run, messages):
    got = run(messages)
    bad = [(len(m), g) for m, g in zip(messages, got) if g != hashlib.sha256(m).hexdigest()]
    assert not bad, f"{len(bad)} of {len(messages)} differ; first (length, digest): {bad[:3]}"


def test_fips_180_4_short_vectors(sha_check):
    msgs = [b"", b"abc", b"abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq"]
    assert len(msgs[2]) == 56
    assert sha_check(msgs) == [
        "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
        "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad",
        "248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1"]
    assert [calc_commitment(m).hex() for m in msgs] == sha_check(msgs)


def test_every_length_to_200_and_two_long_ones(sha_check):
    rng = np.random.default_rng(1)
    msgs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in list(range(201)) + [5000, (1 << 16) + 1]]
    msgs += [bytes([0xFF]) * n for n in (55, 56, 63, 64, 119, 120)] + [bytes(n) for n in (55, 56, 64)]
    check(sha_check, msgs)


# ------------------------------------------------------------------ the model
def test_the_crafted_wires_are_what_the_gpu_tests_assume():
    lengths = ce.phase_lengths()
    assert sorted(lengths) == sorted(list(range(131)) * 2) and len(lengths) == ce.N_PHASE == 262
    assert {ce.blocks_of(n) for n in lengths} == {1, 2, 3}
    assert [ce.blocks_of(n) for n in (55, 56, 119, 120, 67, 68, 75, ce.LONG)] == [1, 2, 2, 3, 2, 2, 2, 79]
    for shift in (0, 4, 8, 12):
        w = ce.phase_wire(shift)
        wins = w.windows()
        assert all(win.lds for win in wins) and len(wins) == 5
        assert all(win.Bend - win.A == 4160 for win in wins[:4])
        assert {int(o) % 4 for o in w.offsets[:-1]} == {0, 1, 2, 3}
        assert all(ok for ok, _ in ce.want_wire(w))
        s = ce.sorted_wire(shift)
        assert ce.serial_windows(s) == [2, 3] and all(ok for ok, _ in ce.want_wire(s))
        long = ce.long_wire(shift)
        assert ce.serial_windows(long) == [0] and long.windows()[1].lds
        assert int(long.offsets[18] - long.offsets[17]) == ce.LONG


def test_the_model_follows_the_header_rule():
    packed = bytes(range(200))
    off = [0, 10, 10, 30] + [30] * 60 + [40, 50]          # n = 65: one full wave and one record
    got = ce.want(packed, off, 200, 65, 16)
    assert all(ok for ok, _ in got) and got[1][1] == ce.sha(b"") and got[0][1] == ce.sha(packed[:10])
    assert got[64] == (True, ce.sha(packed[40:50]))
    # decreasing inside a usable window: that record and the one whose start now lies past its end
    bad = list(off)
    bad[2] = 5
    got = ce.want(packed, bad, 200, 65, 16)
    assert [ok for ok, _ in got[:4]] == [True, False, True, True] and got[1][1] == ce.ZERO
    # a window past the wire: every record of it, and only of it
    far = list(off)
    far[64] = 201
    got = ce.want(packed, far, 200, 65, 16)
    assert not any(ok for ok, _ in got[:64]) and not got[64][0]     # (record 64's window starts at 201 > its end)
    # the staging width never decides: the hostile tables give one answer at 16 and 4
    for name, w in re.hostile_offsets(16).items():
        assert [ok for ok, _ in ce.want_wire(w, 16)] == [ok for ok, _ in ce.want_wire(w, 4)], name


# ------------------------------------------------------------------ exports
def test_symbols_are_declared_exported_and_bound():
    for name in ("dn_sha256_commit_records", "dn_sha256_verify_records"):
        assert name in codec.EXPORTS
        assert hasattr(_native.lib(), name)
        assert getattr(codec._lib(), name).argtypes
    with open(os.path.join(ROOT, "include", "dn_commit.h")) as f:
        text = f.read()
    assert text.count("utils/commitment.py:5-12") >= 3  # the file's header and both entry points cite it
    assert callable(codec.commit_records_vec) and callable(codec.verify_records_vec)


# ------------------------------------------------------------------ argument errors
N = 4


def wire(n=N, **kw):
    return torch.zeros(80 * n, dtype=U8, **kw), torch.zeros(n + 1, dtype=I64, **kw)


def skewed(numel, by):
    buf = torch.zeros(numel + 128, dtype=U8)
    return buf[(-buf.data_ptr()) % 64 + by:][:numel]


def test_argument_errors_fire_before_any_device_use(monkeypatch):
    def no_device():
        raise AssertionError("reached the device before the argument checks")

    monkeypatch.setattr(_native, "require_device", no_device)
    monkeypatch.setattr(_native, "stream_ptr", no_device)
    p, o = wire()
    good_c = torch.zeros(N, 32, dtype=U8)
    commit, verify = codec.commit_records_vec, codec.verify_records_vec
    calls = {"commit_records_vec": lambda p_, o_, n_, **kw: commit(p_, o_, n_, **kw),
             "verify_records_vec": lambda p_, o_, n_, **kw: verify(p_, o_, n_, good_c, **kw)}
    for what, f in calls.items():
        with pytest.raises(ValueError, match=f"^{what}: n must not be negative$"):
            f(p, o, -1)
        for pp, oo, text in [(p.to(torch.int8), o, "packed records must be contiguous 1-D uint8"),       # dtype
                             (torch.zeros(640, dtype=U8)[::2], o, "packed records must be contiguous"),  # strided
                             (p.reshape(2, -1), o, "packed records must be contiguous 1-D uint8"),
                             (bytes(32), o, "packed records must be contiguous 1-D uint8"),
                             (p, o.to(I32), "offsets must be contiguous 1-D int64"),
                             (p, torch.zeros(10, dtype=I64)[::2], "offsets must be contiguous 1-D int64"),
                             (p, o[:N], "offsets must hold n \\+ 1 = 5 entries, got 4"),                  # short
                             (p.to("meta"), o, "must be on one device")]:
            with pytest.raises(ValueError, match=f"^{what}: .*" + text):
                f(pp, oo, N)
        for bad in (torch.zeros(1, dtype=I32), torch.zeros(3, dtype=I32), torch.zeros(2, dtype=I64),
                    torch.zeros(4, dtype=I32)[::2], [0, 0], torch.zeros(2, dtype=I32, device="meta")):
            with pytest.raises(ValueError, match=f"^{what}: bad must be a contiguous int32 tensor \\[2\\]"):
                f(p, o, N, bad=bad)
    # commit: out
    for out in (torch.zeros(32 * N - 1, dtype=U8), torch.zeros(32 * N, dtype=torch.int8),
                torch.zeros(64 * N, dtype=U8)[::2], torch.zeros(32 * N, dtype=U8, device="meta")):
        with pytest.raises(ValueError, match="^commit_records_vec out: expected a contiguous torch.uint8 tensor of "
                                             ">= 128 elements"):
            commit(p, o, N, out=out)
    for by in (1, 2, 3):
        with pytest.raises(ValueError, match="^commit_records_vec out: the buffer must be 4-byte aligned"):
            commit(p, o, N, out=skewed(32 * N, by))
    arena = torch.zeros(1024, dtype=U8)
    for pp, out in [(arena[:320], arena[316:316 + 128]), (arena[128:448], arena[:132]), (arena[:320], arena[:128]),
                    (arena[64:384], arena[128:256])]:
        with pytest.raises(ValueError, match="^commit_records_vec: out overlaps packed$"):
            commit(pp, o, N, out=out)
    # verify: commitments, ok
    for c in (torch.zeros(N, 31, dtype=U8), torch.zeros(32 * N + 1, dtype=U8), torch.zeros(N - 1, 32, dtype=U8),
              torch.zeros(N, 32, dtype=torch.int8), torch.zeros(N, 64, dtype=U8)[:, ::2], torch.zeros(32, N, dtype=U8),
              bytes(32 * N), torch.zeros(N, 32, dtype=U8, device="meta")):
        with pytest.raises(ValueError, match="^verify_records_vec: commitments must be a contiguous uint8 tensor "
                                             "\\[4, 32\\] or \\[128\\] on the records' device$"):
            verify(p, o, N, c)
    for ok in (torch.zeros(N - 1, dtype=U8), torch.zeros(N, dtype=torch.bool), torch.zeros(2 * N, dtype=U8)[::2]):
        with pytest.raises(ValueError, match="^verify_records_vec ok: expected a contiguous torch.uint8 tensor of "
                                             ">= 4 elements"):
            verify(p, o, N, good_c, ok=ok)
    with pytest.raises(ValueError, match="^verify_records_vec: ok overlaps packed$"):
        verify(arena[:320], o, N, good_c, ok=arena[319:323])


def test_the_device_is_required_only_after_the_checks(monkeypatch):
    class Reached(Exception):
        pass

    def reached():
        raise Reached

    monkeypatch.setattr(_native, "require_device", reached)
    monkeypatch.setattr(_native, "stream_ptr", lambda: pytest.fail("launched"))
    p, o = wire()
    flag = torch.zeros(2, dtype=I32)
    with pytest.raises(Reached):
        codec.commit_records_vec(p, o, N, out=torch.zeros(32 * N + 7, dtype=U8), bad=flag)
    with pytest.raises(Reached):
        codec.commit_records_vec(p, o, N, out=torch.zeros(N, 32, dtype=U8))
    with pytest.raises(Reached):
        codec.verify_records_vec(p, o, N, torch.zeros(32 * N, dtype=U8), ok=torch.zeros(N, dtype=U8), bad=flag)
    with pytest.raises(Reached):  # n = 0 still asks for the device its empty result lives on
        codec.commit_records_vec(*wire(0), 0)
    with pytest.raises(Reached):
        codec.verify_records_vec(*wire(0), 0, torch.zeros(0, 32, dtype=U8))


def test_without_a_device_the_calls_raise(monkeypatch):
    """No CPU fallback: valid arguments, no HIP device -> RuntimeError."""
    monkeypatch.setattr(_native, "_HAS_DEVICE", False)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    p, o = wire()
    with pytest.raises(RuntimeError, match="no HIP device visible"):
        codec.commit_records_vec(p, o, N)
    with pytest.raises(RuntimeError, match="no HIP device visible"):
        codec.verify_records_vec(p, o, N, torch.zeros(N, 32, dtype=U8))


def test_a_wire_on_another_device_is_refused(monkeypatch):
    monkeypatch.setattr(_native, "require_device", lambda: torch.device("meta"))
    with pytest.raises(ValueError, match="^commit_records_vec: records must be on meta$"):
        codec.commit_records_vec(*wire(), N)


def test_check_bad_commit_names_both_counts():
    codec.check_bad_commit(torch.zeros(2, dtype=I32))
    with pytest.raises(ValueError, match="^verify_records_vec: 3 records whose offsets leave their window, "
                                         "4 records whose SHA-256 is not their commitment$"):
        codec.check_bad_commit(torch.tensor([3, 4], dtype=I32))
    with pytest.raises(ValueError, match="^commit_records_vec: 1 records whose offsets leave their window, 0 "):
        codec.check_bad_commit(torch.tensor([1, 0], dtype=I32), what="commit_records_vec")


# ------------------------------------------------------------------ the entry points
def test_entry_points_validate_before_any_device_call():
    L = codec._lib()
    commit, verify = L.dn_sha256_commit_records, L.dn_sha256_verify_records
    OK, ARG = _native.DN_OK, _native.DN_ERR_ARG
    base = 0x7F0000000000  # never dereferenced: every call below returns before a launch
    inp, off, dig, okp, bad = base, base + (1 << 20), base + (2 << 20), base + (3 << 20), base + (4 << 20)
    nbytes, n = 4096, 50
    # n == 0: DN_OK whatever else is passed, no pointer touched
    assert commit(None, 0, None, 0, None, None, None) == OK
    assert verify(None, 0, None, 0, None, None, None, None) == OK
    assert commit(1, 5, 3, 0, 2, 1, None) == OK
    # null pointers (ok may be null)
    for args in [(None, nbytes, off, n, dig, bad), (inp, nbytes, None, n, dig, bad), (inp, nbytes, off, n, None, bad),
                 (inp, nbytes, off, n, dig, None)]:
        assert commit(*args, None) == ARG
        assert "dn_sha256_commit_records: null pointer" in _native.last_error()
    for args in [(None, nbytes, off, n, dig, okp, bad), (inp, nbytes, None, n, dig, okp, bad),
                 (inp, nbytes, off, n, None, okp, bad), (inp, nbytes, off, n, dig, None, None)]:
        assert verify(*args, None) == ARG
        assert "dn_sha256_verify_records: null pointer" in _native.last_error()
    # alignment
    for skew in (1, 2, 3):
        assert commit(inp + skew, nbytes, off, n, dig, bad, None) == ARG
        assert "in must be 4-byte aligned" in _native.last_error()
        assert commit(inp, nbytes, off, n, dig + skew, bad, None) == ARG
        assert "digests must be 4-byte aligned" in _native.last_error()
        assert verify(inp, nbytes, off, n, dig + skew, okp, bad, None) == ARG
        assert "expect must be 4-byte aligned" in _native.last_error()
    for skew in (1, 4):
        assert commit(inp, nbytes, off + skew, n, dig, bad, None) == ARG
        assert "offsets must be 8-byte aligned" in _native.last_error()
        assert verify(inp, nbytes, off + skew, n, dig, None, bad, None) == ARG
    # 2^31 workgroups or more
    for f, tail in ((commit, (dig, bad, None)), (verify, (dig, None, bad, None))):
        assert f(inp, nbytes, off, 256 << 31, *tail) == ARG
        assert "2^31" in _native.last_error()
        assert f(inp, nbytes, off, (256 << 31) - 255, *tail) == ARG
    # outputs overlapping the wire
    for d in (inp, inp + nbytes - 4, inp - 32 * n + 4):
        assert commit(inp, nbytes, off, n, d, bad, None) == ARG
        assert "digests overlaps in" in _native.last_error()
    for k in (inp, inp + nbytes - 1, inp - n + 1):
        assert verify(inp, nbytes, off, n, dig, k, bad, None) == ARG
        assert "ok overlaps in" in _native.last_error()
