"""Share wire frames on the host side (no kernel launches).

* the five entry points exist and are listed in codec.EXPORTS (so
  test_host.py::test_library_exports_header_symbols stays green);
* R(n) and the capacity against the formula of include/dn_shamir.h;
* every argument error of encode_share_frame, encode_frames_many and
  open_frames fires before any device use (CPU tensors, no HIP device needed),
  and valid CPU arguments reach the device requirement and go no further;
* dn_m521_frame_finish / dn_m521_frame_open validate before any device call
  (never-dereferenced addresses);
* frame_fields_host round-trips a frame built in numpy from golden F1's
  reference share bytes and rejects each single-field corruption;
* the index arithmetic of csrc/frame_plan.hpp replayed on a model of memory by
  a stand-alone program (tests/host/frame_plan_check.cpp) built with
  AddressSanitizer and UndefinedBehaviorSanitizer (not loaded into this
  process).
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from delta_node.crypto.shamir import _native, codec, field
from golden.fixtures import load_npz, manifest, unpack_share_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dn_m521_frame_records_offset", "dn_m521_frame_capacity", "dn_m521_frame_finish",
         "dn_m521_frame_scratch_bytes", "dn_m521_frame_open")


def plan_constant(name: str) -> int:
    """A literal constant of csrc/frame_plan.hpp."""
    with open(os.path.join(ROOT, "delta-node_amd", "csrc", "frame_plan.hpp")) as f:
        found = re.findall(r"^constexpr \w+ " + name + r" = (\d+);", f.read(), flags=re.M)
    assert len(found) == 1, (name, found)
    return int(found[0])


def group() -> int:
    with open(os.path.join(ROOT, "include", "dn_shamir.h")) as f:
        found = re.findall(r"^#define DN_M521_FRAME_GROUP (\d+)$", f.read(), flags=re.M)
    assert len(found) == 1, found
    return int(found[0])


def R(n: int) -> int:
    return 32 + 16 * ((n + 15) // 16)


def xlen(x: int) -> int:
    return (x.bit_length() + 7) // 8


def test_entry_points_exist_and_are_exported():
    L = _native.lib()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in codec.EXPORTS, name
    for f in ("frame_records_offset", "frame_capacity", "encode_share_frame", "encode_frames_many", "open_frames",
              "open_frame", "check_bad_frames", "frame_fields_host"):
        assert callable(getattr(codec, f)), f
    assert group() == 64


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 1 << 24])
def test_records_offset_and_capacity_against_the_formula(n):
    assert codec.frame_records_offset(n) == R(n)
    assert R(n) % 16 == 0 and R(n) >= 32 + n and R(n) < 32 + n + 16
    for x in (0, 1, 3, 255, 256, (1 << 64) - 1):
        assert codec.encoded_capacity(n, x) == n * (1 + xlen(x) + 66)
        assert codec.frame_capacity(n, x) == R(n) + n * (1 + xlen(x) + 66)
    B = plan_constant("kFrameBlock") * plan_constant("kFrameWord")
    assert _native.lib().dn_m521_frame_scratch_bytes(n, 3) == 3 * 8 * (n // B + 1)


# ---------------------------------------------------------------- argument errors, no device
def _no_device(monkeypatch, what):
    def no_device():
        raise AssertionError(f"{what} reached the device before its argument checks")

    monkeypatch.setattr(_native, "require_device", no_device)
    monkeypatch.setattr(_native, "stream_ptr", no_device)


def test_encode_share_frame_argument_errors_fire_before_any_device_use(monkeypatch):
    _no_device(monkeypatch, "encode_share_frame")
    vb = field.vec_bytes(4)
    vec = torch.zeros(vb, dtype=torch.uint8)
    with pytest.raises(ValueError, match="encode_share_frame: n must not be negative"):
        codec.encode_share_frame(vec, -1, 1)
    for x in (-1, 1 << 64):
        with pytest.raises(NotImplementedError, match="encode_share_frame: x must fit 64 bits"):
            codec.encode_share_frame(vec, 4, x)
    for bad in (vec[:-1], vec.to(torch.int8), torch.zeros(2 * vb, dtype=torch.uint8)[::2], bytes(vb)):
        with pytest.raises(ValueError, match=f"encode_share_frame: vec must be a contiguous uint8 tensor of >= {vb}"):
            codec.encode_share_frame(bad, 4, 1)
    for out in (torch.zeros(4096, dtype=torch.int8), torch.zeros(8192, dtype=torch.uint8)[::2], bytes(4096),
                torch.zeros(4096, dtype=torch.uint8, device="meta")):
        with pytest.raises(ValueError, match="encode_share_frame out: expected a contiguous torch.uint8 tensor"):
            codec.encode_share_frame(vec, 4, 1, out=out)
    for offs in (torch.zeros(5, dtype=torch.int32), torch.zeros(10, dtype=torch.int64)[::2], [0] * 5):
        with pytest.raises(ValueError, match="encode_share_frame offsets: expected a contiguous torch.int64 tensor"):
            codec.encode_share_frame(vec, 4, 1, offsets=offs)


def _blocks(ns, S=3):
    return [torch.zeros(S, field.vec_bytes(n), dtype=torch.uint8) for n in ns]


def test_encode_frames_many_has_encode_shares_manys_errors(monkeypatch):
    _no_device(monkeypatch, "encode_frames_many")
    f = codec.encode_frames_many
    ns = [5, 0, 300]
    with pytest.raises(ValueError, match="^encode_frames_many: 3 blocks for 2 sizes$"):
        f(_blocks(ns), ns[:2])
    with pytest.raises(ValueError, match="encode_frames_many: negative element count"):
        f(_blocks(ns), [5, -1, 300])
    with pytest.raises(ValueError, match="encode_frames_many: block 1 must be a contiguous uint8 tensor"):
        f([_blocks(ns)[0], torch.zeros(3, 7, dtype=torch.uint8), _blocks(ns)[2]], ns)
    with pytest.raises(ValueError, match="encode_frames_many: block 2 has 2 rows on cpu, block 0 has 3 on cpu"):
        f(_blocks(ns)[:2] + _blocks([300], S=2), ns)
    with pytest.raises(ValueError, match="encode_frames_many: rows without xs"):
        f(_blocks(ns), ns, rows=[0])
    for x in (-1, 1 << 64):
        with pytest.raises(NotImplementedError, match="encode_frames_many: x must fit 64 bits"):
            f(_blocks(ns), ns, [1, x])
    with pytest.raises(ValueError, match="encode_frames_many: 1 rows for 2 abscissas"):
        f(_blocks(ns), ns, [1, 2], rows=[0])
    with pytest.raises(ValueError, match="encode_frames_many: rows must lie in \\[0, 3\\)"):
        f(_blocks(ns), ns, [1, 2], rows=[0, 3])
    with pytest.raises(ValueError, match="encode_frames_many: 1 outs for 2 abscissas"):
        f(_blocks(ns), ns, [1, 2], outs=[torch.zeros(8, dtype=torch.uint8)])
    with pytest.raises(ValueError, match="encode_frames_many: 3 offsets for 2 abscissas"):
        f(_blocks(ns), ns, [1, 2], offsets=[torch.zeros(400, dtype=torch.int64)] * 3)
    with pytest.raises(ValueError, match="encode_frames_many: the blocks must be on a HIP device"):
        f(_blocks(ns), ns)
    assert f(_blocks(ns), ns, []) == []


def _frame(n=4, **kw):
    return torch.zeros(R(n) + 8 * n, dtype=torch.uint8, **kw)


def test_open_frames_argument_errors_fire_before_any_device_use(monkeypatch):
    _no_device(monkeypatch, "open_frames")
    f = codec.open_frames
    with pytest.raises(ValueError, match="^open_frames: no frames$"):
        f([], 4, [])
    for bad in (_frame().to(torch.int8), torch.zeros(200, dtype=torch.uint8)[::2], _frame().reshape(2, -1),
                bytes(64)):
        with pytest.raises(ValueError, match="open_frames: frames must be contiguous 1-D uint8 tensors"):
            f([_frame(), bad], 4, [1, 2])
    with pytest.raises(ValueError, match="open_frames: every frame must be on one device"):
        f([_frame(), _frame(device="meta")], 4, [1, 2])
    with pytest.raises(ValueError, match="open_frames: n must not be negative"):
        f([_frame()], -1, [1])
    with pytest.raises(ValueError, match="open_frames: 1 abscissas for 2 frames"):
        f([_frame(), _frame()], 4, [1])
    for x in (-1, 1 << 64):
        with pytest.raises(ValueError, match="open_frames: x must fit 64 bits"):
            f([_frame()], 4, [x])
    with pytest.raises(ValueError, match="open_frames: 2 offsets for 1 frames"):
        f([_frame()], 4, [1], offsets=[torch.zeros(5, dtype=torch.int64)] * 2)
    for offs in (torch.zeros(5, dtype=torch.int32), torch.zeros(10, dtype=torch.int64)[::2], [0] * 5,
                 torch.zeros(5, dtype=torch.int64, device="meta")):
        with pytest.raises(ValueError, match="open_frames: offsets must be contiguous 1-D int64 tensors"):
            f([_frame()], 4, [1], offsets=[offs])
    with pytest.raises(ValueError, match="open_frames: offsets must hold n \\+ 1 = 5 entries, got 4"):
        f([_frame()], 4, [1], offsets=[torch.zeros(4, dtype=torch.int64)])
    for bad in (torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64),
                torch.zeros(4, dtype=torch.int32)[::2], [0, 0], torch.zeros(2, dtype=torch.int32, device="meta")):
        with pytest.raises(ValueError, match="open_frames: bad must be a contiguous int32 tensor \\[2\\]"):
            f([_frame()], 4, [1], bad=bad)
    with pytest.raises(ValueError, match="open_frames: frame 1 has 47 bytes, fewer than the 48 before its records"):
        f([_frame(), torch.zeros(47, dtype=torch.uint8)], 4, [1, 2])
    with pytest.raises(ValueError, match="open_frames: frames must be contiguous"):  # open_frame is open_frames
        codec.open_frame(bytes(64), 4, 1)


def test_the_device_is_required_only_after_the_checks(monkeypatch):
    """Valid CPU arguments get as far as the device requirement, and no further."""
    class Reached(Exception):
        pass

    def reached():
        raise Reached

    monkeypatch.setattr(_native, "require_device", reached)
    monkeypatch.setattr(_native, "stream_ptr", lambda: pytest.fail("launched"))
    with pytest.raises(Reached):
        codec.encode_share_frame(torch.zeros(field.vec_bytes(4), dtype=torch.uint8), 4, 3, trim=False,
                                 out=torch.zeros(4096, dtype=torch.uint8),
                                 offsets=torch.zeros(5, dtype=torch.int64))
    with pytest.raises(Reached):
        codec.open_frames([_frame(), _frame()], 4, [1, 2], offsets=[torch.zeros(5, dtype=torch.int64)] * 2,
                          bad=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(Reached):
        codec.open_frames([_frame()], None, None)
    with pytest.raises(Reached):  # an empty list has no device of its own
        codec.encode_frames_many([], [], [1, 2])


def test_check_bad_frames_names_both_counts():
    codec.check_bad_frames(torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="^open_frames: 2 frames whose header is not \\(magic, n, x, records_bytes\\), "
                                         "1 frames whose lengths do not sum to their records' bytes$"):
        codec.check_bad_frames(torch.tensor([2, 1], dtype=torch.int32))
    with pytest.raises(ValueError, match="^open_frames: 0 frames whose header .*, 3 frames whose lengths"):
        codec.check_bad_frames(torch.tensor([0, 3], dtype=torch.int32))


# ---------------------------------------------------------------- the entry points
def test_entry_points_validate_before_any_device_call():
    codec.frame_records_offset(0)  # binds the argument types
    L = _native.lib()
    fin, opn = L.dn_m521_frame_finish, L.dn_m521_frame_open
    OK, ARG = _native.DN_OK, _native.DN_ERR_ARG
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    base = 0x7F0000000000  # never dereferenced: every call below returns before a launch
    bad, scratch = base + (24 << 20), base + (32 << 20)
    G = group()

    def ptrs(*p):
        return (vp * len(p))(*p)

    def u64s(*v):
        return (u64 * len(v))(*v)

    offs = ptrs(base + (1 << 20), base + (2 << 20), base + (3 << 20))
    frames = ptrs(base, base + 4096, base + 8192)
    xs, nb = u64s(1, 2, 3), u64s(4096, 4096, 4096)
    n = 5
    # --- finish
    assert fin(offs, frames, xs, 0, n, None) == ARG and "no wire" in _native.last_error()
    for args in [(None, frames, xs), (offs, None, xs), (offs, frames, None)]:
        assert fin(*args, 3, n, None) == ARG and "null pointer" in _native.last_error()
    assert fin(ptrs(base, None, base), frames, xs, 3, n, None) == ARG and "null wire 1" in _native.last_error()
    assert fin(offs, ptrs(base, base, None), xs, 3, n, None) == ARG and "null wire 2" in _native.last_error()
    for skew in (1, 4, 8, 15):
        assert fin(offs, ptrs(base, base + 4096 + skew, base + 8192), xs, 3, n, None) == ARG
        assert "frame of wire 1 must be 16-byte aligned" in _native.last_error()
    for skew in (1, 4):
        assert fin(ptrs(base, base, base + skew), frames, xs, 3, n, None) == ARG
        assert "offsets of wire 2 must be 8-byte aligned" in _native.last_error()
    # a wire at fault beyond the first launch's group is still found before anything is launched
    many_f = ptrs(*([base] * (G + 1) + [base + 4]))
    many_o = ptrs(*([base + (1 << 20)] * (G + 2)))
    assert fin(many_o, many_f, u64s(*range(G + 2)), G + 2, n, None) == ARG
    assert f"frame of wire {G + 1} must be 16-byte aligned" in _native.last_error()
    for big in (256 << 31, (256 << 31) - 255):
        assert fin(offs, frames, xs, 3, big, None) == ARG and "2^31" in _native.last_error()
    # --- open
    oo = ptrs(base + (4 << 20), base + (5 << 20), base + (6 << 20))
    sb = L.dn_m521_frame_scratch_bytes(n, 3)
    assert opn(frames, nb, xs, 0, n, oo, bad, scratch, sb, None) == ARG and "no frame" in _native.last_error()
    for args in [(None, nb, xs, 3, n, oo, bad, scratch), (frames, None, xs, 3, n, oo, bad, scratch),
                 (frames, nb, None, 3, n, oo, bad, scratch), (frames, nb, xs, 3, n, None, bad, scratch),
                 (frames, nb, xs, 3, n, oo, None, scratch), (frames, nb, xs, 3, n, oo, bad, None)]:
        assert opn(*args, sb, None) == ARG and "null pointer" in _native.last_error()
    assert opn(ptrs(base, None, base), nb, xs, 3, n, oo, bad, scratch, sb, None) == ARG
    assert "null frame 1" in _native.last_error()
    assert opn(frames, nb, xs, 3, n, ptrs(base, base, None), bad, scratch, sb, None) == ARG
    assert "null frame 2" in _native.last_error()
    for skew in (1, 4, 8, 15):
        assert opn(ptrs(base, base + 4096 + skew, base), nb, xs, 3, n, oo, bad, scratch, sb, None) == ARG
        assert "frame 1 must be 16-byte aligned" in _native.last_error()
    for skew in (1, 4):
        assert opn(frames, nb, xs, 3, n, ptrs(base, base, base + skew), bad, scratch, sb, None) == ARG
        assert "offsets of frame 2 must be 8-byte aligned" in _native.last_error()
    assert opn(frames, u64s(4096, R(n) - 1, 4096), xs, 3, n, oo, bad, scratch, sb, None) == ARG
    assert f"frame 1 has {R(n) - 1} bytes, fewer than the {R(n)} before its records" in _native.last_error()
    assert opn(frames, nb, xs, 3, n, oo, bad, scratch, sb - 1, None) == ARG
    assert "scratch too small" in _native.last_error()
    assert opn(frames, nb, xs, 3, n, oo, bad, scratch + 4, sb, None) == ARG
    assert "scratch must be 8-byte aligned" in _native.last_error()
    big_nb = u64s(*[1 << 62] * 3)
    for big in (256 << 31, (256 << 31) - 255):
        assert opn(frames, big_nb, xs, 3, big, oo, bad, scratch, 1 << 62, None) == ARG and "2^31" in _native.last_error()
    many = ptrs(*([base] * (G + 1) + [base + 8]))
    many_oo = ptrs(*([base + (4 << 20)] * (G + 2)))
    assert opn(many, u64s(*[4096] * (G + 2)), u64s(*range(G + 2)), G + 2, n, many_oo, bad, scratch,
               L.dn_m521_frame_scratch_bytes(n, G + 2), None) == ARG
    assert f"frame {G + 1} must be 16-byte aligned" in _native.last_error()
    assert OK == 0


# ---------------------------------------------------------------- frame_fields_host
def host_frame(x: int, recs, n=None) -> np.ndarray:
    """A frame built in numpy from records: header, lens, pad, records."""
    n = len(recs) if n is None else n
    body = b"".join(recs)
    head = codec.FRAME_MAGIC + np.array([n, x, len(body)], dtype="<u8").tobytes()
    lens = bytes(len(r) for r in recs)
    return np.frombuffer(head + lens + bytes(R(n) - 32 - len(recs)) + body, dtype=np.uint8).copy()


@pytest.fixture(scope="module")
def f1_records():
    cfg = manifest()["f1"]
    z = load_npz(cfg["file"])
    flat, offs = z["share_bytes"], z["share_offsets"]
    return {x: [unpack_share_bytes(flat, offs, e * cfg["n"] + x - 1) for e in range(cfg["N"])] for x in (1, 3)}


def test_frame_fields_host_round_trips_the_reference_share_bytes(f1_records):
    for x, recs in f1_records.items():
        buf = host_frame(x, recs)
        assert buf.size == R(len(recs)) + sum(map(len, recs))
        for form in (buf, buf.tobytes(), torch.from_numpy(buf)):
            got = codec.frame_fields_host(form, n=len(recs), x=x)
            assert (got.n, got.x, got.records_bytes) == (len(recs), x, sum(map(len, recs)))
            assert got.lens.tolist() == [len(r) for r in recs]
            assert got.records.tobytes() == b"".join(recs)
            offs = np.concatenate([[0], np.cumsum(got.lens, dtype=np.int64)])
            assert codec.records_to_list(got.records, offs) == recs
    empty = codec.frame_fields_host(host_frame(7, []))
    assert (empty.n, empty.x, empty.records_bytes, empty.lens.size, empty.records.size) == (0, 7, 0, 0, 0)


def test_frame_fields_host_rejects_each_single_field_corruption(f1_records):
    recs = f1_records[3][:37]
    good = host_frame(3, recs)
    codec.frame_fields_host(good, n=37, x=3)

    def corrupt(pos, delta=1):
        b = good.copy()
        b[pos] = (int(b[pos]) + delta) & 0xFF
        return b

    with pytest.raises(ValueError, match="wrong magic"):
        codec.frame_fields_host(corrupt(0))
    with pytest.raises(ValueError, match="wrong magic"):
        codec.frame_fields_host(corrupt(7))
    with pytest.raises(ValueError, match="the header carries n = 38, expected 37"):
        codec.frame_fields_host(corrupt(8), n=37)
    # (n 37 -> 38 inside one 16-length word is consistent in itself: only the expected n catches it)
    with pytest.raises(ValueError, match="the header carries records_bytes"):
        codec.frame_fields_host(corrupt(8, -6))  # n = 31 moves R(n)
    with pytest.raises(ValueError, match="fewer than the"):
        codec.frame_fields_host(corrupt(11))  # n + 2^24
    with pytest.raises(ValueError, match="the header carries x = 2, expected 3"):
        codec.frame_fields_host(corrupt(16, -1), x=3)
    with pytest.raises(ValueError, match="the header carries records_bytes"):
        codec.frame_fields_host(corrupt(24))
    for delta in (1, -1):
        with pytest.raises(ValueError, match="the lengths sum to"):
            codec.frame_fields_host(corrupt(32 + 5, delta))
    with pytest.raises(ValueError, match="the header carries records_bytes"):
        codec.frame_fields_host(good[:-1])
    with pytest.raises(ValueError, match="fewer than the 32-byte header"):
        codec.frame_fields_host(good[:31])


# ---------------------------------------------------------------- the plan header
def test_frame_plan_against_a_memory_model(tmp_path):
    """The finish launch and the three open launches replayed thread by thread
    from csrc/frame_plan.hpp for every edge n and 1000 seeded random (n, lens):
    every length byte and every offset written exactly once, every offset the
    naive clamped prefix, nothing outside [0, R(n)) of the frame and [0, n] of
    the offsets touched — by a stand-alone program under ASan + UBSan (not
    loaded into this process)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path / "frame_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "delta-node_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "frame_plan_check.cpp"), "-o", exe]
    # the sanitizer runtimes linked statically where the compiler can (the
    # program then runs whatever else the environment loads into processes)
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok"

