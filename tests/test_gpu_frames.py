"""Share wire frames on the GPU (csrc/codec_frame.hip): encode_share_frame /
encode_frames_many / open_frames against encode_share_vec, torch.cumsum, the
numpy parser frame_fields_host and the reference's own share bytes
(tests/golden).  Every comparison is bit for bit.

The edge list: with B the scan's elements per workgroup (frame_plan.hpp), n
takes 0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, B - 1, B, B + 1, 3 B + 17
and the smallest n at which the scan of the block totals (n / B + 1 totals)
takes a second run of a thread (8 B), a second turn of its load loop (1024 B)
and a second pass (8192 B).  For the large ones only the lengths are built
(random u8 with 0 and 255 among them) and compared with torch.cumsum.

The slow case "all lengths 255 at n = 2^24 + B + 1" ends 15.7 MB short of 2^32
bytes (255 * 16 781 313 = 4 279 234 815), so it is kept as stated and a second
one, n = 2^24 + 17 B + 1, does cross 2^32.
"""
import os
import re

import numpy as np
import pytest
import torch

import wire_edges as we
from delta_node.crypto import aes, shamir
from delta_node.crypto.shamir import _native, codec, field
from golden.fixtures import load_npz, manifest, unpack_share_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xC3
GUARD = 64


def _plan(name: str) -> int:
    with open(os.path.join(ROOT, "delta-node_amd", "csrc", "frame_plan.hpp")) as f:
        found = re.findall(r"^constexpr \w+ " + name + r" = (\d+);", f.read(), flags=re.M)
    assert len(found) == 1, (name, found)
    return int(found[0])


B = _plan("kFrameBlock") * _plan("kFrameWord")
SCAN_THREADS, SCAN_RUN = _plan("kFrameScanThreads"), _plan("kFrameScanRun")
SMALL = [0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, B - 1, B, B + 1, 3 * B + 17]
SCAN_EDGES = [SCAN_RUN * B, SCAN_THREADS * B, SCAN_THREADS * SCAN_RUN * B]
XS = [1, 3, 255, 256, 2**64 - 1]
SS = shamir.SecretShare(3)


def dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _native.lib()
    assert B == 4096


def R(n: int) -> int:
    return 32 + 16 * ((n + 15) // 16)


def header(n: int, x: int, nbytes: int) -> np.ndarray:
    return np.frombuffer(codec.FRAME_MAGIC + np.array([n, x, nbytes], dtype="<u8").tobytes(), dtype=np.uint8)


def lens_frame(lens, x: int, total=None, fill_pad: int = 0):
    """A device frame of given lengths (uint8 device tensor) whose record area
    is left as allocated: the open kernels never read it."""
    n = lens.numel()
    total = int(lens.sum(dtype=torch.int64).item()) if total is None else total
    frame = torch.empty(R(n) + total, dtype=torch.uint8, device=dev())
    frame[:32].copy_(torch.from_numpy(header(n, x, total).copy()))
    frame[32:32 + n].copy_(lens)
    frame[32 + n:R(n)].fill_(fill_pad)
    return frame


def random_lens(n: int, seed: int):
    g = torch.Generator(device=dev())
    g.manual_seed(seed)
    lens = torch.randint(0, 256, (n,), dtype=torch.uint8, device=dev(), generator=g)
    if n >= 2:
        lens[0], lens[n - 1] = 0, 255
    if n >= 4:
        lens[n // 2], lens[n // 2 + 1] = 255, 0
    return lens


def prefix(lens, cap=None):
    out = torch.zeros(lens.numel() + 1, dtype=torch.int64, device=lens.device)
    torch.cumsum(lens, 0, dtype=torch.int64, out=out[1:])
    return out if cap is None else out.clamp(max=cap)


def is_record_view(packed, frame, n: int) -> bool:
    """`packed` is frame[R(n):]: the same storage, nothing copied (an empty view has no address of its own)."""
    return (packed.untyped_storage().data_ptr() == frame.untyped_storage().data_ptr()
            and packed.storage_offset() == frame.storage_offset() + R(n)
            and packed.numel() == frame.numel() - R(n))


def vec_of(limbs: np.ndarray):
    return torch.from_numpy(we.tiles_of(limbs)).to(dev()) if len(limbs) else torch.empty(0, dtype=torch.uint8,
                                                                                        device=dev())


# ---------------------------------------------------------------- 1. the scan at its edges
@pytest.mark.parametrize("n", SMALL + SCAN_EDGES)
def test_open_equals_cumsum_at_the_edge_sizes(n):
    lens = random_lens(n, 1000 + n % 997)
    frame = lens_frame(lens, 7, fill_pad=0xFF)  # the pad is not trusted to be zero
    big = torch.full((n + 1 + 2 * GUARD,), -0x0123456789ABCDEF, dtype=torch.int64, device=dev())
    bad = torch.zeros(2, dtype=torch.int32, device=dev())
    packed, offs = codec.open_frame(frame, n, 7, offsets=big[GUARD:GUARD + n + 1], bad=bad)
    assert offs.data_ptr() == big.data_ptr() + 8 * GUARD and offs.shape == (n + 1,)
    assert torch.equal(offs, prefix(lens))
    assert bool((big[:GUARD] == -0x0123456789ABCDEF).all()) and bool((big[GUARD + n + 1:] == -0x0123456789ABCDEF).all())
    assert bad.tolist() == [0, 0]
    assert is_record_view(packed, frame, n) and packed.numel() == int(offs[n])


@pytest.mark.slow
@pytest.mark.parametrize("extra,crosses", [(B + 1, False), (17 * B + 1, True)])
def test_offsets_around_2_32_bytes(extra, crosses):
    """All lengths 255 at n = 2^24 + B + 1 ends 15.7 MB short of 2^32 bytes
    (255 * 16 781 313 = 4 279 234 815); 2^24 + 17 B + 1 is the first size of
    that form whose last offsets lie beyond 2^32."""
    n = (1 << 24) + extra
    lens = torch.full((n,), 255, dtype=torch.uint8, device=dev())
    frame = lens_frame(lens, 3, total=255 * n)
    assert (255 * n > 1 << 32) == crosses
    packed, offs = codec.open_frame(frame, n, 3)
    assert torch.equal(offs, torch.arange(n + 1, dtype=torch.int64, device=dev()) * 255)
    assert packed.numel() == 255 * n


# ---------------------------------------------------------------- 2. parity with encode_share_vec
@pytest.fixture(scope="module")
def edge_vecs():
    """Per edge n a tiled vector of every y length 0..66 (never written) and its limbs."""
    out = {}
    for n in SMALL:
        limbs = we.ragged_limbs(n, 31 * n + 5) if n else np.zeros((0, we.LIMBS), dtype=np.uint32)
        out[n] = (vec_of(limbs), limbs)
    return out


@pytest.mark.parametrize("x", XS)
def test_frame_equals_encode_share_vec_and_the_host_view(x, edge_vecs):
    for n in SMALL:
        vec, limbs = edge_vecs[n]
        want_p, want_o = codec.encode_share_vec(vec, n, x)
        cap = codec.frame_capacity(n, x)
        big = torch.full((cap + 2 * GUARD + 16,), CANARY, dtype=torch.uint8, device=dev())
        lead = GUARD + (-(big.data_ptr() + GUARD)) % 16
        frame, offs = codec.encode_share_frame(vec, n, x, trim=False, out=big[lead:lead + cap])
        assert frame.data_ptr() == big.data_ptr() + lead and frame.numel() == cap
        assert torch.equal(offs, want_o), (x, n)
        total = want_p.numel()
        assert torch.equal(frame[R(n):R(n) + total], want_p), (x, n)
        assert bool((big[:lead] == CANARY).all()) and bool((big[lead + cap:] == CANARY).all()), (x, n)
        host = frame[:R(n) + total].cpu().numpy()
        assert host[:32].tobytes() == header(n, x, total).tobytes(), (x, n)
        assert not host[32 + n:R(n)].any(), (x, n)  # the pad is written as zero over the canary
        fields = codec.frame_fields_host(host, n=n, x=x)
        hp, ho = we.build_records(x, limbs) if n else (np.zeros(0, np.uint8), np.zeros(1, np.int64))
        assert fields.lens.tolist() == np.diff(ho).tolist(), (x, n)
        assert fields.records.tobytes() == hp.tobytes(), (x, n)
        # trimmed and allocated: the same frame cut to its length
        f2, o2 = codec.encode_share_frame(vec, n, x)
        assert f2.numel() == R(n) + total and f2.data_ptr() % 16 == 0 and torch.equal(f2, frame[:R(n) + total])
        assert torch.equal(o2, want_o)
        # and it opens to the wire it was made from
        p3, o3 = codec.open_frame(f2, None, None)
        assert torch.equal(p3, want_p) and torch.equal(o3, want_o), (x, n)


@pytest.fixture(scope="module")
def f1():
    cfg = manifest()["f1"]
    z = load_npz(cfg["file"])
    flat, offs = z["share_bytes"], z["share_offsets"]  # (an npz member is read again at every access)
    recs = {x: [unpack_share_bytes(flat, offs, e * cfg["n"] + x - 1) for e in range(cfg["N"])]
            for x in range(1, cfg["n"] + 1)}
    return cfg, torch.from_numpy(z["secrets"][:cfg["N"]]), recs


def test_record_area_is_the_reference_share_bytes(f1):
    cfg, secrets, recs = f1
    N, n = cfg["N"], cfg["n"]
    ss = shamir.SecretShare(cfg["t"])
    ss.random.seed(cfg["mt_seed"])
    block = ss.make_shares_vec(secrets, n)
    for x in range(1, n + 1):
        frame, offs = codec.encode_share_frame(block[x - 1], N, x)
        want = b"".join(recs[x])
        assert frame[R(N):].cpu().numpy().tobytes() == want, x
        fields = codec.frame_fields_host(frame.cpu(), n=N, x=x)
        assert fields.lens.tolist() == [len(r) for r in recs[x]] and fields.records.tobytes() == want


# ---------------------------------------------------------------- 3. round trips
def test_list_round_trip_gives_the_secrets(f1):
    cfg, secrets, recs = f1
    N, n, t = cfg["N"], cfg["n"], cfg["t"]
    cuts = [1, 255, 256, 257, 0, 255]
    assert sum(cuts) == N
    ss = shamir.SecretShare(t)
    ss.random.seed(cfg["mt_seed"])
    blocks = ss.make_shares_vec_many(list(torch.split(secrets, cuts)), n)
    frames = codec.encode_frames_many(blocks, cuts)
    assert len(frames) == n
    wires = codec.encode_shares_many(blocks, cuts)
    for x, ((frame, fo), (wp, wo)) in enumerate(zip(frames, wires), start=1):
        assert frame.numel() == R(N) + wp.numel() and torch.equal(frame[R(N):], wp) and torch.equal(fo, wo), x
        assert frame[R(N):].cpu().numpy().tobytes() == b"".join(recs[x]), x
        assert codec.frame_fields_host(frame.cpu(), n=N, x=x).lens.tolist() == [len(r) for r in recs[x]]
    key = bytes(range(32))
    pick = [1, 3, 5]
    received = []
    for x in pick:
        f = frames[x - 1][0]
        if x == 3:  # through the envelope, as it stands
            f = aes.decrypt_vec(key, aes.encrypt_vec(key, f, hex=True), hex=True)
            assert torch.equal(f, frames[x - 1][0])
        received.append(f)
    opened = codec.open_frames(received, N, pick)
    for (p, o), x in zip(opened, pick):
        assert torch.equal(p, wires[x - 1][0]) and torch.equal(o, wires[x - 1][1]), x
    assert torch.equal(ss.resolve_records_vec(opened, pick, N), secrets.to(dev()))
    # n and xs from the headers
    again = codec.open_frames(received, None, None)
    assert torch.equal(ss.resolve_records_vec(again, None, N), secrets.to(dev()))
    # caller buffers and abscissas that are not row + 1
    outs = [torch.empty(codec.frame_capacity(N, x), dtype=torch.uint8, device=dev()) for x in (300, 2**40 + 3)]
    got = codec.encode_frames_many(blocks, cuts, [300, 2**40 + 3], rows=[0, 4], trim=False, outs=outs)
    want = codec.encode_shares_many(blocks, cuts, [300, 2**40 + 3], rows=[0, 4])
    for (frame, fo), (wp, wo), buf in zip(got, want, outs):
        assert frame.data_ptr() == buf.data_ptr() and frame.numel() == buf.numel()
        assert torch.equal(frame[R(N):R(N) + wp.numel()], wp) and torch.equal(fo, wo)
    # a list without elements: header-only frames
    empty = codec.encode_frames_many([blocks[4]], [0], [1, 2])
    for x, (frame, fo) in zip((1, 2), empty):
        assert frame.cpu().numpy().tobytes() == header(0, x, 0).tobytes() and fo.tolist() == [0]
        p, o = codec.open_frame(frame, 0, x)
        assert p.numel() == 0 and o.tolist() == [0]


def test_three_members_sum_and_travel_on():
    n, t = 1000, 2
    rng = np.random.default_rng(5)
    secrets = [torch.from_numpy(rng.integers(-(1 << 40), 1 << 40, n, dtype=np.int64)) for _ in range(3)]
    xs = [3, 5]
    sums = {}
    for px in xs:  # party px: the members' frames in, one frame out
        frames = []
        for i, sec in enumerate(secrets):
            ss = shamir.SecretShare(t)
            ss.random.seed(100 + i)
            frames.append(codec.encode_share_frame(ss.make_shares_vec(sec, 5)[px - 1], n, px)[0])
        wires = codec.open_frames(frames, n, [px] * 3)
        total = SS.sum_records_vec(wires, px, n)
        out_frame, _ = codec.encode_share_frame(total, n, px)
        sums[px] = codec.open_frame(out_frame, n, px)
    got = shamir.SecretShare(t).resolve_records_vec([sums[px] for px in xs], xs, n)
    assert torch.equal(got.cpu(), secrets[0] + secrets[1] + secrets[2])


# ---------------------------------------------------------------- 4. batching
@pytest.fixture(scope="module")
def batch_frames():
    n, m = 257, 129
    frames, want = [], []
    for i in range(m):
        lens = random_lens(n, 5000 + i)
        frames.append(lens_frame(lens, i + 1))
        want.append(prefix(lens))
    return n, frames, want


@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 129])
def test_batched_open_equals_single_opens(m, batch_frames):
    n, frames, want = batch_frames
    bad = torch.zeros(2, dtype=torch.int32, device=dev())
    got = codec.open_frames(frames[:m], n, list(range(1, m + 1)), bad=bad)
    assert bad.tolist() == [0, 0] and len(got) == m
    for i, (p, o) in enumerate(got):
        assert torch.equal(o, want[i]), (m, i)
        assert is_record_view(p, frames[i], n)
    if m == 129:  # the single opens themselves
        for i in (0, 63, 64, 128):
            assert torch.equal(codec.open_frame(frames[i], n, i + 1)[1], want[i])


def test_misaligned_frame_is_copied_once():
    n = 300
    lens = random_lens(n, 77)
    frame = lens_frame(lens, 9)
    big = torch.empty(frame.numel() + 16, dtype=torch.uint8, device=dev())
    view = big[4:4 + frame.numel()]
    view.copy_(frame)
    assert view.data_ptr() % 16 == 4
    p, o = codec.open_frame(view, n, 9)
    assert torch.equal(o, prefix(lens)) and p.data_ptr() % 16 == 0 and torch.equal(p, frame[R(n):])


# ---------------------------------------------------------------- 5. faults, by output only
def _corrupt(frame, pos: int, value: int):
    out = frame.clone()
    out[pos] = value
    return out


@pytest.mark.parametrize("kind,want_bad", [("magic", [1, 0]), ("n", [1, 0]), ("x", [1, 0]), ("records_bytes", [1, 0]),
                                           ("len+1", [0, 1]), ("len-1", [0, 1]), ("all255short", [0, 1]),
                                           ("truncated", [1, 1])])
def test_one_corrupted_field_at_a_time(kind, want_bad):
    """The offsets are min(cumsum, frame_bytes - R(n)) whatever the bytes say,
    and `bad` holds the two counts.  (These offsets go to no other kernel here:
    test_gpu_record_edges.py's test_corrupt_frames_open_to_offsets_the_record_kernels_can_take
    hands the offsets of such frames to sum_records_vec and resolve_records_vec.)"""
    n, x = B + 300, 5
    lens = random_lens(n, 4242)
    lens[10] = 100  # so that +-1 stays a u8
    good = lens_frame(lens, x)
    total = good.numel() - R(n)
    frame, exp_lens, cap = good, lens, total
    if kind == "magic":
        frame = _corrupt(good, 3, ord("X"))
    elif kind == "n":
        frame = _corrupt(good, 8, (n + 1) & 0xFF)
    elif kind == "x":
        frame = _corrupt(good, 16, x + 1)
    elif kind == "records_bytes":
        frame = _corrupt(good, 24, (total + 1) & 0xFF)
    elif kind in ("len+1", "len-1"):
        d = 1 if kind == "len+1" else -1
        frame = _corrupt(good, 32 + 10, 100 + d)
        exp_lens = lens.clone()
        exp_lens[10] = 100 + d
    elif kind == "all255short":
        exp_lens = torch.full((n,), 255, dtype=torch.uint8, device=dev())
        cap = 1000
        frame = lens_frame(exp_lens, x, total=cap)
    elif kind == "truncated":  # the frame lost its last 100 bytes: the header's count and the sum both disagree
        cap = total - 100
        frame = good[:R(n) + cap]
    bad = torch.zeros(2, dtype=torch.int32, device=dev())
    packed, offs = codec.open_frame(frame, n, x, bad=bad)
    assert packed.numel() == cap
    assert torch.equal(offs, prefix(exp_lens, cap)), kind
    assert bool((offs[1:] >= offs[:-1]).all()) and int(offs.max()) <= cap
    assert bad.tolist() == want_bad, kind
    with pytest.raises(ValueError, match=f"^open_frames: {want_bad[0]} frames whose header .*, {want_bad[1]} frames "
                                         "whose lengths"):
        codec.open_frame(frame, n, x)
    codec.open_frame(good, n, x)  # and the good frame passes the checked form


def test_counts_are_per_frame_and_add_up():
    n = 257
    lens = random_lens(n, 1)
    good = lens_frame(lens, 1)
    wrong_x, wrong_len = good, _corrupt(good, 32 + 100, int(lens[100]) ^ 1)
    bad = torch.zeros(2, dtype=torch.int32, device=dev())
    codec.open_frames([good, wrong_x, wrong_len, good], n, [1, 2, 1, 1], bad=bad)
    assert bad.tolist() == [1, 1]
    codec.open_frames([wrong_len] * 70, n, [1] * 69 + [4], bad=bad)  # past one launch's group; the flag is added to
    assert bad.tolist() == [2, 71]
    with pytest.raises(ValueError, match="^open_frames: 2 frames whose header .*, 71 frames whose lengths"):
        codec.check_bad_frames(bad)


# ---------------------------------------------------------------- 6. no synchronisation
def test_deferred_forms_do_not_synchronise():
    """With trim=False, n and xs given and a `bad` tensor, the stream still has
    a pending event when every call has returned."""
    n, x = 3 * B + 17, 3
    vec = vec_of(we.ragged_limbs(n, 99))
    blocks = [torch.stack([vec, vec])]
    cap = codec.frame_capacity(n, x)
    out = torch.empty(cap, dtype=torch.uint8, device=dev())
    outs = [torch.empty(cap, dtype=torch.uint8, device=dev()) for _ in range(2)]
    offs = [torch.empty(n + 1, dtype=torch.int64, device=dev()) for _ in range(5)]
    bad = torch.zeros(2, dtype=torch.int32, device=dev())
    want_p, want_o = codec.encode_share_vec(vec, n, x)
    # warm up with the same shapes: scratch buffers, code objects
    warm = codec.encode_share_frame(vec, n, x)[0]
    codec.open_frames([warm, warm], n, [x, x])
    codec.encode_frames_many(blocks, [n], [1, 2])
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    torch.cuda._sleep(20_000_000)
    end.record()
    end.synchronize()
    cycles_per_ms = 20_000_000 / max(start.elapsed_time(end), 1e-3)
    torch.cuda.synchronize()
    pending = torch.cuda.Event()
    torch.cuda._sleep(int(400 * cycles_per_ms))
    pending.record()
    frame, fo = codec.encode_share_frame(vec, n, x, trim=False, out=out, offsets=offs[0])
    many = codec.encode_frames_many(blocks, [n], [1, 2], trim=False, outs=outs, offsets=offs[1:3])
    full = frame[:R(n) + want_p.numel()]  # the length known from elsewhere: no read-back
    opened = codec.open_frames([full, full], n, [x, x], offsets=offs[3:5], bad=bad)
    still_pending = not pending.query()
    torch.cuda.synchronize()
    assert still_pending, "a call synchronised (or the device finished 400 ms of work before the host queued five calls)"
    assert bad.tolist() == [0, 0]
    assert torch.equal(fo, want_o) and torch.equal(opened[0][0], want_p) and torch.equal(opened[1][1], want_o)
    assert len(many) == 2 and many[0][0].data_ptr() == outs[0].data_ptr()
