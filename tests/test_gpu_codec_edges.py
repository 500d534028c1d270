"""The share wire codec (csrc/codec_m521.hip) where test_gpu_codec.py's shapes
do not reach: the block-total scan with more than a few totals and with a
second staging pass, wave windows smaller than one aligned chunk, header
edges on decode in the LDS and in the byte-serial path, the window limit that
switches between the two, and the alignment contract of the C entry points.

Expected bytes: tests/wire_edges.py's numpy record builder (pinned record by
record to oracle/py_shamir.share_to_bytes in test_wire_edges_host.py), Python
integers and hand-built records; bit-exact.
"""
import ctypes

import numpy as np
import pytest
import torch

import wire_edges as we
from delta_node.crypto.shamir import _native, codec, field
from oracle.py_shamir import share_to_bytes

pytestmark = pytest.mark.gpu

CANARY = 0xC3
I64_CANARY = -0x0123456789ABCDEF


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def up(a: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def device_vec(limbs: np.ndarray):
    """The tiled device vector of dense limbs, filled tile-wise (lanes past n zero)."""
    vec = torch.zeros(we.vec_bytes(limbs.shape[0]), dtype=torch.uint8, device=dev())

    def put(off, b):
        vec[off:off + b.size] = torch.from_numpy(b).to(dev())

    we.fill_tiles(put, limbs)
    return vec


def decode_zeroed(packed, offs, n, **kw):
    """decode_share_vec into zeroed buffers, so the whole tiled vector compares."""
    out = torch.zeros(we.vec_bytes(n), dtype=torch.uint8, device=dev())
    return codec.decode_share_vec(packed, offs, n, out=out, **kw)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------- 1. scan shapes
@pytest.mark.parametrize("nb", [8, 9, 64, 65, 512, 513])
def test_scan_of_many_block_totals(nb):
    """nb block totals: thread t of scan_blocks_kernel scans totals 8t .. 8t + 7,
    so 9 totals need a second thread, 65 a ninth, 513 a second wave (the
    cross-wave step); each with a one-element last block and a full one."""
    for n in (we.SCAN_BLOCK * (nb - 1) + 1, we.SCAN_BLOCK * nb):
        assert -(-n // we.SCAN_BLOCK) == nb
        limbs = we.ragged_limbs(n, nb)
        want_p, want_o = we.build_records(3, limbs)
        vec = device_vec(limbs)
        packed, offs = codec.encode_share_vec(vec, n, 3)
        assert torch.equal(offs, up(want_o)), n
        assert int(offs[n].item()) == want_p.size and torch.equal(packed, up(want_p)), n
        back, xs = decode_zeroed(packed, offs, n)
        assert torch.equal(back, vec) and bool((xs == 3).all()), n


# ---------------------------------------------------------------- 2. second scan pass
@pytest.mark.slow
def test_scan_second_staging_pass():
    """n = 8192 * 1024 + 1025: 8194 block totals, so scan_blocks_kernel stages
    twice and the second pass starts from the first one's carry.  A sparse
    vector keeps the expected bytes small: zero but for every 1021st element
    and 66- / 64-byte values on both sides of the block edges that matter."""
    n = we.SCAN2_N
    nb = -(-n // we.SCAN_BLOCK)
    assert nb > we.SCAN_STAGE and nb - we.SCAN_STAGE == 2
    index, nbytes, limbs = we.sparse_values(n)
    want_p, want_o = we.build_records(3, limbs, n=n, index=index)
    assert want_o[n] == 2 * n + int(nbytes.sum())
    vec = torch.zeros(we.vec_bytes(n), dtype=torch.uint8, device=dev())
    pos, val = we.scatter_tiles(index, limbs)
    vec[up(pos)] = up(val)
    packed, offs = codec.encode_share_vec(vec, n, 3)
    assert int(offs[n].item()) == int(want_o[n])
    assert torch.equal(offs, up(want_o))
    assert torch.equal(packed, up(want_p))
    back, xs = decode_zeroed(packed, offs, n)
    assert torch.equal(back, vec) and bool((xs == 3).all())


# ---------------------------------------------------------------- 3. tiny windows
def encode_raw(vec, n, x, shift):
    """dn_m521_encode_shares into canary-filled buffers, `out` `shift` bytes
    into its allocation: (out view, offsets int64[n + 2], whole out buffer)."""
    L = codec._lib()
    cap = int(L.dn_m521_encoded_capacity(n, x))
    big = torch.full((shift + cap + 64,), CANARY, dtype=torch.uint8, device=dev())
    out = big[shift:]
    assert out.data_ptr() % 16 == shift
    offs = torch.full((n + 2,), I64_CANARY, dtype=torch.int64, device=dev())
    sb = int(L.dn_m521_codec_scratch_bytes(n))
    scratch = torch.empty(sb, dtype=torch.uint8, device=dev())
    rc = L.dn_m521_encode_shares(vec.data_ptr(), n, x, offs.data_ptr(), out.data_ptr(), cap, scratch.data_ptr(), sb,
                                 stream())
    torch.cuda.synchronize()
    return rc, out, offs, big


def check_encode(vals, x, shift):
    n = len(vals)
    limbs = we.ints_to_limbs(vals)
    want = b"".join(share_to_bytes(x, v) for v in vals)
    want_o = np.cumsum([0] + [len(share_to_bytes(x, v)) for v in vals])
    rc, out, offs, big = encode_raw(device_vec(limbs), n, x, shift)
    what = (n, x, shift)
    assert rc == 0, what
    assert offs[:n + 1].tolist() == want_o.tolist(), what
    assert int(offs[n + 1].item()) == I64_CANARY, what
    assert bytes(out[:len(want)].cpu().numpy()) == want, what
    assert bool((out[len(want):] == CANARY).all()) and bool((big[:shift] == CANARY).all()), what
    return want_o


@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("x", [0, 1, (1 << 64) - 1])
def test_tiny_windows(x, shift):
    """Waves whose records total a few bytes: all-zero vectors (x = 0, y = 0
    is the one-byte record) and values below 256, n on both sides of a wave."""
    rng = np.random.default_rng(x % 1000 + shift)
    for n in (1, 2, 3, 64, 65, 1000):
        check_encode([0] * n, x, shift)
        check_encode([int(v) for v in rng.integers(0, 256, n)], x, shift)


@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("x,last", [(0, 0), (0, 7), (0xB7, 0)])
def test_last_wave_inside_one_aligned_chunk(x, last, shift):
    """64 full-size records, the first three bytes short, then a last wave
    holding one 1- or 2-byte record: its range [A, B) lies strictly inside one
    aligned chunk (encode_kernel's `a4 > b4` branch), and the window base is
    below A, so a copy from the wrong LDS position shows."""
    al = 16 if shift == 0 else 4
    vals = [(1 << 503) + 5] + [(1 << 520) + 3 * e for e in range(1, 64)] + [last]
    want_o = check_encode(vals, x, shift)
    A, B, one_chunk = we.encode_window(want_o, 64, len(vals), al)
    assert B - A in (1, 2) and one_chunk and A % al != 0, (A, B, al)
    # wave 0 starts at its window base and spans many chunks: not that branch
    assert not we.encode_window(want_o, 0, len(vals), al)[2]


# ---------------------------------------------------------------- 4. header edges on decode
def decode_flagging(packed, offs, n):
    """(values, xs, bad count) of a decode that counts bad records instead of raising."""
    flag = torch.zeros(1, dtype=torch.int32, device=dev())
    vec, xs = decode_zeroed(packed, offs, n, bad=flag)
    return field.vec_to_ints(vec.cpu().numpy(), n), xs.cpu().tolist(), int(flag.item())


def special_records():
    """(record, expected (x, y) or None when it must be flagged)."""
    y = (1 << 519) + 77
    yb = y.to_bytes(66, "big").lstrip(b"\0")
    big_x = (1 << 64) - 1
    return [
        (bytes([8]) + big_x.to_bytes(8, "big") + yb, (big_x, y)),       # the widest x
        (bytes([9]) + bytes(range(1, 10)) + yb, None),                   # x of 9 bytes
        (bytes([5, 1, 2]), None),                                        # xlen runs past the record
        (bytes([1, 3]), (3, 0)),                                         # header only: y = 0
        (bytes([0]), (0, 0)),                                            # the one-byte record
        (b"", None),                                                     # empty
        (bytes([8]) + (1 << 63).to_bytes(8, "big"), (1 << 63, 0)),       # 8-byte x, header only
    ]


@pytest.mark.parametrize("shift", [0, 4])
def test_header_edges_in_both_decode_paths(shift):
    """Each header edge among ordinary records in a wave that stages its window
    in LDS, and again in a wave that a padded neighbour (5000 leading zero
    bytes) pushes onto the byte-serial path; the bad count is exactly the
    number of records that must be flagged and every other record is exact."""
    al = 16 if shift == 0 else 4
    rng = np.random.default_rng(17)
    ordinary = we.limbs_to_ints(we.ragged_limbs(192, 23))
    recs, want = [], []
    for w in range(3):
        wave = [(share_to_bytes(4, v), (4, v)) for v in ordinary[64 * w:64 * w + 64]]
        if w < 2:
            for i, sp in zip(rng.permutation(63)[:7], special_records()):
                wave[int(i)] = sp
        if w == 1:
            v = ordinary[70]
            wave[63] = (bytes([1, 4]) + bytes(5000) + v.to_bytes(66, "big"), (4, v))
        recs += [r for r, _ in wave]
        want += [e for _, e in wave]
    n = len(recs)
    packed, offs = we.pack_records(recs)
    assert we.decode_window(offs, 0, n, al) <= we.DEC_WINDOW_LIMIT < we.decode_window(offs, 64, n, al)
    assert we.decode_window(offs, 128, n, al) <= we.DEC_WINDOW_LIMIT
    buf = torch.zeros(shift + packed.size, dtype=torch.uint8, device=dev())
    buf[shift:] = up(packed)
    assert buf[shift:].data_ptr() % 16 == shift
    vals, xs, bad = decode_flagging(buf[shift:], up(offs), n)
    assert bad == sum(e is None for e in want) == 6
    for e, (got_v, got_x, exp) in enumerate(zip(vals, xs, want)):
        if exp is None:
            assert got_v == 0, e  # flagged records decode as 0
        else:
            assert (got_x % (1 << 64), got_v) == exp, (e, recs[e][:12])
    with pytest.raises(ValueError, match="6 records"):
        codec.decode_share_vec(buf[shift:], up(offs), n)


# ---------------------------------------------------------------- 5. window limit
@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("amod", [0, 1, 15])
def test_decode_window_limit(amod, delta, shift):
    """Four waves of one workgroup, records of the largest size (8-byte x,
    66-byte y); leading zero bytes bring the second wave's Bend - A4 to the
    limit - 1, the limit and limit + 1 (LDS path, LDS path, byte-serial path)
    with its first byte at 0, 1 and 15 (mod 16); the other waves fill the
    neighbouring LDS rows.  Every value and every x is exact on both sides."""
    al = 16 if shift == 0 else 4
    ys = we.limbs_to_ints(we.ragged_limbs(256, 100 + amod))
    ys = [y | (1 << 520) for y in ys]
    xs = [(0xF1 << 56) + 0x0102030405 * (e + 1) for e in range(256)]
    pad = [0] * 256
    pad[9] = amod                                    # wave 0 ends, and wave 1 starts, at amod (mod 16)
    pad[64 + 17] = we.DEC_WINDOW_LIMIT + delta - 64 * we.MAX_RECORD - amod % al
    assert pad[64 + 17] >= 0
    recs = [bytes([8]) + x.to_bytes(8, "big") + bytes(p) + y.to_bytes(66, "big") for x, p, y in zip(xs, pad, ys)]
    packed, offs = we.pack_records(recs)
    assert int(offs[64]) % 16 == amod
    assert we.decode_window(offs, 64, 256, al) == we.DEC_WINDOW_LIMIT + delta
    assert all(we.decode_window(offs, e0, 256, al) <= we.DEC_WINDOW_LIMIT for e0 in (0, 128, 192))
    buf = torch.zeros(shift + packed.size, dtype=torch.uint8, device=dev())
    buf[shift:] = up(packed)
    assert buf[shift:].data_ptr() % 16 == shift
    vals, got_xs, bad = decode_flagging(buf[shift:], up(offs), 256)
    assert bad == 0
    assert vals == ys
    assert [x % (1 << 64) for x in got_xs] == xs


# ---------------------------------------------------------------- 6. alignment contract
@pytest.mark.parametrize("shift", [1, 2, 3])
def test_misaligned_buffers_are_refused(shift):
    """out / in not 4-byte aligned: the body accesses of the narrow path would
    be misaligned dwords.  The C entry points return DN_ERR_ARG and launch
    nothing; encode_share_vec raises; decode_share_vec decodes an aligned copy."""
    L = codec._lib()
    n = 300
    limbs = we.ragged_limbs(n, shift)
    vec = device_vec(limbs)
    want_p, want_o = we.build_records(3, limbs)
    rc, out, offs, big = encode_raw(vec, n, 3, shift)
    assert rc == _native.DN_ERR_ARG and "4-byte aligned" in _native.last_error()
    assert bool((big == CANARY).all()) and bool((offs == I64_CANARY).all())  # nothing ran
    with pytest.raises(ValueError, match="4-byte aligned"):
        codec.encode_share_vec(vec, n, 3, out=big[shift:])
    # decode: the C entry point refuses, the wrapper copies once
    buf = torch.zeros(shift + want_p.size, dtype=torch.uint8, device=dev())
    buf[shift:] = up(want_p)
    packed, d_offs = buf[shift:], up(want_o)
    assert packed.data_ptr() % 4 == shift
    back = torch.full((we.vec_bytes(n),), CANARY, dtype=torch.uint8, device=dev())
    xs = torch.full((n,), I64_CANARY, dtype=torch.int64, device=dev())
    bad = torch.zeros(1, dtype=torch.int32, device=dev())
    rc = L.dn_m521_decode_shares(packed.data_ptr(), packed.numel(), d_offs.data_ptr(), n, back.data_ptr(),
                                 xs.data_ptr(), bad.data_ptr(), stream())
    torch.cuda.synchronize()
    assert rc == _native.DN_ERR_ARG and "4-byte aligned" in _native.last_error()
    assert bool((back == CANARY).all()) and bool((xs == I64_CANARY).all()) and int(bad.item()) == 0
    got, got_x = decode_zeroed(packed, d_offs, n)
    ref, ref_x = decode_zeroed(packed.clone(), d_offs, n)
    assert torch.equal(got, ref) and torch.equal(got, vec) and torch.equal(got_x, ref_x) and bool((got_x == 3).all())
