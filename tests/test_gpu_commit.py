"""Share commitments on the MI355X: commit_records_vec / verify_records_vec
(csrc/commit_sha256.hip) against hashlib.sha256 of every record's bytes — the
reference's calc_commitment — bit for bit.

The expected values come from tests/commit_edges.py (a Python model of the
rule in include/dn_commit.h; nothing there calls the library) or straight
from hashlib over a host copy of the wire.  Every call runs with guard bytes
around its outputs, and the wire is compared with its upload afterwards.
"""
import hashlib
import threading

import numpy as np
import pytest
import torch

import commit_edges as ce
import record_edges as re
import wire_edges as we
from delta_node.crypto import shamir
from delta_node.crypto.shamir import _native, codec, field

pytestmark = pytest.mark.gpu

CANARY = 0xC3
GUARD = 64


def dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _native.lib()


def up(a: np.ndarray, shift: int = 0):
    """A device copy of `a` whose address is `shift` bytes past a 16-byte boundary (uint8 only when shifted)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not shift:
        out = t.to(dev())
    else:
        big = torch.empty(t.numel() + 16, dtype=torch.uint8, device=dev())
        out = big[shift:shift + t.numel()]
        out.copy_(t)
    assert out.data_ptr() % 16 == shift
    return out


def guarded(nbytes: int, shift: int = 0):
    """(arena, view): nbytes at `shift` past a 16-byte boundary with GUARD canary bytes on both sides."""
    arena = torch.full((nbytes + 2 * GUARD + 16,), CANARY, dtype=torch.uint8, device=dev())
    assert arena.data_ptr() % 16 == 0
    return arena, arena[GUARD + shift:GUARD + shift + nbytes]


def guards_intact(arena, view) -> bool:
    lo = view.data_ptr() - arena.data_ptr()
    host = arena.cpu().numpy()
    return bool((host[:lo] == CANARY).all() and (host[lo + view.numel():] == CANARY).all())


def flag():
    return torch.zeros(2, dtype=torch.int32, device=dev())


def check_wire(w: re.Wire, align=None, out_shift: int = 0):
    """Commit and verify one model wire: digests, counts, ok bytes, guards, and the wire itself untouched."""
    align = align or re.align_of(w.shift)
    assert align == re.align_of(w.shift)  # the staging width is the address's: the builders place the wire for it
    wanted = ce.want_wire(w, align)
    want_d = ce.digests_of(wanted)
    hashable = np.array([ok for ok, _ in wanted], dtype=np.uint8)
    nbad = int((hashable == 0).sum())
    packed, offsets = up(w.packed, w.shift), up(w.offsets)
    n = w.n
    arena, out = guarded(32 * n, out_shift)
    bad = flag()
    got = codec.commit_records_vec(packed, offsets, n, out=out, bad=bad)
    assert got.shape == (n, 32) and got.data_ptr() == out.data_ptr()
    got_h = got.cpu().numpy()
    wrong = np.nonzero((got_h != want_d).any(axis=1))[0]
    assert wrong.size == 0, (wrong[:8].tolist(), [int(w.offsets[e + 1] - w.offsets[e]) for e in wrong[:8]])
    assert bad.tolist() == [nbad, 0]
    assert guards_intact(arena, out)
    # verify against the model's digests: exactly the unhashable records fail, none is a mismatch
    ok_arena, ok = guarded(n)
    codec.verify_records_vec(packed, offsets, n, up(want_d), ok=ok, bad=bad)
    assert np.array_equal(ok.cpu().numpy(), hashable)
    assert bad.tolist() == [2 * nbad, 0]
    assert guards_intact(ok_arena, ok)
    assert np.array_equal(packed.cpu().numpy(), w.packed)
    if nbad:
        with pytest.raises(ValueError,
                           match=f"^commit_records_vec: {nbad} records whose offsets leave their window, 0 "):
            codec.commit_records_vec(packed, offsets, n)
    return got


# ------------------------------------------------------------------ padding classes and byte phases
@pytest.mark.parametrize("shift", [0, 1, 2, 3, 4, 8, 12])
def test_every_padding_class_at_every_byte_phase_on_the_lds_path(shift):
    """Lengths 0..130 (one, two and three blocks; 55/56, 63/64/65, 119/120) in
    windows of 4160 bytes, the wire at byte shifts 0..3 (by three leading slack
    bytes that belong to no record: record starts move through the alignbyte
    phases) and 4, 8, 12 (by its address: the narrow staging path)."""
    if shift in (1, 2, 3):
        base = ce.phase_wire(0)
        w = re.Wire(bytes(shift) + base.packed.tobytes(), base.offsets + shift, 0, 0)
    else:
        w = ce.phase_wire(shift)
    assert all(win.lds for win in w.windows()), "a changed window limit moved this case off the LDS path"
    want = check_wire(w)
    if shift in (1, 2, 3):  # ... and the wire itself at that address: a view the wrapper copies once
        view = up(base.packed, shift)
        assert view.data_ptr() % 4 == shift
        got = codec.commit_records_vec(view, up(base.offsets), base.n)
        assert torch.equal(got, want)


@pytest.mark.parametrize("shift", [0, 4])
def test_sorted_lengths_take_the_byte_serial_path(shift):
    w = ce.sorted_wire(shift)
    assert ce.serial_windows(w), "no window beyond the limit: the byte-serial path is not reached"
    check_wire(w)


@pytest.mark.parametrize("shift", [0, 12])
def test_a_79_block_record_beside_short_ones(shift):
    w = ce.long_wire(shift)
    assert ce.serial_windows(w) == [0]
    check_wire(w)


# ------------------------------------------------------------------ the project's edge wires
@pytest.mark.parametrize("amod, delta, align", re.LIMIT_CASES + re.TAIL_CASES)
def test_windows_at_the_limit_and_tails(amod, delta, align):
    check_wire(re.limit_wire(amod, delta, align), align)


@pytest.mark.parametrize("align", [16, 4])
def test_the_last_staging_row(align):
    check_wire(re.row_edge_wire(align), align)


def test_window_sequences():
    for w in re.sequence_wires():
        check_wire(w)


@pytest.mark.parametrize("align", [16, 4])
def test_hostile_offsets(align):
    for name, w in re.hostile_offsets(align).items():
        assert w.in_bytes > re.HOSTILE_SLACK
        check_wire(w, align)


# ------------------------------------------------------------------ sizes: real records
def host_digests(packed, offsets, n):
    recs = codec.records_to_list(packed.cpu(), offsets.cpu()[: n + 1])
    return np.frombuffer(b"".join(hashlib.sha256(r).digest() for r in recs), dtype=np.uint8).reshape(n, 32)


@pytest.fixture(scope="module")
def big_vec():
    n = (1 << 16) + 37
    limbs = np.random.default_rng(31).integers(0, 1 << 32, (n, 17), dtype=np.uint64).astype(np.uint32)
    limbs[:, 16] = (limbs[:, 16] & 0x1FF) | 0x100  # 521-bit values: y of 66 bytes, records of 68 and 69 bytes
    return n, up(we.tiles_of(limbs))


@pytest.mark.parametrize("x", [3, 300])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, (1 << 16) + 37])
def test_real_records_at_block_and_wave_edges(big_vec, n, x):
    """encode_share_vec's own records (two blocks each); a vector of n elements
    is the first tiles of the big one."""
    _, vec = big_vec
    packed, offsets = codec.encode_share_vec(vec[: field.vec_bytes(n)].clone(), n, x)
    want = host_digests(packed, offsets, n)
    got = codec.commit_records_vec(packed, offsets, n)
    assert np.array_equal(got.cpu().numpy(), want)
    codec.verify_records_vec(packed, offsets, n, got)


# ------------------------------------------------------------------ outputs
@pytest.mark.parametrize("out_shift", [0, 4])
def test_caller_out_alignment_and_bytes_past_32n(out_shift):
    w = ce.phase_wire(0)
    packed, offsets = up(w.packed), up(w.offsets)
    n = w.n
    arena, out = guarded(32 * n + 100, out_shift)
    assert out.data_ptr() % 16 == out_shift
    bad = flag()
    got = codec.commit_records_vec(packed, offsets, n, out=out, bad=bad)
    assert np.array_equal(got.cpu().numpy(), ce.digests_of(ce.want_wire(w)))
    assert bool((out[32 * n:] == CANARY).all()) and guards_intact(arena, out)
    # the same digests as expect at that alignment
    ok = torch.zeros(n, dtype=torch.uint8, device=dev())
    codec.verify_records_vec(packed, offsets, n, out[: 32 * n], ok=ok, bad=bad)
    assert bool(ok.all()) and bad.tolist() == [0, 0]


# ------------------------------------------------------------------ verify
def test_verify_finds_flipped_commitments_and_flipped_records():
    n = 300
    w = re.ordinary_wire(3, n, 5)
    packed, offsets = up(w.packed), up(w.offsets)
    com = codec.commit_records_vec(packed, offsets, n)
    assert np.array_equal(com.cpu().numpy(), ce.digests_of(ce.want_wire(w)))
    codec.verify_records_vec(packed, offsets, n, com)                      # clean
    codec.verify_records_vec(packed, offsets, n, com.reshape(-1).clone())  # flat
    at = [0, 63, 64, n - 1]
    flipped = com.clone()
    for i, e in enumerate(at):
        flipped[e, (7 * i) % 32] ^= 1 << (i % 8)
    with pytest.raises(ValueError, match="^verify_records_vec: 0 records whose offsets leave their window, "
                                         "4 records whose SHA-256 is not their commitment$"):
        codec.verify_records_vec(packed, offsets, n, flipped)
    bad = torch.tensor([5, 7], dtype=torch.int32, device=dev())
    ok = torch.full((n,), 9, dtype=torch.uint8, device=dev())
    codec.verify_records_vec(packed, offsets, n, flipped, ok=ok, bad=bad)
    assert bad.tolist() == [5, 11]
    assert np.nonzero(ok.cpu().numpy() == 0)[0].tolist() == at and int(ok.sum()) == n - 4
    with pytest.raises(ValueError, match="^verify_records_vec: 5 records .*, 11 records"):
        codec.check_bad_commit(bad)
    # a flipped byte of a record instead
    e = 77
    tampered = packed.clone()
    tampered[int(w.offsets[e + 1]) - 1] ^= 0x40
    bad, ok = flag(), torch.zeros(n, dtype=torch.uint8, device=dev())
    codec.verify_records_vec(tampered, offsets, n, com, ok=ok, bad=bad)
    assert bad.tolist() == [0, 1] and np.nonzero(ok.cpu().numpy() == 0)[0].tolist() == [e]


def test_an_unhashable_record_fails_without_counting_as_a_mismatch():
    w = re.hostile_offsets(16)["end-above-Bend"]
    wanted = ce.want_wire(w)
    unhashable = [e for e, (ok, _) in enumerate(wanted) if not ok]
    assert unhashable
    packed, offsets = up(w.packed), up(w.offsets)
    # commitments that would match whatever bytes the offsets name: the records must fail all the same
    named = [hashlib.sha256(w.packed.tobytes()[int(a):int(b)]).digest() if b >= a else bytes(32)
             for a, b in zip(w.offsets[:-1], w.offsets[1:])]
    expect = up(np.frombuffer(b"".join(named), dtype=np.uint8).reshape(w.n, 32).copy())
    bad, ok = flag(), torch.ones(w.n, dtype=torch.uint8, device=dev())
    codec.verify_records_vec(packed, offsets, w.n, expect, ok=ok, bad=bad)
    assert np.nonzero(ok.cpu().numpy() == 0)[0].tolist() == unhashable
    assert bad.tolist() == [len(unhashable), 0]


# ------------------------------------------------------------------ the path as a user runs it
def test_encode_commit_frame_open_verify_resolve():
    ss = shamir.SecretShare(2)
    ss.random.seed(99)
    ns = [1, 257, 4095]
    rng = np.random.default_rng(8)
    secrets = [torch.from_numpy(rng.integers(-(1 << 62), 1 << 62, n, dtype=np.int64)).to(dev()) for n in ns]
    blocks = ss.make_shares_vec_many(secrets, 3)
    n_total = sum(ns)
    # the tensor list's wires, one per receiver
    wires = codec.encode_shares_many(blocks, ns)
    coms = []
    for packed, offsets in wires:
        com = codec.commit_records_vec(packed, offsets, n_total)
        assert np.array_equal(com.cpu().numpy(), host_digests(packed, offsets, n_total))
        coms.append(com)
    # one tensor as a frame: the record view on the sender's side, then out of open_frames
    n, x = ns[2], 2
    frame, offsets = codec.encode_share_frame(blocks[2][x - 1], n, x)
    R = codec.frame_records_offset(n)
    sent = codec.commit_records_vec(frame[R:], offsets, n)
    assert np.array_equal(sent.cpu().numpy(), host_digests(frame[R:], offsets, n))
    frame1, offsets1 = codec.encode_share_frame(blocks[2][0], n, 1)
    sent1 = codec.commit_records_vec(frame1[codec.frame_records_offset(n):], offsets1, n)
    opened = codec.open_frames([frame1.clone(), frame.clone()], n, [1, 2])
    for (packed, offs), com in zip(opened, (sent1, sent)):
        codec.verify_records_vec(packed, offs, n, com)
    with pytest.raises(ValueError, match=f"{n} records whose SHA-256 is not their commitment"):
        codec.verify_records_vec(*opened[0], n, sent)  # the other receiver's commitments
    got = ss.resolve_records_vec(opened, [1, 2], n)
    assert torch.equal(got, secrets[2])


# ------------------------------------------------------------------ capture
def test_captured_calls_replay_and_add_their_counts_twice():
    w = re.hostile_offsets(16)["start-below-A"]
    wanted = ce.want_wire(w)
    nbad = sum(not ok for ok, _ in wanted)
    assert nbad
    want_d = ce.digests_of(wanted)
    n = w.n
    packed, offsets = up(w.packed), up(w.offsets)
    expect = up(want_d)
    expect[5, 0] ^= 1  # one mismatch per run (record 5 is hashable)
    assert wanted[5][0]
    out = torch.zeros(32 * n, dtype=torch.uint8, device=dev())
    ok = torch.zeros(n, dtype=torch.uint8, device=dev())
    cbad, vbad = flag(), flag()

    def sequence():
        codec.commit_records_vec(packed, offsets, n, out=out, bad=cbad)
        codec.verify_records_vec(packed, offsets, n, expect, ok=ok, bad=vbad)

    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        sequence()  # the eager call, on the capture stream
    torch.cuda.synchronize()
    assert cbad.tolist() == [nbad, 0] and vbad.tolist() == [nbad, 1]
    for t in (out, ok, cbad, vbad):
        t.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        sequence()
    torch.cuda.synchronize()
    assert cbad.tolist() == [0, 0] and not bool(out.any())  # captured, not run
    for k in (1, 2):
        out.zero_()
        ok.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().reshape(n, 32), want_d), k
        assert cbad.tolist() == [k * nbad, 0] and vbad.tolist() == [k * nbad, k], k
        want_ok = np.array([int(h) for h, _ in wanted], dtype=np.uint8)
        want_ok[5] = 0
        assert np.array_equal(ok.cpu().numpy(), want_ok), k


# ------------------------------------------------------------------ threads
def test_two_threads_on_two_streams():
    """The kernel and its wrappers share no state: two threads, each on its own
    stream, each looping calls over its own wire with no host synchronisation."""
    wires = [ce.phase_wire(0), ce.sorted_wire(4)]
    R = 6
    dev_wires = [(up(w.packed, w.shift), up(w.offsets)) for w in wires]
    wants = [ce.digests_of(ce.want_wire(w)) for w in wires]
    expects = [up(d) for d in wants]
    outs = [[torch.zeros(32 * w.n, dtype=torch.uint8, device=dev()) for _ in range(R)] for w in wires]
    oks = [[torch.zeros(w.n, dtype=torch.uint8, device=dev()) for _ in range(R)] for w in wires]
    flags = [flag(), flag()]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    barrier = threading.Barrier(2)
    errors = []
    torch.cuda.synchronize()

    def work(t):
        try:
            packed, offsets = dev_wires[t]
            with torch.cuda.stream(streams[t]):
                barrier.wait()
                for r in range(R):
                    codec.commit_records_vec(packed, offsets, wires[t].n, out=outs[t][r], bad=flags[t])
                    codec.verify_records_vec(packed, offsets, wires[t].n, expects[t], ok=oks[t][r], bad=flags[t])
        except Exception as e:  # noqa: BLE001 - reported by the main thread
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    assert not errors, errors
    for t in range(2):
        assert flags[t].tolist() == [0, 0]
        for r in range(R):
            assert np.array_equal(outs[t][r].cpu().numpy().reshape(-1, 32), wants[t]), (t, r)
            assert bool(oks[t][r].all()), (t, r)
