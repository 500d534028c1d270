"""The vector API where calls share state (MI355X): four threads on ONE stream,
calls queued behind a stalled stream, and captured graphs replayed over
rewritten inputs.

The library's contract is that calls never synchronise and are re-entrant
(include/dn_shamir.h), yet three pieces of state outlive a call: the codec
wrappers' cached scratch and flag (codec._scratch, codec._checked_flag), the
pinned staging pool behind the table uploads (csrc/shamir_m521.hip, stage_take /
stage_give), and whatever a captured graph bakes in.  Every other GPU test
issues one call at a time on one stream with a synchronise in between.

Every comparison is bit for bit against values Python builds: wires and frames
against `_share_to_bytes` per record, field and int64 results against Python
integers mod p = 2^521 - 1.  No call is checked against another call of the
API.

A. Threads on one stream.  T = 4 threads start at a barrier inside
`with torch.cuda.stream(S)` for ONE side stream S (and again on the default
stream, where Python threads start), each looping R calls with no host
synchronisation: trim=False, caller out= / offsets= / bad=, every call into its
own slot of a ring the main thread allocated.  After the joins one
synchronise, then EVERY slot of every thread is checked.  ctypes releases the
GIL, so the launches of the multi-launch entry points interleave on the stream
(A.scan, B.scan, A.encode); with a scratch shared by the threads one call then
reads another's lengths, table or totals.  The conditions that keep such a
mix-up a wrong wire and never a stray store:
  - all threads of a test use identical shapes: the same n, the same segment
    list, the same number of wires and of frames;
  - all threads use abscissas of one byte length (3..70 here), so capacities
    are equal and a thread that picks up another's lengths, table or totals
    still addresses live memory of the right size;
  - only the data, the abscissas and the output buffers differ;
  - every tensor any thread touches is allocated before the threads start and
    stays referenced until after the final synchronise;
  - a scan that runs twice over shared block totals scans prefixes: with the
    three blocks of test 1 that only shrinks them ([t0, t1, t2] -> [0, t0, t0 +
    t1] -> [0, 0, t0]), and open_frames clamps every offset; the tile totals of
    encode_shares_many (13 tiles) can grow past the wire's capacity, at most
    fourfold-scanned (each thread's scan follows its own totals launch), so
    that test's outputs are slots of one arena with that bound of slack behind
    them.
  These tests must not be run with unequal shapes against wrappers that share
  their scratch.

B. A stalled stream.  A spin kernel of about 200 ms holds a side stream while
one thread queues nine calls behind it; an event behind the spin must still
be pending when the last call has been queued (else the test FAILS with "stall
too short").  A staging buffer handed out while its copy is pending, an input
read on the host, or a call on another stream gives a wrong result.

C. Capture, replay, rewrite, replay.  One linear graph (one stream, no fork;
the MT draw is not captured) of the calls the header documents as capturable;
the second replay, over inputs rewritten in place, must give the NEW data's
results and add a second call's counts to the flags.
"""
import contextlib
import functools
import math
import os
import re
import threading
import time

import numpy as np
import pytest
import torch

import field_edges as fe
import wire_edges as we
from delta_node.crypto import shamir
from delta_node.crypto.shamir import _native, codec, field
from delta_node.crypto.shamir import shamir as shamir_mod
from test_share_sum_host import sum_group

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = we.P
T = 4                 # threads of every part A test
KINDS = ["side", "default"]
to_bytes = shamir_mod._share_to_bytes


def _constant(path: str, name: str) -> int:
    with open(os.path.join(ROOT, "delta-node_amd", "csrc", path)) as f:
        found = re.findall(r"^\s*constexpr \w+ " + name + r" = (\d+);", f.read(), flags=re.M)
    assert len(found) == 1, (path, name, found)
    return int(found[0])


SCAN = _constant("codec_m521.hip", "kScanElems")       # elements per block of lengths_scan_kernel
ENC_GROUP = _constant("codec_many.hip", "kGroup")      # wires per launch group of encode_shares_many
FRAME_B = _constant("frame_plan.hpp", "kFrameBlock") * _constant("frame_plan.hpp", "kFrameWord")
SUM_G = sum_group()                                    # DN_M521_SUM_GROUP


def dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _native.lib()
    assert (SCAN, ENC_GROUP, FRAME_B, SUM_G) == (1024, 16, 4096, 256)


# ------------------------------------------------------------------ values Python builds
def up(a):
    return torch.from_numpy(np.array(a)).to(dev())  # (a writable copy: frombuffer arrays are read-only)


def ragged(n: int, seed: int):
    """n Python ints below p of every byte length 0..66."""
    return we.limbs_to_ints(we.ragged_limbs(n, seed))


def dvec(vals):
    """The tiled device vector of Python ints below 2^521."""
    return up(field.ints_to_vec(vals))


def as_i64(v: int) -> int:
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def want_i64(vals):
    return torch.tensor([as_i64(v) for v in vals], dtype=torch.int64, device=dev())


def records(x: int, ys):
    return [to_bytes((x, y)) for y in ys]


def pack(recs):
    """Records back to back and their int64 offsets (numpy)."""
    offs = np.zeros(len(recs) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in recs], out=offs[1:])
    return np.frombuffer(b"".join(recs), dtype=np.uint8).copy(), offs


def frame_of(x: int, recs):
    """[magic][n][x][records_bytes][lens u8[n], zero-padded to 16][records] (numpy) and the offsets."""
    n, body = len(recs), b"".join(recs)
    head = codec.FRAME_MAGIC + np.array([n, x, len(body)], dtype="<u8").tobytes()
    lens = bytes(len(r) for r in recs) + bytes(-n % 16)
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(r) for r in recs], out=offs[1:])
    return np.frombuffer(head + lens + body, dtype=np.uint8).copy(), offs


def R_of(n: int) -> int:
    return 32 + 16 * ((n + 15) // 16)


def poly_shares(vals, coefs, x: int):
    """y_e = vals[e] + sum_j coefs[j][e] x^(j + 1) mod p."""
    return [fe.split_expected([v] + [c[e] for c in coefs], x) for e, v in enumerate(vals)]


def device_wire(x: int, ys):
    p, o = pack(records(x, ys))
    return up(p), up(o)


def same_wire(out, offs, want_packed, want_offs) -> bool:
    return torch.equal(offs, want_offs) and torch.equal(out[: want_packed.numel()], want_packed)


# ------------------------------------------------------------------ A. the thread form
def run_threads(kind: str, body) -> None:
    """body(t) from T threads that start together on ONE stream: a side stream
    they all enter, or the default stream every thread starts on."""
    side = torch.cuda.Stream() if kind == "side" else None
    with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
        stream = _native.stream_ptr()
    assert (stream == side.cuda_stream) if side is not None else (stream == torch.cuda.default_stream().cuda_stream)
    torch.cuda.synchronize()  # the inputs were written on the main thread's stream
    barrier = threading.Barrier(T)
    errs = [None] * T

    def run(t):
        try:
            with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
                assert _native.stream_ptr() == stream  # the premise: one stream for all threads
                barrier.wait(timeout=30)
                body(t)
        except BaseException as e:  # noqa: BLE001 (reported by the asserting thread)
            errs[t] = e

    threads = [threading.Thread(target=run, args=(t,)) for t in range(T)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=60)
    assert not any(th.is_alive() for th in threads), "a thread is still running"
    assert errs == [None] * T, errs
    torch.cuda.synchronize()


def run_ring(name: str, kind: str, R: int, call, right) -> None:
    """call(t, r): call r of thread t into slot r, nothing that synchronises;
    right(t, r): slot r of thread t holds what Python built.  Every slot is
    looked at; the count of wrong ones is printed before it is asserted."""

    def body(t):
        for r in range(R):
            call(t, r)

    run_threads(kind, body)
    wrong = [(t, r) for t in range(T) for r in range(R) if not right(t, r)]
    print(f"{name}[{kind}]: {len(wrong)} of T*R = {T}*{R} = {T * R} slots wrong")
    assert not wrong, f"(thread, call) slots that differ from the Python-built result: {wrong}"


# ---- A1. encode_share_vec
N1 = 2 * 1024 + 301   # two whole scan blocks of kScanElems = 1024 and a ragged third
R1 = 256


@functools.lru_cache(maxsize=None)
def encode_case():
    """Per thread: (x, vector, the wire Python builds, its offsets)."""
    assert N1 == 2 * SCAN + 301
    out = []
    for t in range(T):
        x, vals = 3 + t, ragged(N1, 100 + t)
        out.append((x, dvec(vals)) + device_wire(x, vals))
    assert len({tuple(c[3][:64].tolist()) for c in out}) == T  # the threads' offsets differ
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_threads_encode_share_vec(kind):
    """Three launches per call that hand `local` and the block totals on
    through the scratch: lengths_scan_kernel (3 blocks), scan_blocks_kernel,
    encode_kernel."""
    case = encode_case()
    cap = codec.encoded_capacity(N1, 3)
    assert all(codec.encoded_capacity(N1, c[0]) == cap for c in case)
    outs = torch.zeros((T, R1, cap), dtype=torch.uint8, device=dev())
    offs = torch.zeros((T, R1, N1 + 1), dtype=torch.int64, device=dev())

    def call(t, r):
        x, vec = case[t][:2]
        codec.encode_share_vec(vec, N1, x, trim=False, out=outs[t, r], offsets=offs[t, r])

    run_ring("encode_share_vec", kind, R1, call,
             lambda t, r: same_wire(outs[t, r], offs[t, r], case[t][2], case[t][3]))


# ---- A2. encode_shares_many / encode_frames_many
NS2 = [1, 255, 256, 257, 3, 511, 512, 513]   # sizes around the tile edges: 13 tiles
M2 = 17                                      # wires: two launch groups (kGroup = 16) over one uploaded table
ROWS2 = [i % 3 for i in range(M2)]           # three share rows per block, each under several abscissas
R2 = 32


@functools.lru_cache(maxsize=None)
def many_case():
    """Per thread: (xs, blocks, [per wire: records])."""
    assert M2 == ENC_GROUP + 1
    out = []
    for t in range(T):
        xs = [3 + M2 * t + i for i in range(M2)]  # 3..70: one byte each
        vals = [[ragged(n, 1000 * t + 10 * k + s) for s in range(3)] for k, n in enumerate(NS2)]
        blocks = [torch.stack([dvec(v) for v in rows]) for rows in vals]
        recs = [[r for rows in vals for r in records(x, rows[row])] for x, row in zip(xs, ROWS2)]
        out.append((xs, blocks, recs))
    return out


@functools.lru_cache(maxsize=None)
def many_want(framed: bool):
    """Per thread and wire: (bytes, offsets) on the device."""
    return [[tuple(up(a) for a in (frame_of(x, r) if framed else pack(r))) for x, r in zip(xs, recs)]
            for xs, _, recs in many_case()]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("framed", [False, True], ids=["wires", "frames"])
def test_threads_encode_many(framed, kind):
    """One table upload into the scratch and two launch groups of three
    launches over it per call (and one finish launch for frames): 17 wires of
    8 tensors, every wire (frame: header and length bytes included) against
    Python's."""
    case, want = many_case(), many_want(framed)
    n_total, tiles = sum(NS2), sum((n + 255) // 256 for n in NS2)
    head = R_of(n_total) if framed else 0
    slot = (head + codec.encoded_capacity(n_total, 3) + 15) & ~15
    # A scan that runs again over shared tile totals scans prefixes, and entry
    # k of a fourfold scan is sum_j C(k - j + 2, 3) t_j <= C(tiles + 2, 4) * (a
    # tile's most bytes), where the tile's own records start: stores that far
    # past a wire's start stay in the arena.
    slack = (math.comb(tiles + 2, 4) + 1) * 256 * we.MAX_RECORD
    arena = torch.zeros(T * R2 * M2 * slot + slack, dtype=torch.uint8, device=dev())
    outs = [[list(arena[(t * R2 + r) * M2 * slot:(t * R2 + r + 1) * M2 * slot].split(slot)) for r in range(R2)]
            for t in range(T)]
    offs = torch.zeros((T, R2, M2, n_total + 1), dtype=torch.int64, device=dev())
    encode = codec.encode_frames_many if framed else codec.encode_shares_many

    def call(t, r):
        xs, blocks, _ = case[t]
        encode(blocks, NS2, xs, rows=ROWS2, trim=False, outs=outs[t][r], offsets=list(offs[t, r]))

    def right(t, r):
        return all(same_wire(outs[t][r][i], offs[t, r, i], *want[t][i]) for i in range(M2))

    run_ring("encode_frames_many" if framed else "encode_shares_many", kind, R2, call, right)


# ---- A3. open_frames
N3 = 2 * 4096 + 77    # two whole blocks of the frame scan (B = 4096 lengths) and a ragged third
F3 = 2                # frames per call
R3 = 256


@functools.lru_cache(maxsize=None)
def frames_case():
    """Per thread: (xs, frames, Python's prefix sums)."""
    assert N3 == 2 * FRAME_B + 77
    out = []
    for t in range(T):
        xs = [3 + F3 * t + i for i in range(F3)]
        built = [frame_of(x, records(x, ragged(N3, 300 + F3 * t + i))) for i, x in enumerate(xs)]
        out.append((xs, [up(f) for f, _ in built], [up(o) for _, o in built]))
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_threads_open_frames(kind):
    """Block totals, their scan and the expansion pass through the scratch;
    each thread has its own frames, lengths and flag."""
    case = frames_case()
    offs = torch.zeros((T, R3, F3, N3 + 1), dtype=torch.int64, device=dev())
    flags = torch.zeros((T, 2), dtype=torch.int32, device=dev())
    packed = {}

    def call(t, r):
        xs, frames, _ = case[t]
        packed[t, r] = codec.open_frames(frames, N3, xs, offsets=list(offs[t, r]), bad=flags[t])

    def right(t, r):
        _, frames, want = case[t]
        return all(torch.equal(offs[t, r, i], want[i]) and o.data_ptr() == offs[t, r, i].data_ptr()
                   and p.data_ptr() == frames[i].data_ptr() + R_of(N3) for i, (p, o) in enumerate(packed[t, r]))

    try:
        run_ring("open_frames", kind, R3, call, right)
    finally:
        print(f"open_frames[{kind}]: flags {flags.tolist()}")
    assert flags.tolist() == [[0, 0]] * T


# ---- A4. decode_share_vec, checked form
N4 = 300
R4 = 256
BAD4 = (5, 77, 299)   # the three unrepresentable records of the bad wires


@pytest.mark.parametrize("kind", KINDS)
def test_threads_checked_decode(kind):
    """bad=None zeroes a cached counter, launches and reads it back (a
    synchronise per call by construction).  Threads 0 and 1 decode clean wires
    and must never raise; threads 2 and 3 decode a wire with exactly three
    unrepresentable records and must raise, naming 3, on every iteration."""
    vals = [ragged(N4, 400 + t) for t in range(T)]
    wires, want = [], []
    for t in range(T):
        recs = records(3 + t, vals[t])
        if t >= 2:
            for e in BAD4:
                recs[e] = bytes([9]) + bytes(12)  # an x of 9 bytes
        wires.append(tuple(up(a) for a in pack(recs)))
        want.append(dvec([0 if t >= 2 and e in BAD4 else v for e, v in enumerate(vals[t])]))
    outs = torch.zeros((T, R4, field.vec_bytes(N4)), dtype=torch.uint8, device=dev())
    xs = torch.zeros((T, R4, N4), dtype=torch.int64, device=dev())
    seen = {}

    def body(t):
        for r in range(R4):
            try:
                codec.decode_share_vec(*wires[t], N4, out=outs[t, r], xs=xs[t, r])
                seen[t, r] = None
            except ValueError as e:
                seen[t, r] = str(e)

    run_threads(kind, body)
    message = "decode_share_vec: 3 records with x > 8 bytes or y > 68 bytes"
    wrong = [(t, r, seen[t, r]) for t in range(T) for r in range(R4)
             if seen[t, r] != (message if t >= 2 else None) or not torch.equal(outs[t, r], want[t])]
    print(f"decode_share_vec(bad=None)[{kind}]: {len(wrong)} of T*R = {T}*{R4} = {T * R4} outcomes wrong")
    assert not wrong, wrong
    good = [e for e in range(N4) if e not in BAD4]
    for t in range(T):  # (the x of an unrepresentable record is left unparsed)
        assert bool((xs[t][:, good if t >= 2 else slice(None)] == 3 + t).all())


# ---- A5. controls: the state of these calls is per call
N5 = 300
NS5 = [1, 255, 257]
R5 = 64
M5 = 2 * 256 + 1      # sum_shares_vec: chained launches of DN_M521_SUM_GROUP = 256 inputs accumulating in `out`


def control_resolve_many(t):
    ss, xs = shamir.SecretShare(2), [3 + t, 8 + t]
    vals = [ragged(n, 500 + 10 * t + j) for j, n in enumerate(NS5)]
    blocks = [torch.stack([dvec(poly_shares(v, [ragged(len(v), 900 + 10 * t + j)], x)) for x in xs])
              for j, v in enumerate(vals)]
    outs = [[torch.zeros(n, dtype=torch.int64, device=dev()) for n in NS5] for _ in range(R5)]
    want, over, got = [want_i64(v) for v in vals], [sum(y >> 64 != 0 for y in v) for v in vals], {}

    def call(r):
        got[r] = ss.resolve_shares_vec_many(blocks, xs, NS5, outs=outs[r], return_overflow=True)[1]

    return call, lambda r: all(torch.equal(o, w) for o, w in zip(outs[r], want)) and got[r].tolist() == over


def control_sum_vecs(t):
    ss = shamir.SecretShare(2)
    edges = fe.edge_values()
    pool = [ragged(N5, 600 + 10 * t + i) for i in range(6)] + [(edges * 2)[t:t + N5]]  # p itself among them
    vecs = [dvec(v) for v in pool]
    signs = [-1 if (5 * i + t) % 3 == 0 else 1 for i in range(M5)]
    assert M5 == 2 * SUM_G + 1 and len(pool[6]) == N5
    want = dvec([sum(s * pool[i % 7][e] for i, s in enumerate(signs)) % P for e in range(N5)])
    outs = torch.zeros((R5, field.vec_bytes(N5)), dtype=torch.uint8, device=dev())

    def call(r):
        ss.sum_shares_vec([vecs[i % 7] for i in range(M5)], signs=signs, out=outs[r])

    return call, lambda r: torch.equal(outs[r], want)


def control_resolve_records(t):
    ss, xs = shamir.SecretShare(2), [3 + t, 8 + t]
    vals, coef = ragged(N5, 700 + t), ragged(N5, 750 + t)
    wires = [device_wire(x, poly_shares(vals, [coef], x)) for x in xs]
    flag, want, got = torch.zeros(2, dtype=torch.int32, device=dev()), want_i64(vals), {}

    def call(r):
        got[r] = ss.resolve_records_vec(wires, xs, N5, bad=flag)

    return call, lambda r: torch.equal(got[r], want) and flag.tolist() == [0, 0]


def control_sum_records(t):
    ss, x = shamir.SecretShare(2), 3 + t
    vals = [ragged(N5, 800 + 10 * t + i) for i in range(3)]
    wires = [device_wire(x, v) for v in vals]
    flag = torch.zeros(2, dtype=torch.int32, device=dev())
    want = dvec([(a - b + c) % P for a, b, c in zip(*vals)])
    outs = torch.zeros((R5, field.vec_bytes(N5)), dtype=torch.uint8, device=dev())

    def call(r):
        ss.sum_records_vec(wires, x, N5, signs=[1, -1, 1], out=outs[r], bad=flag)

    return call, lambda r: torch.equal(outs[r], want) and flag.tolist() == [0, 0]


CONTROLS = {"resolve_shares_vec_many": control_resolve_many, "sum_shares_vec": control_sum_vecs,
            "resolve_records_vec": control_resolve_records, "sum_records_vec": control_sum_records}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(CONTROLS))
def test_threads_calls_with_state_per_call(name, kind):
    """The same thread form over calls whose scratch is allocated per call or
    that have none: they pin the contract and prove the harness."""
    per_thread = [CONTROLS[name](t) for t in range(T)]
    run_ring(name, kind, R5, lambda t, r: per_thread[t][0](r), lambda t, r: per_thread[t][1](r))


# ------------------------------------------------------------------ B. a stalled stream
STALL_MS = 200.0
STALL_CAP_MS = 1000.0


class Stall:
    """A spin of about STALL_MS on `stream`, its cycle count calibrated by a
    short timed spin, and an event right behind it."""

    def __init__(self, stream):
        self.stream = stream
        with torch.cuda.stream(stream):
            torch.cuda._sleep(1000)  # (the spin kernel's first launch is not timed)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(2_000_000)
            b.record()
        b.synchronize()
        per_cycle = a.elapsed_time(b) / 2_000_000
        assert per_cycle > 0
        self.cycles = int(min(STALL_MS, STALL_CAP_MS) / per_cycle)
        self.start, self.end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def __enter__(self):
        torch.cuda.synchronize()
        self.stream_ctx = torch.cuda.stream(self.stream)
        self.stream_ctx.__enter__()
        self.start.record()
        torch.cuda._sleep(self.cycles)
        self.end.record()
        self.t0 = time.perf_counter()
        return self

    def __exit__(self, *exc):
        pending = not self.end.query()  # read first: everything is queued, nothing has synchronised
        queued_ms = 1e3 * (time.perf_counter() - self.t0)
        self.stream_ctx.__exit__(*exc)
        torch.cuda.synchronize()
        self.ms = self.start.elapsed_time(self.end)
        print(f"stall: {self.ms:.1f} ms on the device; the host queued its calls in {queued_ms:.1f} ms")
        if exc[0] is None:
            assert pending, (f"stall too short: the {self.ms:.1f} ms spin had ended when the last call was queued "
                             f"({queued_ms:.1f} ms after it): nothing was held back")
            assert self.ms <= 1.5 * STALL_CAP_MS, f"the stall ran {self.ms:.1f} ms"
        return False


def share_list(ns, xs, seed: int):
    """A tensor list's values, its share blocks [k, vec_bytes(n)] in xs order (a
    polynomial of degree k - 1) and the shares as Python ints."""
    vals = [ragged(n, seed + j) for j, n in enumerate(ns)]
    ys = [[poly_shares(v, [ragged(len(v), seed + 50 + 7 * j + d) for d in range(len(xs) - 1)], x) for x in xs]
          for j, v in enumerate(vals)]
    return vals, [torch.stack([dvec(y) for y in rows]) for rows in ys], ys


def test_calls_queued_behind_a_stalled_stream():
    """Five resolve_shares_vec_many calls (three lists and abscissa sets; each
    uploads its table through a pinned staging buffer), three
    encode_shares_many calls (a table upload each, into the stream's scratch)
    and a sum_shares_vec over two of the resolved field results, queued by one
    thread with no synchronisation while the stream is held.  With the guard of
    stage_take wrong, call k's table is overwritten by call k + 1's before its
    copy has run."""
    lists = [([300, 1, 257], [1, 3], 2), ([300, 1, 257], [2, 5, 7], 3), ([64, 513], [258, 259], 2)]
    data = [share_list(ns, xs, 2000 + 100 * i) for i, (ns, xs, _) in enumerate(lists)]
    int_outs = [[torch.zeros(n, dtype=torch.int64, device=dev()) for n in ns] for ns, _, _ in lists]
    flat = [torch.zeros(sum(field.vec_bytes(n) for n in lists[i][0]), dtype=torch.uint8, device=dev())
            for i in range(2)]
    total = torch.zeros_like(flat[0])
    wires = []  # per list: (outs, offsets) of its abscissas
    for ns, xs, _ in lists:
        wires.append(([torch.zeros(codec.encoded_capacity(sum(ns), x), dtype=torch.uint8, device=dev()) for x in xs],
                      [torch.zeros(sum(ns) + 1, dtype=torch.int64, device=dev()) for _ in xs]))
    overs = []
    with Stall(torch.cuda.Stream()) as stall:
        for (ns, xs, t), (_, blocks, _), outs in zip(lists, data, int_outs):
            overs.append(shamir.SecretShare(t).resolve_shares_vec_many(blocks, xs, ns, out="int64", outs=outs,
                                                                       return_overflow=True)[1])
        for (ns, xs, _), (_, blocks, _), (outs, offs) in zip(lists, data, wires):
            codec.encode_shares_many(blocks, ns, xs, rows=list(range(len(xs))), trim=False, outs=outs, offsets=offs)
        for (ns, xs, t), (_, blocks, _), buf in zip(lists[:2], data[:2], flat):
            shamir.SecretShare(t).resolve_shares_vec_many(blocks, xs, ns, out="field",
                                                          outs=list(buf.split([field.vec_bytes(n) for n in ns])))
        shamir.SecretShare(2).sum_shares_vec(flat, out=total)
    assert 0.5 * STALL_MS <= stall.ms
    for (ns, xs, _), (vals, _, ys), outs, over, (packed, offs) in zip(lists, data, int_outs, overs, wires):
        for v, o in zip(vals, outs):
            assert torch.equal(o, want_i64(v))
        assert over.tolist() == [sum(y >> 64 != 0 for y in v) for v in vals]
        for i, x in enumerate(xs):
            assert same_wire(packed[i], offs[i], *(up(a) for a in pack([r for rows in ys for r in records(x, rows[i])])))
    off = 0
    for j, n in enumerate(lists[0][0]):  # the chained consumer: list 0 + list 1, element-wise mod p
        want = dvec([(a + b) % P for a, b in zip(data[0][0][j], data[1][0][j])])
        assert torch.equal(total[off:off + want.numel()], want)
        off += want.numel()


def test_split_to_reconstruct_chain_behind_a_stalled_stream():
    """make_shares_vec_prng -> encode_share_frame(trim=False) -> open_frames(bad=flag)
    -> resolve_records_vec(bad=flag) as one un-synchronised chain: the result is
    the secrets, both flags zero, read once at the end.  open_frames takes
    frames cut to their length, which trim=False leaves on the device, so the
    lengths come from an eager run of the same keyed (hence deterministic)
    split; a wrong one would be counted in the frame flag."""
    n, shares, xs, key = 300, 3, [1, 3], bytes(range(32))
    ss = shamir.SecretShare(2)
    secrets = np.random.default_rng(7).integers(-(1 << 63), (1 << 63) - 1, size=n, endpoint=True, dtype=np.int64)
    edge = [0, 1, -1, -(1 << 63), (1 << 63) - 1]
    secrets[:len(edge)] = edge
    values = up(secrets)
    block = torch.zeros((shares, field.vec_bytes(n)), dtype=torch.uint8, device=dev())
    ss.make_shares_vec_prng(values, shares, key=key, out=block)
    lengths = [R_of(n) + int(codec.encode_share_vec(block[x - 1], n, x, trim=False)[1][n].item()) for x in xs]
    block.zero_()
    frames = [torch.zeros(codec.frame_capacity(n, x), dtype=torch.uint8, device=dev()) for x in xs]
    enc_offs = [torch.zeros(n + 1, dtype=torch.int64, device=dev()) for _ in xs]
    open_offs = [torch.zeros(n + 1, dtype=torch.int64, device=dev()) for _ in xs]
    frame_flag = torch.zeros(2, dtype=torch.int32, device=dev())
    record_flag = torch.zeros(2, dtype=torch.int32, device=dev())
    with Stall(torch.cuda.Stream()):
        ss.make_shares_vec_prng(values, shares, key=key, out=block)
        for x, f, o in zip(xs, frames, enc_offs):
            codec.encode_share_frame(block[x - 1], n, x, trim=False, out=f, offsets=o)
        opened = codec.open_frames([f[:length] for f, length in zip(frames, lengths)], n, xs, offsets=open_offs,
                                   bad=frame_flag)
        got = ss.resolve_records_vec(opened, xs, n, bad=record_flag)
    assert torch.equal(got.cpu(), torch.from_numpy(secrets))
    assert frame_flag.tolist() == [0, 0] and record_flag.tolist() == [0, 0]
    for eo, oo in zip(enc_offs, open_offs):
        assert torch.equal(eo, oo)


# ------------------------------------------------------------------ C. capture, replay, rewrite, replay
def test_captured_calls_replay_over_rewritten_inputs():
    """One linear graph of sum_shares_vec (m = 5, and m = 2 G + 1 with mixed
    signs), resolve_records_vec(bad=flag), sum_records_vec(out=, bad=flag),
    encode_share_frame(trim=False, out=, offsets=) and open_frames(offsets=,
    bad=flag).  The eager warm-up on the capture stream (so that the cached
    scratch exists outside the graph's pool) is itself checked against Python;
    the replay must reproduce it into zeroed outputs; after every input has
    been overwritten in place — share vectors with a fresh draw, wires and
    frames with the same records in reversed element order, so that the packed
    length stays and every offset moves — the second replay must give the new
    data's results, and the flags a second call's counts on top of the first's.
    (resolve_records_vec has no out= argument: its result is allocated by the
    captured call, lives in the graph's pool and is rewritten by every replay.)"""
    n, x, xs2 = 300, 5, [3, 8]
    ss = shamir.SecretShare(2)
    vb = field.vec_bytes(n)
    signs = [-1 if i % 3 == 1 else 1 for i in range(M5)]
    bad_at = (5, 77)  # sum_records_vec: two unrepresentable records in wire 1, counted once per call

    def build(gen: int, flip: bool):
        """The inputs of generation `gen` as host arrays and the expected outputs."""
        order = (lambda seq: seq[::-1]) if flip else (lambda seq: seq)
        d = {}
        pool = [ragged(n, 3000 + 100 * gen + i) for i in range(6)] + [(fe.edge_values() * 2)[gen:gen + n]]
        d["pool"] = [field.ints_to_vec(v) for v in pool]
        d["sum5"] = field.ints_to_vec([sum(pool[i][e] for i in range(5)) % P for e in range(n)])
        d["sumG"] = field.ints_to_vec([sum(s * pool[i % 7][e] for i, s in enumerate(signs)) % P for e in range(n)])
        # the wires hold generation 0's records in both generations, reversed in the second
        vals, coef = order(ragged(n, 3500)), order(ragged(n, 3501))
        d["rec_wires"] = [pack(records(xx, poly_shares(vals, [coef], xx))) for xx in xs2]
        d["rec_want"] = np.array([as_i64(v) for v in vals], dtype=np.int64)
        members = [order(ragged(n, 3600 + i)) for i in range(3)]
        recs = [records(x, m) for m in members]
        for e in bad_at:
            recs[1][n - 1 - e if flip else e] = bytes([9]) + bytes(12)
        d["sum_wires"] = [pack(r) for r in recs]
        lost = {n - 1 - e if flip else e for e in bad_at}
        d["sum_want"] = field.ints_to_vec([(a - (0 if e in lost else b) + c) % P
                                          for e, (a, b, c) in enumerate(zip(*members))])
        enc = order(ragged(n, 3700))
        d["enc_vec"] = field.ints_to_vec(enc)
        d["enc_want"] = frame_of(x, records(x, enc))
        d["frames"] = [frame_of(xx, records(xx, order(ragged(n, 3800 + i)))) for i, xx in enumerate(xs2)]
        return d

    first, second = build(0, False), build(1, True)
    for key in ("rec_wires", "sum_wires", "frames"):  # the same byte counts: rewritten in place
        assert [p.size for p, _ in first[key]] == [p.size for p, _ in second[key]]
        assert all(not np.array_equal(a[1], b[1]) for a, b in zip(first[key], second[key]))

    pool = [up(v) for v in first["pool"]]
    rec_wires = [(up(p), up(o)) for p, o in first["rec_wires"]]
    sum_wires = [(up(p), up(o)) for p, o in first["sum_wires"]]
    enc_vec = up(first["enc_vec"])
    frames = [up(f) for f, _ in first["frames"]]
    out5, outG, out_sum = (torch.zeros(vb, dtype=torch.uint8, device=dev()) for _ in range(3))
    enc_frame = torch.zeros(codec.frame_capacity(n, x), dtype=torch.uint8, device=dev())
    enc_offs = torch.zeros(n + 1, dtype=torch.int64, device=dev())
    open_offs = [torch.zeros(n + 1, dtype=torch.int64, device=dev()) for _ in xs2]
    rec_flag, sum_flag, frame_flag = (torch.zeros(2, dtype=torch.int32, device=dev()) for _ in range(3))
    wrong_xs = [xs2[0], xs2[1] + 1]  # open_frames: frame 1's header carries another abscissa, counted once per call
    res = {}

    def sequence():
        ss.sum_shares_vec(pool[:5], out=out5)
        ss.sum_shares_vec([pool[i % 7] for i in range(M5)], signs=signs, out=outG)
        res["rec"] = ss.resolve_records_vec(rec_wires, xs2, n, bad=rec_flag)
        ss.sum_records_vec(sum_wires, x, n, signs=[1, -1, 1], out=out_sum, bad=sum_flag)
        codec.encode_share_frame(enc_vec, n, x, trim=False, out=enc_frame, offsets=enc_offs)
        res["open"] = codec.open_frames(frames, n, wrong_xs, offsets=open_offs, bad=frame_flag)

    def check(d, calls: int, what: str):
        assert torch.equal(out5, up(d["sum5"])), what
        assert torch.equal(outG, up(d["sumG"])), what
        assert torch.equal(res["rec"].cpu(), torch.from_numpy(d["rec_want"])), what
        assert torch.equal(out_sum, up(d["sum_want"])), what
        want_frame, want_offs = d["enc_want"]
        assert torch.equal(enc_frame[: want_frame.size], up(want_frame)) and torch.equal(enc_offs, up(want_offs)), what
        for (packed, offs), buf, frame, (_, want) in zip(res["open"], open_offs, frames, d["frames"]):
            assert offs.data_ptr() == buf.data_ptr() and packed.data_ptr() == frame.data_ptr() + R_of(n), what
            assert torch.equal(buf, up(want)), what
        assert (rec_flag.tolist(), sum_flag.tolist(), frame_flag.tolist()) == ([0, 0], [2 * calls, 0], [calls, 0]), what

    def clear(flags: bool):
        for t in (out5, outG, out_sum, enc_frame, enc_offs, *open_offs) + ((rec_flag, sum_flag, frame_flag) if flags
                                                                          else ()):
            t.zero_()
        if "rec" in res:
            res["rec"].zero_()

    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        sequence()  # the eager call, on the capture stream
    torch.cuda.synchronize()
    check(first, 1, "the eager calls")
    clear(flags=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        sequence()
    torch.cuda.synchronize()
    assert sum_flag.tolist() == [0, 0] and not bool(out5.any())  # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    check(first, 1, "the first replay")

    for t, a in zip(pool, second["pool"]):
        t.copy_(torch.from_numpy(a))
    for key, held in (("rec_wires", rec_wires), ("sum_wires", sum_wires)):
        for (p, o), (hp, ho) in zip(held, second[key]):
            p.copy_(torch.from_numpy(hp))
            o.copy_(torch.from_numpy(ho))
    enc_vec.copy_(torch.from_numpy(second["enc_vec"]))
    for f, (hf, _) in zip(frames, second["frames"]):
        f.copy_(torch.from_numpy(hf))
    clear(flags=False)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    check(second, 2, "the second replay, over rewritten inputs")
