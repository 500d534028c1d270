#!/usr/bin/env python3
"""commit_records_vec / verify_records_vec against the route they replace —
a device-to-host copy of the wire, codec.records_to_list and hashlib.sha256
per record on one core — and against the kernel's instruction-mix bound.

One configuration: 2^24 elements, abscissa x = 3, a 16-byte aligned wire
(codec.encode_share_vec of a random tiled vector of 521-bit values: records of
68 bytes, two SHA-256 blocks each).  Before timing, the digests of the first
and the last 4096 records are compared with hashlib and the verify's flag is
checked; a mismatch ends the run.  Rows a-c are timed with device events
around one pass that ends in a synchronise, REPS passes after a warm-up,
alternating within this one process; medians are reported:
  a  commit_records_vec into a caller's out, with a deferred `bad`
  b  verify_records_vec of those commitments, with a deferred `bad`
  c  encode_share_vec (trim=False, caller buffers) on the same build, for scale
  d  the host route at 2^20 records, wall clock, three passes: the D2H copy of
     the wire and offsets, records_to_list, hashlib per record.  Its time at
     2^24 is the median SCALED LINEARLY by 16 (the route is per-record work on
     one core; 2^24 bytes objects would only add allocator pressure)
The instruction-mix bound prices the VALU instructions of one record — two
trips of the block loop on the LDS path plus the code around it, counted from
the built ISA of sha_records_kernel<false> (DESIGN.md §4.23 gives the counts
by opcode) — with the measured issue rates of DESIGN.md §4.10: a half-rate
instruction takes two full-rate slots.
Writes profiles/r16/commit.json and prints it."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 20
X = 3
N = 1 << 24
N_HOST = 1 << 20
# VALU instructions per trip of the block loop (LDS path) and around the loop, from the ISA
FULL_PER_BLOCK, HALF_PER_BLOCK = 672, 948
FULL_OUTSIDE, HALF_OUTSIDE = 100, 16
FULL_RATE = (6.0e13, 6.5e13)  # lane-ops/s, DESIGN.md §4.10


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--n-host", type=int, default=N_HOST)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "commit.json"))
    args = ap.parse_args()
    assert args.reps >= 20, "at least 20 repetitions"

    sys.path.insert(0, os.path.join(ROOT, "delta-node_amd"))
    import numpy as np
    import torch

    from delta_node.crypto.shamir import _native, codec, field

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    n = args.n

    # a tiled vector of random 521-bit values, filled on the device
    vb = field.vec_bytes(n)
    gen = torch.Generator(device=dev)
    gen.manual_seed(16)
    vec = torch.randint(0, 256, (vb,), dtype=torch.uint8, device=dev, generator=gen)
    tiles = vec.view(-1, field.TILE_BYTES)
    tiles[:, 64 * field.TILE + 1::2] = 1  # the top plane (uint16 per element): bit 520 set, bits 521.. clear
    cap = codec.encoded_capacity(n, X)
    wire = torch.empty(cap, dtype=torch.uint8, device=dev)
    offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    packed, offsets = codec.encode_share_vec(vec, n, X, out=wire, offsets=offs)
    assert packed.data_ptr() % 16 == 0
    out = torch.empty(32 * n, dtype=torch.uint8, device=dev)
    flag = torch.zeros(2, dtype=torch.int32, device=dev)

    def row_a():
        codec.commit_records_vec(packed, offsets, n, out=out, bad=flag)

    def row_b():
        codec.verify_records_vec(packed, offsets, n, out, bad=flag)

    def row_c():
        codec.encode_share_vec(vec, n, X, trim=False, out=wire, offsets=offs)

    def one_pass(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(stream)
        fn()
        e.record(stream)
        torch.cuda.synchronize()
        return s.elapsed_time(e)

    # correctness first
    row_a()
    row_b()
    torch.cuda.synchronize()
    if flag.tolist() != [0, 0]:
        sys.exit(f"measure_commit: the flag reads {flag.tolist()}")
    o_host = offsets.cpu().numpy()
    for lo, hi in ((0, min(4096, n)), (max(n - 4096, 0), n)):
        recs = codec.records_to_list(packed[int(o_host[lo]):int(o_host[hi])].cpu(),
                                     torch.from_numpy(o_host[lo:hi + 1] - o_host[lo]))
        want = b"".join(hashlib.sha256(r).digest() for r in recs)
        if bytes(out[32 * lo:32 * hi].cpu().numpy()) != want:
            sys.exit("measure_commit: digests differ from hashlib")
    lens = np.diff(o_host)
    rows = {"a_commit": row_a, "b_verify": row_b, "c_encode": row_c}
    times = {r: [] for r in rows}
    for fn in rows.values():
        one_pass(fn)
    for _ in range(args.reps):
        for r, fn in rows.items():
            times[r].append(one_pass(fn))
    if flag.tolist() != [0, 0]:
        sys.exit("measure_commit: records counted during the timed passes")
    res_rows = {r: {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts),
                    "mean_ms": statistics.fmean(ts)} for r, ts in times.items()}

    # d: the host route at n_host records
    nh = min(args.n_host, n)
    end = int(o_host[nh])
    host_ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        p_host = packed[:end].cpu()
        of_host = offsets[: nh + 1].cpu()
        recs = codec.records_to_list(p_host, of_host)
        digests = [hashlib.sha256(r).digest() for r in recs]
        host_ts.append((time.perf_counter() - t0) * 1e3)
        assert len(digests) == nh
    d_ms = statistics.median(host_ts)
    d_scaled = d_ms * (n / nh)
    res_rows["d_host_route"] = {"n": nh, "median_ms": d_ms, "min_ms": min(host_ts), "max_ms": max(host_ts),
                                "scaled_linearly_to_n_ms": d_scaled, "scale": n / nh}

    slots = 2 * (FULL_PER_BLOCK + 2 * HALF_PER_BLOCK) + FULL_OUTSIDE + 2 * HALF_OUTSIDE
    bound_ms = [slots * n / r * 1e3 for r in FULL_RATE]  # at the lower and at the upper measured rate
    a_ms = res_rows["a_commit"]["median_ms"]
    res = {"lib": os.path.basename(_native.lib_path()), "reps": args.reps, "n": n, "x": X,
           "wire_bytes": int(o_host[n]), "record_bytes": {"min": int(lens.min()), "max": int(lens.max())},
           "rows": res_rows,
           "instruction_mix": {"full_rate_per_block": FULL_PER_BLOCK, "half_rate_per_block": HALF_PER_BLOCK,
                               "full_rate_outside_loop": FULL_OUTSIDE, "half_rate_outside_loop": HALF_OUTSIDE,
                               "full_rate_slots_per_two_block_record": slots, "full_rate_lane_ops_per_s": FULL_RATE,
                               "bound_ms": {"at_low_rate": bound_ms[0], "at_high_rate": bound_ms[1]},
                               "fraction_of_bound_reached": {"at_low_rate": bound_ms[0] / a_ms,
                                                             "at_high_rate": bound_ms[1] / a_ms}},
           "ratios": {"d_scaled_over_a": d_scaled / a_ms, "b_over_a": res_rows["b_verify"]["median_ms"] / a_ms,
                      "a_over_c": a_ms / res_rows["c_encode"]["median_ms"]},
           "bytes": {"a": int(o_host[n]) + 8 * (n + 1) + 32 * n},
           "note": "row d is timed at n_host records and scaled linearly to n"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
