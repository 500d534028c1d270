#!/usr/bin/env python3
"""Wire frames against the framing scripts/e2e_round.py does by hand with
torch ops, at 2^24 elements, abscissa x = 3, on one MI355X.

Before timing, the routes' outputs are compared bit for bit (record bytes,
lengths, offsets); a mismatch ends the run.  Every row is timed with device
events around one pass that ends in a synchronise, REPS passes after a
warm-up, the rows alternating within this one process.

Sender rows, all into caller buffers without trim:
  a  a lone codec.encode_share_vec
  b  a plus e2e_round.py's framing ops as written there (lengths by a
     difference cast to uint8, a fresh `plain`, the records copied in, the
     lengths copied in behind them)
  c  codec.encode_share_frame
Receiver rows, from a plaintext already on the device:
  d  e2e_round.py's four torch ops (two slices, a cast to int64, zeros(n + 1),
     cumsum)
  e  codec.open_frames with m = 1, a deferred `bad`, a caller's offsets
  f  ten times d, against codec.open_frames with m = 10
  g  f followed by sum_records_vec over the ten wires, both ways
Bars (orderings, no ratio fixed in advance): c's slowest repetition below b's
fastest, e's below d's, the m = 10 open's below ten d's.
Writes profiles/r13/frames.json and prints it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 20
HBM_BYTES_PER_S = 8.0e12
X = 3
SHARES = 5
M = 10


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--n", type=int, default=1 << 24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "frames.json"))
    args = ap.parse_args()
    assert args.reps >= 20, "at least 20 repetitions"

    sys.path.insert(0, os.path.join(ROOT, "delta-node_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch

    from delta_node.crypto import shamir
    from delta_node.crypto.shamir import _native, codec
    from golden.fixtures import secrets_int64

    assert torch.cuda.is_available(), "measure_frames needs a HIP device"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    n = args.n
    R = codec.frame_records_offset(n)
    cap = codec.encoded_capacity(n, X)
    ss = shamir.SecretShare(3)

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(stream)
        fn()
        e.record(stream)
        torch.cuda.synchronize()
        return s.elapsed_time(e)

    # member j's share for party X, as a tiled vector
    vecs = []
    for j in range(M):
        sec = torch.from_numpy(secrets_int64(100 + j, n)).to(dev)
        ss.random.seed(9 + j)
        block = ss.make_shares_vec(sec, SHARES)
        vecs.append(block[X - 1].clone())
        del block, sec
    vec = vecs[0]

    # ---- sender
    out_a = torch.empty(cap, dtype=torch.uint8, device=dev)
    offs_a = torch.empty(n + 1, dtype=torch.int64, device=dev)
    frame_c = torch.empty(R + cap, dtype=torch.uint8, device=dev)
    offs_c = torch.empty(n + 1, dtype=torch.int64, device=dev)
    codec.encode_share_vec(vec, n, X, trim=False, out=out_a, offsets=offs_a)
    nb = int(offs_a[n].item())  # the record bytes: known to the rows below, as a caller without trim knows it
    keep = {}

    def row_a():
        codec.encode_share_vec(vec, n, X, trim=False, out=out_a, offsets=offs_a)

    def row_b():
        recs, offs = codec.encode_share_vec(vec, n, X, trim=False, out=out_a, offsets=offs_a)
        recs = recs[:nb]
        lens = (offs[1:] - offs[:-1]).to(torch.uint8)
        plain = torch.empty(nb + n, dtype=torch.uint8, device=dev)
        plain[:nb].copy_(recs)
        plain[nb:].copy_(lens)
        keep["plain"] = plain

    def row_c():
        codec.encode_share_frame(vec, n, X, trim=False, out=frame_c, offsets=offs_c)

    row_b()
    row_c()
    torch.cuda.synchronize()
    plain = keep["plain"]
    if not (torch.equal(frame_c[R:R + nb], plain[:nb]) and torch.equal(frame_c[32:32 + n], plain[nb:])
            and torch.equal(offs_c, offs_a) and not bool(frame_c[32 + n:R].any())):
        sys.exit("measure_frames: the frame differs from the hand-made framing")
    fields = codec.frame_fields_host(frame_c[:R + nb].cpu(), n=n, x=X)
    assert fields.records_bytes == nb

    # ---- receiver: M members' plaintexts, both forms
    frames, raws = [], []
    for j in range(M):
        f, o = codec.encode_share_frame(vecs[j], n, X)
        frames.append(f.clone())
        nbj = f.numel() - R
        raw = torch.empty(nbj + n, dtype=torch.uint8, device=dev)
        raw[:nbj].copy_(f[R:])
        raw[nbj:].copy_(f[32:32 + n])
        raws.append((raw, nbj))
        del f, o
    del vecs
    offs_e = [torch.empty(n + 1, dtype=torch.int64, device=dev) for _ in range(M)]
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    flag_sum = torch.zeros(2, dtype=torch.int32, device=dev)
    out_sum = torch.empty(_native.vec_bytes(n), dtype=torch.uint8, device=dev)

    def by_hand(j):
        raw, rec_bytes = raws[j]
        packed = raw[:rec_bytes].to(dev)
        lens = raw[rec_bytes:rec_bytes + n].to(dev).to(torch.int64)
        offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lens, 0, out=offsets[1:])
        return packed, offsets

    def row_d():
        keep["d"] = by_hand(0)

    def row_e():
        keep["e"] = codec.open_frames(frames[:1], n, [X], offsets=offs_e[:1], bad=flag)

    def row_f_hand():
        keep["f_hand"] = [by_hand(j) for j in range(M)]

    def row_f_open():
        keep["f_open"] = codec.open_frames(frames, n, [X] * M, offsets=offs_e, bad=flag)

    def row_g_hand():
        ss.sum_records_vec([by_hand(j) for j in range(M)], X, n, out=out_sum, bad=flag_sum)

    def row_g_open():
        ss.sum_records_vec(codec.open_frames(frames, n, [X] * M, offsets=offs_e, bad=flag), X, n, out=out_sum,
                           bad=flag_sum)

    row_f_hand()
    row_f_open()
    torch.cuda.synchronize()
    for (hp, ho), (fp, fo) in zip(keep["f_hand"], keep["f_open"]):
        if not (torch.equal(hp, fp) and torch.equal(ho, fo)):
            sys.exit("measure_frames: open_frames differs from the hand-made offsets")
    row_g_hand()
    want_sum = out_sum.clone()
    row_g_open()
    torch.cuda.synchronize()
    if not torch.equal(out_sum, want_sum) or flag.tolist() != [0, 0] or flag_sum.tolist() != [0, 0]:
        sys.exit("measure_frames: the sums differ, or a flag counted")
    keep.clear()

    todo = {"a_encode_share_vec": row_a, "b_encode_plus_hand_framing": row_b, "c_encode_share_frame": row_c,
            "d_hand_offsets": row_d, "e_open_frames_m1": row_e, "f_hand_offsets_x10": row_f_hand,
            "f_open_frames_m10": row_f_open, "g_hand_x10_then_sum_records": row_g_hand,
            "g_open_m10_then_sum_records": row_g_open}
    times = {r: [] for r in todo}
    for fn in todo.values():  # warm-up
        timed(fn)
        timed(fn)
    for _ in range(args.reps):
        for r, fn in todo.items():
            times[r].append(timed(fn))
            keep.clear()
    if flag.tolist() != [0, 0] or flag_sum.tolist() != [0, 0]:
        sys.exit("measure_frames: a flag counted during the timed passes")
    rows = {r: {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts),
                "mean_ms": statistics.fmean(ts)} for r, ts in times.items()}
    open_bytes = 2 * frame_pad(n) + 8 * (n + 1)  # the lengths twice, the offsets once
    res = {"lib": os.path.basename(_native.lib_path()), "reps": args.reps, "n": n, "x": X, "m": M,
           "record_bytes": nb, "frame_bytes": R + nb, "outputs_equal": True, "rows": rows,
           "hbm_bytes_per_s": HBM_BYTES_PER_S,
           "bars": {"c_slowest_below_b_fastest":
                    rows["c_encode_share_frame"]["max_ms"] < rows["b_encode_plus_hand_framing"]["min_ms"],
                    "e_slowest_below_d_fastest": rows["e_open_frames_m1"]["max_ms"] < rows["d_hand_offsets"]["min_ms"],
                    "open_m10_slowest_below_ten_d_fastest":
                    rows["f_open_frames_m10"]["max_ms"] < rows["f_hand_offsets_x10"]["min_ms"]},
           "report": {"c_minus_a_median_ms": rows["c_encode_share_frame"]["median_ms"]
                      - rows["a_encode_share_vec"]["median_ms"],
                      "b_minus_a_median_ms": rows["b_encode_plus_hand_framing"]["median_ms"]
                      - rows["a_encode_share_vec"]["median_ms"],
                      "e_bytes": open_bytes,
                      "e_fraction_of_hbm": open_bytes / (rows["e_open_frames_m1"]["median_ms"] * 1e-3) / HBM_BYTES_PER_S,
                      "g_hand_over_open_median": rows["g_hand_x10_then_sum_records"]["median_ms"]
                      / rows["g_open_m10_then_sum_records"]["median_ms"]}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def frame_pad(n: int) -> int:
    return (n + 15) & ~15


if __name__ == "__main__":
    main()
