#!/usr/bin/env python3
"""sum_shares_vec against the only route a caller had before it: the private
`_native.reconstruct` with all-ones weights — one launch for m <= 16 vectors,
the 16-wide tree of `_resolve_vectors` (partial sums of 16, then their sum)
beyond that.

Rows (m vectors of N random field elements each, drawn on the device):
  m3_2e24    m = 3,  N = 2^24   the parent's unrolled, prefetched K = 3 kernel
  m10_2e24   m = 10, N = 2^24   the parent's runtime-K kernel
  m40_2e22   m = 40, N = 2^22   the parent's tree: 3 partial sums + 1
  m10_2e20   m = 10, N = 2^20
Before timing, the two routes' outputs are compared on the device; a mismatch
ends the run.  Each row is timed with device events around one pass that ends
in a synchronise, REPS passes after a warm-up, the two routes alternating
within this one process.  Recorded per row and route: median, minimum and
maximum, the algorithmic bytes (m + 1) * 66 * N and their fraction of 8 TB/s
at the median.
With --parent-lib PATH (a build of the parent commit's library) the old route
runs on that library — the baseline is then not the code under test.
Writes profiles/r09/share_sum.json and prints it."""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 20
PEAK = 8e12  # B/s
ROWS = [("m3_2e24", 3, 1 << 24), ("m10_2e24", 10, 1 << 24), ("m40_2e22", 40, 1 << 22), ("m10_2e20", 10, 1 << 20)]
G = 16  # _native.MAX_RESOLVE: the old route's widest launch


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libdn_shamir.so built from the parent commit (the old route runs on it)")
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "share_sum.json"))
    ap.add_argument("--only", help="run one variant REPS times and exit (for a kernel trace), e.g. m10_2e24_new")
    args = ap.parse_args()
    assert args.reps >= 20 or args.only, "at least 20 repetitions"

    sys.path.insert(0, os.path.join(ROOT, "delta-node_amd"))
    import torch

    from delta_node.crypto import shamir
    from delta_node.crypto.shamir import _native, field

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    ss = shamir.SecretShare(3)

    def draw(m, n, seed):
        """m tiled vectors of n field elements in [1, p - 1], ten rows per device draw."""
        vb = field.vec_bytes(n)
        vecs = []
        for g in range(0, m, 10):
            blk = torch.empty((min(10, m - g), vb), dtype=torch.uint8, device=dev)
            if not _native.mt_draw_coeffs_device(random.Random(seed + g), n, blk.shape[0], blk):
                sys.exit("measure_share_sum: the device draw was refused")
            vecs.extend(blk.unbind(0))
        return vecs

    big = draw(10, 1 << 24, 1)
    inputs = {"m3_2e24": big[:3], "m10_2e24": big, "m40_2e22": draw(40, 1 << 22, 100), "m10_2e20": draw(10, 1 << 20, 200)}

    def old_route(vecs, n, out, parts):
        """One all-ones reconstruct, or the 16-wide tree (parts: the partial vectors, made beforehand)."""
        if len(vecs) <= G:
            _native.reconstruct(vecs, _native.ones_weights(len(vecs)), out_fe=out, n=n)
            return out
        for part, g in zip(parts, range(0, len(vecs), G)):
            _native.reconstruct(vecs[g:g + G], _native.ones_weights(len(vecs[g:g + G])), out_fe=part, n=n)
        _native.reconstruct(parts, _native.ones_weights(len(parts)), out_fe=out, n=n)
        return out

    todo, meta = {}, {}
    for name, m, n in ROWS:
        vecs = inputs[name]
        vb = field.vec_bytes(n)
        out_new = torch.empty(vb, dtype=torch.uint8, device=dev)
        out_old = torch.empty(vb, dtype=torch.uint8, device=dev)
        parts = [torch.empty(vb, dtype=torch.uint8, device=dev) for _ in range(0, m, G)] if m > G else []
        assert len(parts) <= G
        todo[f"{name}_new"] = (lambda vecs=vecs, o=out_new: ss.sum_shares_vec(vecs, out=o), None)
        todo[f"{name}_old"] = (lambda vecs=vecs, n=n, o=out_old, parts=parts: old_route(vecs, n, o, parts),
                               args.parent_lib)
        meta[name] = {"m": m, "n": n, "bytes": (m + 1) * 66 * n,
                      "old_route": "one reconstruct, all-ones weights" if m <= G else
                      f"{len(parts)} all-ones reconstructs of up to {G} vectors, then one of their {len(parts)} results"}
    if args.only:
        todo = {args.only: todo[args.only]}

    def one_pass(fn, lib_path):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if lib_path:
            with _native.library(lib_path):
                s.record(stream)
                out = fn()
                e.record(stream)
                torch.cuda.synchronize()
        else:
            s.record(stream)
            out = fn()
            e.record(stream)
            torch.cuda.synchronize()
        return s.elapsed_time(e), out

    res = {"lib": os.path.basename(_native.lib_path()), "parent_lib": args.parent_lib, "reps": args.reps,
           "peak_bytes_per_s": PEAK}
    outs = {}
    for k, (fn, lib_path) in todo.items():  # warm-up; the outputs kept for the comparison
        one_pass(fn, lib_path)
        outs[k] = one_pass(fn, lib_path)[1]
    if not args.only:
        for name, _, _ in ROWS:  # whole tiles: every byte is a live lane
            if not torch.equal(outs[f"{name}_new"], outs[f"{name}_old"]):
                sys.exit(f"measure_share_sum: {name}: the two routes differ")
        res["outputs_equal"] = True
    times = {k: [] for k in todo}
    for name, _, _ in ROWS:  # a row's two routes alternate
        pair = [k for k in todo if k.startswith(name + "_")]
        for _ in range(args.reps):
            for k in pair:
                times[k].append(one_pass(*todo[k])[0])
    rows = {}
    for k, ts in times.items():
        b = meta[k.rsplit("_", 1)[0]]["bytes"]
        med = statistics.median(ts)
        rows[k] = {"median_ms": med, "min_ms": min(ts), "max_ms": max(ts), "bytes": b,
                   "fraction_of_8TBps": b / (med * 1e-3) / PEAK}
    res["rows"] = rows
    res["shapes"] = meta
    if not args.only:
        new = {n: rows[f"{n}_new"] for n, _, _ in ROWS}
        old = {n: rows[f"{n}_old"] for n, _, _ in ROWS}
        acc = {"baseline": "parent library" if args.parent_lib else "this library (no --parent-lib)"}
        acc["m3_new_median_within_parent_spread_or_better"] = new["m3_2e24"]["median_ms"] <= old["m3_2e24"]["max_ms"]
        acc["m10_new_median_below_parent_median"] = new["m10_2e24"]["median_ms"] < old["m10_2e24"]["median_ms"]
        acc["m40_new_median_below_parent_median"] = new["m40_2e22"]["median_ms"] < old["m40_2e22"]["median_ms"]
        for n, _, _ in ROWS:
            acc[f"{n}_old_over_new"] = old[n]["median_ms"] / new[n]["median_ms"]
        # the project's yardstick for read-dominated streaming: the parent's K = 3 row of this run
        acc["m10_new_fraction_at_or_above_parent_m3_fraction"] = (new["m10_2e24"]["fraction_of_8TBps"]
                                                                  >= old["m3_2e24"]["fraction_of_8TBps"])
        acc["met"] = all(acc[k] for k in ("m3_new_median_within_parent_spread_or_better",
                                          "m10_new_median_below_parent_median",
                                          "m40_new_median_below_parent_median"))
        res["acceptance"] = acc
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
