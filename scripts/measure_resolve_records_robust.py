#!/usr/bin/env python3
"""resolve_records_vec_robust against the routes it replaces, on records of
the fused split's shares.

Shapes: 3-of-5 with all five wires (xs 1..5) and 5-of-9 with all nine (xs
1..9), each at 2^24 and 2^20 elements, out="field" and out="int64", clean; and
3-of-5 at 2^24 with wire 2 replaced whole by the records of another sharing's
row.  The wires are what a receiver holds: codec.encode_share_vec of the rows
of make_shares_vec.  Before anything is timed the new call's result, counts and
culprit bytes are compared with route a's at the timed size; a difference ends
the run.  Rows, each timed with device events around one pass that ends in a
synchronise, REPS passes after a warm-up, the rows of a shape alternating
within this one process, every flag deferred:
  a  k decode_share_vec into caller buffers, then resolve_shares_vec_robust
  b  (clean shapes) check_records_vec, then resolve_records_vec
  n  resolve_records_vec_robust
With --parent-lib PATH (a build of the parent commit's library) rows a and b
are also taken on that library: the baseline is then not the code under test.
The bar: row n's slowest pass below row a's fastest.
Writes profiles/r22/resolve_records_robust.json and prints it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 20
SHAPES = [("3of5_2e24", 3, 5, 1 << 24, False), ("3of5_2e20", 3, 5, 1 << 20, False),
          ("5of9_2e24", 5, 9, 1 << 24, False), ("5of9_2e20", 5, 9, 1 << 20, False),
          ("3of5_2e24_wire2_bad", 3, 5, 1 << 24, True)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libdn_shamir.so built from the parent commit (rows a and b on it too)")
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--shapes", help="comma-separated subset of " + ",".join(c[0] for c in SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "resolve_records_robust.json"))
    args = ap.parse_args()
    assert args.reps >= 20, "at least 20 repetitions"

    sys.path.insert(0, os.path.join(ROOT, "delta-node_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch

    from delta_node.crypto import shamir
    from delta_node.crypto.shamir import _native, codec, field
    from golden.fixtures import secrets_int64

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    res = {"lib": os.path.basename(_native.lib_path()),
           "parent_lib": os.path.basename(args.parent_lib) if args.parent_lib else None, "reps": args.reps,
           "shapes": {}}
    wanted = args.shapes.split(",") if args.shapes else [c[0] for c in SHAPES]

    def one_pass(fn, lib_path):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if lib_path:
            with _native.library(lib_path):
                s.record(stream)
                fn()
                e.record(stream)
                torch.cuda.synchronize()
        else:
            s.record(stream)
            fn()
            e.record(stream)
            torch.cuda.synchronize()
        return s.elapsed_time(e)

    def wires_of(ss, sec, k, n, seed):
        ss.random.seed(seed)
        block = ss.make_shares_vec(sec, k)
        out = []
        for x in range(1, k + 1):
            p, o = codec.encode_share_vec(block[x - 1], n, x)
            out.append((p.clone(), o))  # the trimmed view's own allocation
        return out

    for name, t, k, n, damaged in SHAPES:
        if name not in wanted:
            continue
        xs = list(range(1, k + 1))
        sec = torch.from_numpy(secrets_int64(5, n)).to(dev)
        ss = shamir.SecretShare(t)
        wires = wires_of(ss, sec, k, n, 9)
        if damaged:
            wires[2] = wires_of(ss, sec, k, n, 10)[2]  # another polynomial's share 3 under every element
        torch.cuda.empty_cache()
        dec_out = [torch.empty(field.vec_bytes(n), dtype=torch.uint8, device=dev) for _ in xs]
        dec_xs = [torch.empty(n, dtype=torch.int64, device=dev) for _ in xs]
        flag1 = torch.zeros(1, dtype=torch.int32, device=dev)
        counts = torch.zeros(2, dtype=torch.int32, device=dev)
        recs = torch.zeros(2, dtype=torch.int32, device=dev)
        shape = {"threshold": t, "xs": xs, "n": n, "wire_bytes": [p.numel() for p, _ in wires], "out": {}}

        for out in ("field", "int64"):
            def row_a(culprit=False):
                got = [codec.decode_share_vec(p, o, n, out=b, xs=x, bad=flag1)[0]
                       for (p, o), b, x in zip(wires, dec_out, dec_xs)]
                return ss.resolve_shares_vec_robust(got, xs, n, out=out, culprit=culprit, bad=counts)

            def row_b():
                ss.check_records_vec(wires, xs, n, bad=counts, bad_records=recs)
                ss.resolve_records_vec(wires, xs, n, out=out, bad=recs)

            def row_n(culprit=False):
                return ss.resolve_records_vec_robust(wires, xs, n, out=out, culprit=culprit, bad=counts,
                                                     bad_records=recs)

            # the results at the timed size, before timing
            counts.zero_()
            want, _, want_marks = row_a(True)
            want_counts = counts.tolist()
            counts.zero_()
            got, _, got_marks = row_n(True)
            if not (torch.equal(got, want) and torch.equal(got_marks, want_marks) and counts.tolist() == want_counts
                    and recs.tolist() == [0, 0] and int(flag1.item()) == 0):
                sys.exit(f"measure_resolve_records_robust: {name} {out}: the new call and route a differ")
            if want_counts != ([n, n] if damaged else [0, 0]) or (out == "int64" and not torch.equal(got, sec)):
                sys.exit(f"measure_resolve_records_robust: {name} {out}: counts {want_counts} or secrets not as built")
            del want, want_marks, got, got_marks

            todo = {"a_decode_then_robust": (row_a, None), "n_resolve_records_robust": (row_n, None)}
            if not damaged:
                todo["b_check_then_resolve_records"] = (row_b, None)
            if args.parent_lib:
                todo["a_decode_then_robust_parent"] = (row_a, args.parent_lib)
                if not damaged:
                    todo["b_check_then_resolve_records_parent"] = (row_b, args.parent_lib)
            times = {r: [] for r in todo}
            for fn, path in todo.values():  # warm-up
                one_pass(fn, path)
                one_pass(fn, path)
            for _ in range(args.reps):
                for r, (fn, path) in todo.items():
                    times[r].append(one_pass(fn, path))
            rows = {r: {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts),
                        "mean_ms": statistics.fmean(ts)} for r, ts in times.items()}
            sfx = "_parent" if args.parent_lib else ""
            new, base = rows["n_resolve_records_robust"], rows["a_decode_then_robust" + sfx]
            acc = {"baseline": "parent library" if args.parent_lib else "this library (no --parent-lib)",
                   "a_over_n_median": base["median_ms"] / new["median_ms"],
                   "n_slowest_below_a_fastest": new["max_ms"] < base["min_ms"]}
            if not damaged:
                acc["b_over_n_median"] = rows["b_check_then_resolve_records" + sfx]["median_ms"] / new["median_ms"]
            shape["out"][out] = {"counts": want_counts, "rows": rows, "acceptance": acc}
        res["shapes"][name] = shape
        del wires, dec_out, dec_xs, sec
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
