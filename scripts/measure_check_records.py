#!/usr/bin/env python3
"""check_records_vec against the route it replaces — decode_share_vec on every
wire, then check_shares_vec — on records of the fused split's shares
(DESIGN.md §4.27).

Configurations: 3-of-5 with all five wires (xs 1..5) and 5-of-9 with all nine
(xs 1..9), each at 2^24 and 2^20 elements, count only.  The wires are what a
receiver holds: codec.encode_share_vec of the rows of make_shares_vec, genuine
sharings, so nothing may be flagged; the counts are checked after the warm-up
and after the timed passes, and a non-zero one ends the run.  Rows, each timed
with device events around one pass that ends in a synchronise, REPS passes
after a warm-up, the rows of a configuration alternating within this one
process:
  a  the existing route as a careful caller runs it: k decode_share_vec into
     caller buffers with a deferred flag, then check_shares_vec (deferred)
  b  check_records_vec with both flags deferred
  c  _native.check_records alone (descriptors and plan made beforehand)
  d  a lone check_shares_vec on ready vectors, for scale
With --parent-lib PATH (a build of the parent commit's library) rows a and d
are also taken on that library: the baseline is then not the code under test.
--culprit times b and c with the culprit bytes as well.
Writes profiles/r20/check_records.json and prints it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 20
HBM_BYTES_PER_S = 8.0e12
CONFIGS = [("3of5_2e24", 3, 5, 1 << 24), ("3of5_2e20", 3, 5, 1 << 20),
           ("5of9_2e24", 5, 9, 1 << 24), ("5of9_2e20", 5, 9, 1 << 20)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libdn_shamir.so built from the parent commit (rows a and d on it too)")
    ap.add_argument("--culprit", action="store_true", help="rows b and c with the culprit bytes as well")
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--configs", help="comma-separated subset of " + ",".join(c[0] for c in CONFIGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20", "check_records.json"))
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
           "hbm_bytes_per_s": HBM_BYTES_PER_S, "configs": {}}
    wanted = args.configs.split(",") if args.configs else [c[0] for c in CONFIGS]

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

    for cname, t, k, n in CONFIGS:
        if cname not in wanted:
            continue
        xs = list(range(1, k + 1))
        sec = torch.from_numpy(secrets_int64(5, n)).to(dev)
        ss = shamir.SecretShare(t)
        ss.random.seed(9)
        block = ss.make_shares_vec(sec, k)
        wires = []
        for x in xs:
            p, o = codec.encode_share_vec(block[x - 1], n, x)
            wires.append((p.clone(), o))  # the trimmed view's own allocation
        vecs = [block[x - 1] for x in xs]
        wire_bytes = [p.numel() for p, _ in wires]
        # caller buffers of the existing route, the culprit bytes, the deferred flags
        dec_out = [torch.empty(field.vec_bytes(n), dtype=torch.uint8, device=dev) for _ in xs]
        dec_xs = [torch.empty(n, dtype=torch.int64, device=dev) for _ in xs]
        flag1 = torch.zeros(1, dtype=torch.int32, device=dev)
        counts = torch.zeros(2, dtype=torch.int32, device=dev)
        recs = torch.zeros(2, dtype=torch.int32, device=dev)
        marks = torch.empty(n, dtype=torch.uint8, device=dev) if args.culprit else None
        plan = _native.check_plan(xs, t)
        desc = [(p.data_ptr(), p.numel(), o.data_ptr()) for p, o in wires]

        def row_a():
            got = [codec.decode_share_vec(p, o, n, out=b, xs=x, bad=flag1)[0]
                   for (p, o), b, x in zip(wires, dec_out, dec_xs)]
            ss.check_shares_vec(got, xs, n, bad=counts)

        def row_b():
            ss.check_records_vec(wires, xs, n, culprit=args.culprit, bad=counts, bad_records=recs)

        def row_c():
            _native.check_records(desc, xs, plan, counts, recs, marks, n)

        def row_d():
            ss.check_shares_vec(vecs, xs, n, bad=counts)

        todo = {"a_decode_then_check": (row_a, None), "b_check_records": (row_b, None), "c_binding": (row_c, None),
                "d_lone_check": (row_d, None)}
        if args.parent_lib:
            todo.update({"a_decode_then_check_parent": (row_a, args.parent_lib),
                         "d_lone_check_parent": (row_d, args.parent_lib)})

        def nothing_flagged(when):
            if int(flag1.sum().item()) or int(counts.sum().item()) or int(recs.sum().item()):
                sys.exit(f"measure_check_records: genuine sharings were flagged {when}")

        times = {r: [] for r in todo}
        for fn, path in todo.values():  # warm-up
            one_pass(fn, path)
            one_pass(fn, path)
        nothing_flagged("in the warm-up")
        for _ in range(args.reps):
            for r, (fn, path) in todo.items():
                times[r].append(one_pass(fn, path))
        nothing_flagged("during the timed passes")
        rows = {r: {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts),
                    "mean_ms": statistics.fmean(ts)} for r, ts in times.items()}
        bytes_b = sum(wire_bytes) + 8 * k * (n + 1) + (n if args.culprit else 0)
        bytes_d = 66 * k * n

        def frac(nbytes, row):
            return nbytes / (rows[row]["median_ms"] * 1e-3) / HBM_BYTES_PER_S

        base = "a_decode_then_check_parent" if args.parent_lib else "a_decode_then_check"
        acc = {"baseline": "parent library" if args.parent_lib else "this library (no --parent-lib)",
               "a_over_b_median": rows[base]["median_ms"] / rows["b_check_records"]["median_ms"],
               "b_slowest_below_a_fastest": rows["b_check_records"]["max_ms"] < rows[base]["min_ms"],
               "b_over_d_median": rows["b_check_records"]["median_ms"] / rows["d_lone_check"]["median_ms"]}
        if args.parent_lib:
            p0 = rows["d_lone_check_parent"]
            acc["d_lone_check_new_over_parent"] = rows["d_lone_check"]["median_ms"] / p0["median_ms"]
        res["configs"][cname] = {
            "threshold": t, "xs": xs, "n": n, "culprit": args.culprit, "wire_bytes": wire_bytes,
            "nothing_flagged": True, "rows": rows,
            "bytes": {"b": bytes_b, "lone_check": bytes_d,
                      "a_route": sum(w + 8 * (n + 1) + 74 * n for w in wire_bytes) + bytes_d},
            "fraction_of_hbm": {"b_check_records": frac(bytes_b, "b_check_records"),
                                "c_binding": frac(bytes_b, "c_binding"), "d_lone_check": frac(bytes_d, "d_lone_check")},
            "acceptance": acc}
        del block, vecs, wires, dec_out, dec_xs, sec
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
