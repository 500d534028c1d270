#!/usr/bin/env python3
"""The tiled-row check family on this build against the parent's.

Three libraries, each loaded once: this build, the library built from the parent
commit (`make -C delta-node_amd ab REF=<rev>`) and a copy of that file, loaded a
second time for the day's noise.  The calls and shapes are those of
measure_check.py, measure_check_records.py and measure_resolve_robust.py
(deferred flags, 3-of-5 and 5-of-9, 2^24 elements; the records form at 2^20 too).
Device events around each call, --reps alternating repetitions; the three
libraries' results are compared at the timed size before anything is timed.
A row passes when this build's median is no higher than the larger parent median
plus the distance between the two.  Writes one JSON document.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", required=True, help="libdn_shamir.so built from the parent commit")
    ap.add_argument("--parent-copy", required=True, help="a copy of that file under another name")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", help="comma-separated substrings: only rows whose name holds one of them")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "rows_ab.json"))
    args = ap.parse_args()

    sys.path.insert(0, os.path.join(ROOT, "delta-node_amd"))
    import torch

    from delta_node.crypto import shamir
    from delta_node.crypto.shamir import _native, codec

    dev = torch.device("cuda", 0)
    libs = {"now": _native.lib(), "parent": _native._load(args.parent_lib),
            "parent_again": _native._load(args.parent_copy)}
    n24 = 1 << 24
    values = torch.randint(-(1 << 62), 1 << 62, (n24,), dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    recs = torch.zeros(2, dtype=torch.int32, device=dev)
    rows = {}  # name -> call returning the tensors to compare

    for t, k in ((3, 5), (5, 9)):
        tag = f"{t}of{k}"
        ss, xs = shamir.SecretShare(t), list(range(1, k + 1))
        ss.random.seed(t)
        vecs = list(ss.make_shares_vec(values, k).unbind(0))

        def check(culprit, ss=ss, xs=xs, vecs=vecs):
            return ss.check_shares_vec(vecs, xs, n24, culprit=culprit, bad=counts)

        def robust(out, ss=ss, xs=xs, vecs=vecs):
            return ss.resolve_shares_vec_robust(vecs, xs, n24, out=out, culprit=True, bad=counts)

        rows[f"check_{tag}_2e24_count"] = lambda f=check: f(False)
        if t == 3:
            rows[f"check_{tag}_2e24_culprit"] = lambda f=check: f(True)
        rows[f"robust_{tag}_2e24_field"] = lambda f=robust: f("field")
        rows[f"robust_{tag}_2e24_int64"] = lambda f=robust: f("int64")
        if t == 3:
            wire = list(vecs)
            wire[2] = vecs[3]  # a whole wire of well-formed field elements that are not its shares
            rows[f"robust_{tag}_2e24_field_badwire"] = lambda ss=ss, xs=xs, wire=wire: ss.resolve_shares_vec_robust(
                wire, xs, n24, out="field", culprit=True, bad=counts)
        for log2n in (24, 20):
            n = 1 << log2n
            small = vecs if n == n24 else list(ss.make_shares_vec(values[:n].contiguous(), k).unbind(0))
            wires = []
            for x in xs:
                p, o = codec.encode_share_vec(small[x - 1], n, x)
                wires.append((p.clone(), o))  # the trimmed view's own allocation

            def records(culprit, ss=ss, xs=xs, wires=wires, n=n):
                return ss.check_records_vec(wires, xs, n, culprit=culprit, bad=counts, bad_records=recs)

            rows[f"check_records_{tag}_2e{log2n}_count"] = lambda f=records: f(False)
            rows[f"check_records_{tag}_2e{log2n}_culprit"] = lambda f=records: f(True)

    if args.rows:
        rows = {r: f for r, f in rows.items() if any(s in r for s in args.rows.split(","))}

    def on(lib, f):
        _native._lib = libs[lib]
        try:
            return f()
        finally:
            _native._lib = libs["now"]

    def tensors(x):
        return [y for y in (x if isinstance(x, (tuple, list)) else [x]) if isinstance(y, torch.Tensor)]

    for name, f in rows.items():  # warm-up, and the same results at the timed size
        ref = [y.clone() for y in tensors(on("parent", f))]
        for lib in ("now", "parent_again"):
            got = tensors(on(lib, f))
            assert len(got) == len(ref) and all(torch.equal(a, b) for a, b in zip(got, ref)), (name, lib)
    torch.cuda.synchronize()
    ms = {name: {lib: [] for lib in libs} for name in rows}
    for _ in range(args.reps):
        for name, f in rows.items():
            for lib in ("parent", "now", "parent_again"):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                on(lib, f)
                t1.record()
                t1.synchronize()
                ms[name][lib].append(t0.elapsed_time(t1))
    result = {"reps": args.reps, "device": torch.cuda.get_device_name(0), "rows": {}}
    for name, by in ms.items():
        med = {lib: statistics.median(v) for lib, v in by.items()}
        bar = max(med["parent"], med["parent_again"]) + abs(med["parent"] - med["parent_again"])
        result["rows"][name] = {"ms": by, "median_ms": med, "min_ms": {lib: min(v) for lib, v in by.items()},
                                "max_ms": {lib: max(v) for lib, v in by.items()}, "bar_ms": bar,
                                "passes": med["now"] <= bar}
        print(f"{name}: " + "  ".join(f"{lib} {med[lib]:.4f} ({min(by[lib]):.4f}-{max(by[lib]):.4f})" for lib in by)
              + f"  bar {bar:.4f}  {'passes' if med['now'] <= bar else 'MISSES'}", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
