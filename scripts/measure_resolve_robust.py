#!/usr/bin/env python3
"""resolve_shares_vec_robust next to the route a caller had before it.

Device events around each form, REPS alternating repetitions, at 2^24 elements,
deferred flags wherever the form allows them:
  clean data, 3-of-5 on xs 1..5 and 5-of-9 on xs 1..9
    new    resolve_shares_vec_robust(culprit=True, bad=flag), out="field" and "int64"
    route  check_shares_vec(culprit=True, bad=flag), then resolve_shares_vec over
           the first t rows, out="field" and "int64" (the five-limb reconstruct)
  one bad wire, 3-of-5 (row 2 replaced)
    new    as above, out="field"
    route  the check, a read-back of the culprits that occur and one
           resolve_shares_vec(out="field") per culprit over t of the rows without
           it; here one culprit covers every element, so the torch.where that
           would stitch several is not even paid for
--baseline-lib names the library the route runs on (the parent revision's build:
`make -C delta-node_amd ab REF=<rev>`); without it the route runs on this build,
whose check and reconstruct kernels are the same text.
The bar: the new call's slowest repetition below the route's
fastest, for out="field" at each of the three shapes.  Results are compared at the
timed size before anything is timed.  Writes one JSON document.
"""
import argparse
import contextlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "delta-node_amd"))

from delta_node.crypto import shamir  # noqa: E402
from delta_node.crypto.shamir import _native  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "resolve_robust.json"))
    args = ap.parse_args()
    n = 1 << args.log2n
    dev = torch.device("cuda", 0)
    values = torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, device=dev)
    flag = torch.zeros(2, dtype=torch.int32, device=dev)

    ours = _native.lib()
    theirs = _native._load(args.baseline_lib) if args.baseline_lib else ours  # loaded and bound once

    @contextlib.contextmanager
    def parent():
        _native._lib = theirs
        try:
            yield
        finally:
            _native._lib = ours

    def shape(t, k, seed):
        ss, xs = shamir.SecretShare(t), list(range(1, k + 1))
        ss.random.seed(seed)
        rows = list(ss.make_shares_vec(values, k).unbind(0))

        def new(out):
            return ss.resolve_shares_vec_robust(rows, xs, n, out=out, culprit=True, bad=flag)[0]

        def route(out):
            with parent():
                ss.check_shares_vec(rows, xs, n, culprit=True, bad=flag)
                return ss.resolve_shares_vec(rows[:t], xs[:t], n, out=out)

        return ss, xs, rows, new, route

    s3, x5, rows5, new5, route5 = shape(3, 5, 1)
    _, _, _, new9, route9 = shape(5, 9, 2)
    wire = list(rows5)
    wire[2] = rows5[3]  # a whole wire of well-formed field elements that are not its shares

    def new_wire():
        return s3.resolve_shares_vec_robust(wire, x5, n, out="field", culprit=True, bad=flag)[0]

    def route_wire():
        with parent():
            _, marks = s3.check_shares_vec(wire, x5, n, culprit=True, bad=flag)
            occur = torch.unique(marks).tolist()  # the read-back and the host decision
            assert occur == [2], occur  # one culprit covers every element: no torch.where to pay for
            keep = [i for i in range(5) if i != occur[0]][:3]
            return s3.resolve_shares_vec([wire[i] for i in keep], [x5[i] for i in keep], n, out="field")

    forms = {
        "clean_3of5_field_new": lambda: new5("field"), "clean_3of5_field_route": lambda: route5("field"),
        "clean_5of9_field_new": lambda: new9("field"), "clean_5of9_field_route": lambda: route9("field"),
        "wire_3of5_field_new": new_wire, "wire_3of5_field_route": route_wire,
        "clean_3of5_int64_new": lambda: new5("int64"), "clean_3of5_int64_route": lambda: route5("int64"),
        "clean_5of9_int64_new": lambda: new9("int64"), "clean_5of9_int64_route": lambda: route9("int64"),
    }
    # warm up, and the same results at the timed size
    for name in [m for m in forms if m.endswith("_new")]:
        a, b = forms[name](), forms[name[:-3] + "route"]()
        assert torch.equal(a, b), name
    assert torch.equal(new5("int64"), values)
    counts = flag.cpu().tolist()
    flag.zero_()
    ms = {name: [] for name in forms}
    for _ in range(args.reps):
        for name, f in forms.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            f()
            t1.record()
            t1.synchronize()
            ms[name].append(t0.elapsed_time(t1))
    result = {"n_elem": n, "reps": args.reps, "device": torch.cuda.get_device_name(0),
              "route_library": os.path.basename(args.baseline_lib or "this build"), "warmup_counts": counts, "forms": {}, "bar": {}}
    for name, v in ms.items():
        result["forms"][name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "ms": v}
    for name in [m[:-4] for m in forms if m.endswith("_new")]:
        new, route = result["forms"][name + "_new"], result["forms"][name + "_route"]
        result["bar"][name] = {"new_max_ms": new["max_ms"], "route_min_ms": route["min_ms"],
                               "met": new["max_ms"] < route["min_ms"], "gated": "field" in name}
    result["accepted"] = all(b["met"] for b in result["bar"].values() if b["gated"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps({"accepted": result["accepted"], "bar": result["bar"],
                      "median_ms": {m: round(f["median_ms"], 4) for m, f in result["forms"].items()}}))


if __name__ == "__main__":
    main()
