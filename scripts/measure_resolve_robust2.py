#!/usr/bin/env python3
"""The two-error robust reconstruct (errors=2) next to errors=1 and next to the
route a caller had before it.

Device events around each form, REPS alternating repetitions, 5-of-9 on xs 1..9
with all nine rows, out="field", deferred flags, at 2^24 and 2^20 elements, for
the share-vector form and for the records form (wires of encode_share_vec):
  clean     errors=2 against errors=1 (the parent's kernel) on clean data: the
            cost of the capability to the common case.  The bar: the median of
            errors=2 no higher than the slowest repetition of errors=1
  row1      one whole row bad: errors=2 against errors=1, reported
  rows2     two whole rows bad (2 and 7): errors=2 against the only route there
            was: the check with culprits, a read-back (all 0xFE), then per pair
            of rows left out, in the order of the pair bytes, a check over the
            seven others with its read-back until one is consistent, and the
            reconstruct over threshold of those (whole rows: nothing to stitch)
  sparse    two bad shares in one element per 2^10: errors=2, against clean
--baseline-lib names the library the route and errors=1 run on (the parent
revision's build: `make -C delta-node_amd ab REF=<rev>`); without it they run on
this build, whose check, reconstruct and errors=1 kernels are the same text.
Results are compared at the timed size before anything is timed.  Writes one
JSON document with every repetition.
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
from delta_node.crypto.shamir import _native, codec  # noqa: E402

T, K, BAD = 5, 9, (2, 7)
PAIRS = [(i, j) for j in range(K) for i in range(j)]  # the order of the pair bytes


def measure(n, reps, parent):
    dev = torch.device("cuda", 0)
    ss, xs = shamir.SecretShare(T), list(range(1, K + 1))
    ss.random.seed(n)
    values = torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, device=dev)
    flag, rec = (torch.zeros(2, dtype=torch.int32, device=dev) for _ in range(2))
    clean = list(ss.make_shares_vec(values, K).unbind(0))
    truth = ss.resolve_shares_vec(clean[:T], xs[:T], n, out="field")
    # damaged rows: a neighbour's row (well-formed field elements that are not the shares); sparse: bit 0 of
    # the first limb of element 0 of every fourth tile (a tile: 256 elements, 66 * 256 bytes), in both rows
    other = {i: clean[(i + 1) % K] for i in BAD}
    row1 = [other[i] if i == BAD[0] else r for i, r in enumerate(clean)]
    rows2 = [other[i] if i in BAD else r for i, r in enumerate(clean)]
    sparse = list(clean)
    for i in BAD:
        patched = clean[i].clone()
        words = patched.view(torch.int32)
        tiles = torch.arange(0, (n + 255) // 256, 4, device=dev)  # element 0 of every fourth tile: one per 2^10
        words[tiles * (256 * 66 // 4)] ^= 1
        sparse[i] = patched
    as_wires = lambda rows: [codec.encode_share_vec(v, n, x) for v, x in zip(rows, xs)]  # noqa: E731

    def forms(tag, data, robust, check, resolve):
        def route():
            with parent():
                count, marks = check(data["rows2"], xs)
                assert torch.unique(marks).tolist() == [0xFE]  # the read-back and the host decision
                for tried, (i, j) in enumerate(PAIRS):
                    keep = [m for m in range(K) if m not in (i, j)]
                    if check([data["rows2"][m] for m in keep], [xs[m] for m in keep])[0] == 0:
                        return resolve([data["rows2"][m] for m in keep[:T]], [xs[m] for m in keep[:T]])

        def one(rows):
            with parent():
                return robust(rows, 1)

        return {f"{tag}_clean_e1": lambda: one(data["clean"]), f"{tag}_clean_e2": lambda: robust(data["clean"], 2),
                f"{tag}_row1_e1": lambda: one(data["row1"]), f"{tag}_row1_e2": lambda: robust(data["row1"], 2),
                f"{tag}_rows2_route": route, f"{tag}_rows2_e2": lambda: robust(data["rows2"], 2),
                f"{tag}_sparse_e2": lambda: robust(data["sparse"], 2)}

    rows = {"clean": clean, "row1": row1, "rows2": rows2, "sparse": sparse}
    todo = forms("shares", rows,
                 lambda d, e: ss.resolve_shares_vec_robust(d, xs, n, out="field", culprit=True, bad=flag, errors=e)[0],
                 lambda d, x: ss.check_shares_vec(d, x, n, culprit=True),
                 lambda d, x: ss.resolve_shares_vec(d, x, n, out="field"))
    todo.update(forms("records", {name: as_wires(r) for name, r in rows.items()},
                      lambda d, e: ss.resolve_records_vec_robust(d, xs, n, out="field", culprit=True, bad=flag,
                                                                 bad_records=rec, errors=e)[0],
                      lambda d, x: ss.check_records_vec(d, x, n, culprit=True, bad_records=rec),
                      lambda d, x: ss.resolve_records_vec(d, x, n, out="field", bad=rec)))
    for name, f in todo.items():  # warm up, and the same results at the timed size
        assert torch.equal(f(), truth), name
    counts = flag.cpu().tolist()
    ms = {name: [] for name in todo}
    for _ in range(reps):
        for name, f in todo.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            f()
            t1.record()
            t1.synchronize()
            ms[name].append(t0.elapsed_time(t1))
    out = {"n_elem": n, "warmup_counts": counts, "forms": {}, "bar": {}}
    for name, v in ms.items():
        out["forms"][name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "ms": v}
    for tag in ("shares", "records"):
        e1, e2 = out["forms"][tag + "_clean_e1"], out["forms"][tag + "_clean_e2"]
        out["bar"][tag] = {"e2_median_ms": e2["median_ms"], "e1_max_ms": e1["max_ms"], "met": e2["median_ms"] <= e1["max_ms"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="+", default=[24, 20])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23", "resolve_robust2.json"))
    args = ap.parse_args()
    ours = _native.lib()
    theirs = _native._load(args.baseline_lib) if args.baseline_lib else ours  # loaded and bound once

    @contextlib.contextmanager
    def parent():
        _native._lib = theirs
        try:
            yield
        finally:
            _native._lib = ours

    result = {"reps": args.reps, "device": torch.cuda.get_device_name(0), "threshold": T, "shares": K, "bad_rows": BAD,
              "route_library": os.path.basename(args.baseline_lib or "this build"),
              "sizes": [measure(1 << b, args.reps, parent) for b in args.log2n]}
    result["accepted"] = all(b["met"] for s in result["sizes"] for b in s["bar"].values())
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps({"accepted": result["accepted"], "sizes": [
        {"n_elem": s["n_elem"], "bar": s["bar"], "median_ms": {m: round(f["median_ms"], 4) for m, f in s["forms"].items()}}
        for s in result["sizes"]]}))


if __name__ == "__main__":
    main()
