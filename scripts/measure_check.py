#!/usr/bin/env python3
"""check_shares_vec next to the route there was before it.

Device events around each form, REPS alternating repetitions, median and
min-max, at 2^24 elements:
  a  check_shares_vec, 3-of-5 on xs 1..5, count only (deferred: no read-back)
  b  the same with the culprit bytes
  c  5-of-9 on xs 1..9, count only
  d  three resolve_shares_vec(out="field") over {1,2,3}, {1,2,4}, {1,2,5} and
     the torch compares that say whether they agree (and name no culprit)
Writes one JSON document (default profiles/r19/share_check.json).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "delta-node_amd"))

from delta_node.crypto import shamir  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, the figure DESIGN.md states every fraction against


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "share_check.json"))
    args = ap.parse_args()
    n = 1 << args.log2n
    dev = torch.device("cuda", 0)
    values = torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, device=dev)
    s3, s5 = shamir.SecretShare(3), shamir.SecretShare(5)
    s3.random.seed(1)
    s5.random.seed(2)
    rows5 = s3.make_shares_vec(values, 5)
    rows9 = s5.make_shares_vec(values, 9)
    bad = torch.zeros(2, dtype=torch.int32, device=dev)
    x5, x9 = [1, 2, 3, 4, 5], list(range(1, 10))

    def before():
        r = [s3.resolve_shares_vec([rows5[0], rows5[1], rows5[j]], [1, 2, j + 1], n, out="field") for j in (2, 3, 4)]
        return (r[0] != r[1]).any() | (r[0] != r[2]).any()

    forms = {
        "a_check_3of5": lambda: s3.check_shares_vec(rows5, x5, n, bad=bad),
        "b_check_3of5_culprit": lambda: s3.check_shares_vec(rows5, x5, n, culprit=True, bad=bad),
        "c_check_5of9": lambda: s5.check_shares_vec(rows9, x9, n, bad=bad),
        "d_three_resolves_and_compares": before,
    }
    for f in forms.values():  # warm up; the rows are genuine: nothing may be flagged
        f()
    assert s3.check_shares_vec(rows5, x5, n) == 0 and s5.check_shares_vec(rows9, x9, n) == 0
    assert not bool(before())
    assert bad.cpu().tolist() == [0, 0]
    ms = {name: [] for name in forms}
    for _ in range(args.reps):
        for name, f in forms.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            f()
            t1.record()
            t1.synchronize()
            ms[name].append(t0.elapsed_time(t1))
    result = {"n_elem": n, "reps": args.reps, "device": torch.cuda.get_device_name(0), "forms": {}}
    for name, v in ms.items():
        result["forms"][name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "ms": v}
    for name, k in (("a_check_3of5", 5), ("b_check_3of5_culprit", 5), ("c_check_5of9", 9)):
        f = result["forms"][name]
        f["bytes"] = (66 * k + (1 if "culprit" in name else 0)) * n
        f["fraction_of_8TBps"] = f["bytes"] / (f["median_ms"] * 1e-3) / HBM_PEAK
    d = result["forms"]["d_three_resolves_and_compares"]
    a = result["forms"]["a_check_3of5"]
    result["a_faster_than_d_by_ms"] = d["median_ms"] - a["median_ms"]
    result["d_spread_ms"] = d["max_ms"] - d["min_ms"]
    result["accepted"] = result["a_faster_than_d_by_ms"] > 5 * result["d_spread_ms"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps({k: (v if k != "forms" else {m: round(f["median_ms"], 4) for m, f in v.items()})
                      for k, v in result.items()}))


if __name__ == "__main__":
    main()
