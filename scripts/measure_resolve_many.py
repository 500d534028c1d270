#!/usr/bin/env python3
"""resolve_shares_vec_many against the per-tensor resolve_shares_vec loop,
xs {1, 3, 5} -> int64, over the model-like mix of scripts/measure_many.py
(mix_sizes: 127 tensors totalling 2^24 elements, aligned and +-1 ragged).

The inputs are what the sending side leaves: make_shares_vec_many's per-tensor
blocks of each mix, and one make_shares_vec block of the same 2^24 secrets.
Before timing, every variant's output is compared with the secrets on the
device; a mismatch ends the run.  Rows, each timed with device events around
one pass that ends in a synchronise, REPS passes after a warm-up, the variants
alternating within this one process:
  a  resolve_shares_vec of one 2^24 vector
  b  the per-tensor resolve_shares_vec loop over each mix (today's caller)
  c  resolve_shares_vec_many over each mix: default outs, caller outs, and
     the binding alone (_native.reconstruct_many on address lists made
     beforehand: no per-tensor Python work)
The 2^24 single-vector rows of both libraries alternate among themselves
first, then the mixes' rows.
With --parent-lib PATH (a build of the parent commit's library) rows a and b
are also taken on that library — the baseline is then not the code under
test.  Writes profiles/r08/resolve_many.json and prints it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from measure_many import N_TOTAL, REPS, mix_sizes  # noqa: E402

XS = [1, 3, 5]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libdn_shamir.so built from the parent commit (rows a and b on it too)")
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "resolve_many.json"))
    ap.add_argument("--only", help="run one variant REPS times and exit (for a kernel trace), e.g. c_ragged_default")
    args = ap.parse_args()
    assert args.reps >= 20 or args.only, "at least 20 repetitions"

    sys.path.insert(0, os.path.join(ROOT, "delta-node_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch

    from delta_node.crypto import shamir
    from delta_node.crypto.shamir import _native
    from golden.fixtures import secrets_int64

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    sec = torch.from_numpy(secrets_int64(5, N_TOTAL)).to(dev)
    mixes = {"aligned": mix_sizes(False), "ragged": mix_sizes(True)}
    ss = shamir.SecretShare(3)
    ss.random.seed(9)
    # the three share rows of every tensor, kept as allocations of their own
    # (the split's pooled block is reused by the next split)
    shares = {}
    for name, sizes in mixes.items():
        blocks = ss.make_shares_vec_many(list(torch.split(sec, sizes)), 5)
        shares[name] = [[b[x - 1].clone() for x in XS] for b in blocks]
    blocks = ss.make_shares_vec(sec, 5)
    big = [blocks[x - 1].clone() for x in XS]
    del blocks
    caller_outs = {name: list(torch.split(torch.empty(N_TOTAL, dtype=torch.int64, device=dev), sizes))
                   for name, sizes in mixes.items()}
    res = {"lib": os.path.basename(_native.lib_path()), "parent_lib": args.parent_lib, "reps": args.reps,
           "n_total": N_TOTAL, "tensors": 127, "xs": XS, "out": "int64"}

    weights = _native.lagrange(XS, 3)

    def variants(tag, lib_path):
        """name -> (callable of one pass returning the outputs, library path or None)"""
        v = {f"a_lone_2e24{tag}": (lambda: [ss.resolve_shares_vec(big, XS, N_TOTAL)], lib_path)}
        for name, sizes in mixes.items():
            v[f"b_{name}_loop{tag}"] = (lambda name=name, sizes=sizes: [ss.resolve_shares_vec(sh, XS, n) for sh, n in
                                                                        zip(shares[name], sizes)], lib_path)
            if lib_path is None:
                v[f"c_{name}_default"] = (lambda name=name, sizes=sizes: ss.resolve_shares_vec_many(
                    shares[name], XS, sizes), None)
                v[f"c_{name}_caller"] = (lambda name=name, sizes=sizes: ss.resolve_shares_vec_many(
                    shares[name], XS, sizes, outs=caller_outs[name]), None)
                rows = [v.data_ptr() for sh in shares[name] for v in sh]
                optrs = [o.data_ptr() for o in caller_outs[name]]
                v[f"c_{name}_binding"] = (lambda name=name, sizes=sizes, rows=rows, optrs=optrs: (
                    _native.reconstruct_many(sizes, rows, weights, dev, out_u64_ptrs=optrs), caller_outs[name])[1],
                    None)
        return v

    todo = variants("", None)
    if args.parent_lib:
        todo.update(variants("_parent", args.parent_lib))
    if args.only:
        todo = {args.only: todo[args.only]}

    def one_pass(fn, lib_path, check=None):
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
        if check and not torch.equal(torch.cat(list(out)), sec):
            sys.exit(f"measure_resolve_many: {check} does not reconstruct the secrets")
        return s.elapsed_time(e)

    times = {k: [] for k in todo}
    for k, (fn, lib_path) in todo.items():  # warm-up and correctness: every variant against the secrets
        one_pass(fn, lib_path, check=k)
        one_pass(fn, lib_path)
    res["outputs_equal_secrets"] = True
    for phase in ([k for k in todo if k.startswith("a_")], [k for k in todo if not k.startswith("a_")]):
        for _ in range(args.reps):
            for k in phase:
                times[k].append(one_pass(*todo[k]))
    rows = {}
    for k, ts in times.items():
        rows[k] = {"mean_ms": statistics.fmean(ts), "median_ms": statistics.median(ts), "min_ms": min(ts),
                   "max_ms": max(ts), "stdev_ms": statistics.stdev(ts) if len(ts) > 1 else 0.0}
    res["rows"] = rows
    if not args.only:
        m = {k: r["median_ms"] for k, r in rows.items()}
        base = "_parent" if args.parent_lib else ""
        acc = {"baseline": "parent library" if args.parent_lib else "this library (no --parent-lib)"}
        lone = m[f"a_lone_2e24{base}"]
        for name in mixes:
            for outs in ("default", "caller", "binding"):
                acc[f"{name}_{outs}_over_lone_2e24"] = m[f"c_{name}_{outs}"] / lone
                acc[f"{name}_{outs}_bar_1.15_met"] = m[f"c_{name}_{outs}"] / lone <= 1.15
            acc[f"{name}_loop_over_many"] = m[f"b_{name}_loop{base}"] / m[f"c_{name}_default"]
        acc["ragged_over_aligned_default"] = m["c_ragged_default"] / m["c_aligned_default"]
        acc["ragged_over_aligned_caller"] = m["c_ragged_caller"] / m["c_aligned_caller"]
        if args.parent_lib:
            a0, a1 = rows["a_lone_2e24_parent"], rows["a_lone_2e24"]
            acc["lone_2e24_new_over_parent"] = a1["median_ms"] / a0["median_ms"]
            acc["lone_2e24_within_parent_spread"] = (a0["min_ms"] <= a1["median_ms"] <= a0["max_ms"])
        res["acceptance"] = acc
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
