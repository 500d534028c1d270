#!/usr/bin/env python3
"""make_shares_vec_many against the per-tensor make_shares_vec loop, 3-of-5,
over a model-like mix of 127 tensors totalling 2^24 elements.

The mix (mix_sizes): 2 x 2^22, 4 x 2^20, 9 x 2^18, 16 x 2^16, 32 x 2^14,
64 x 2^12 in a fixed seeded order (aligned), and the same list with sizes
alternately +1 / -1, the last tensor absorbing the remainder (ragged).

Before timing, both mixes' assembled outputs are checked against the
reference's own 2^24 digest (tests/golden, split_t3n5_2e24); a mismatch ends
the run.  Rows, each timed with device events around one pass that ends in a
synchronise, REPS passes after a warm-up, the variants alternating within
this one process (rows a among themselves, then rows b and c):
  a  make_shares_vec(2^24): a lone call, and a loop of 4 (per call)
  b  the per-tensor make_shares_vec loop over each mix (today's caller), into
     caller-given blocks and into the default pooled ones
  c  make_shares_vec_many over each mix: pooled outs, caller outs, and pooled
     outs from separately allocated inputs (one torch.cat of the secrets)
With --parent-lib PATH (a build of the parent commit's library) rows a and b
are also taken on that library — the baseline is then not the code under
test.  Writes profiles/r07/many.json and prints it."""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_TOTAL = 1 << 24
REPS = 20


def mix_sizes(ragged: bool):
    sizes = [1 << 22] * 2 + [1 << 20] * 4 + [1 << 18] * 9 + [1 << 16] * 16 + [1 << 14] * 32 + [1 << 12] * 64
    random.Random(2024).shuffle(sizes)
    if ragged:
        sizes = [n + (1 if k % 2 == 0 else -1) for k, n in enumerate(sizes)]
        sizes[-1] = N_TOTAL - sum(sizes[:-1])
    assert sum(sizes) == N_TOTAL and len(sizes) == 127
    return sizes


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libdn_shamir.so built from the parent commit (rows a and b on it too)")
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "many.json"))
    ap.add_argument("--only", help="run one variant REPS times and exit (for a kernel trace), e.g. c_ragged_pooled")
    args = ap.parse_args()
    assert args.reps >= 20 or args.only, "at least 20 repetitions"

    sys.path.insert(0, os.path.join(ROOT, "delta-node_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch

    from delta_node.crypto import shamir
    from delta_node.crypto.shamir import _native, field, memory
    from golden.fixtures import chunk_digests, combine_digests, manifest, secrets_int64

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    d = [d for d in manifest()["digests"] if d["name"] == "split_t3n5_2e24"][0]
    assert d["N"] == N_TOTAL and d["t"] == 3 and d["n"] == 5
    sec = torch.from_numpy(secrets_int64(d["secret_seed"], N_TOTAL)).to(dev)
    mixes = {"aligned": mix_sizes(False), "ragged": mix_sizes(True)}
    tensors = {k: list(torch.split(sec, v)) for k, v in mixes.items()}  # views of one buffer: no concatenation
    separate = {k: [x.clone() for x in v] for k, v in tensors.items()}   # separate allocations: one torch.cat per call
    res = {"lib": os.path.basename(_native.lib_path()), "parent_lib": args.parent_lib, "reps": args.reps,
           "n_total": N_TOTAL, "tensors": 127, "t": 3, "n": 5}

    if not args.only:
        for name, sizes in mixes.items():  # correctness first: the reference's own digest
            ss = shamir.SecretShare(3)
            ss.random.seed(d["mt_seed"])
            outs = ss.make_shares_vec_many(tensors[name], 5)
            planes = np.empty((5, 17, N_TOTAL), dtype=np.uint32)
            off = 0
            for out, n in zip(outs, sizes):
                h = out.cpu().numpy()
                for s in range(5):
                    planes[s, :, off:off + n] = field.vec_to_planes(h[s], n)
                off += n
            ok = combine_digests(chunk_digests(planes)) == d["digest"]
            res[f"digest_ok_{name}"] = ok
            del planes, outs
            if not ok:
                print(json.dumps(res))
                sys.exit(f"measure_many: the {name} mix does not reproduce the reference digest")

    def instance():
        ss = shamir.SecretShare(3)
        ss.random.seed(9)
        return ss

    caller_outs = {}
    for name, sizes in mixes.items():
        blk = memory.share_block((5 * sum(field.vec_bytes(n) for n in sizes),), dev)
        outs, off = [], 0
        for n in sizes:
            vb = field.vec_bytes(n)
            outs.append(blk[off:off + 5 * vb].view(5, vb))
            off += 5 * vb
        caller_outs[name] = outs

    big = memory.share_block((5, field.vec_bytes(N_TOTAL)), dev)

    def variants(tag, lib_path):
        """name -> (callable of one pass, calls per pass, library path or None)"""
        v = {}
        # rows a and b write caller-given blocks on both libraries: the block
        # pool lives in the library, so a second library cannot take blocks
        # from it (b_*_loop_pooled, this library only: the default outs)
        lone, loop = instance(), instance()
        v[f"a_lone_2e24{tag}"] = (lambda: lone.make_shares_vec(sec, 5, out=big), 1, lib_path)
        v[f"a_loop4_2e24{tag}"] = (lambda: [loop.make_shares_vec(sec, 5, out=big) for _ in range(4)], 4, lib_path)
        for name in mixes:
            ss = instance()
            v[f"b_{name}_loop{tag}"] = (lambda ss=ss, name=name: [ss.make_shares_vec(x, 5, out=o) for x, o in
                                                                  zip(tensors[name], caller_outs[name])], 1, lib_path)
        if lib_path is None:
            for name in mixes:
                d0 = instance()
                v[f"b_{name}_loop_pooled"] = (lambda d0=d0, name=name: [d0.make_shares_vec(x, 5)
                                                                        for x in tensors[name]], 1, None)
                p, c = instance(), instance()
                v[f"c_{name}_pooled"] = (lambda p=p, name=name: p.make_shares_vec_many(tensors[name], 5), 1, None)
                q = instance()
                v[f"c_{name}_separate"] = (lambda q=q, name=name: q.make_shares_vec_many(separate[name], 5), 1, None)
                v[f"c_{name}_caller"] = (lambda c=c, name=name: c.make_shares_vec_many(tensors[name], 5,
                                                                                      outs=caller_outs[name]), 1, None)
        return v

    todo = variants("", None)
    if args.parent_lib:
        todo.update(variants("_parent", args.parent_lib))
    if args.only:
        todo = {args.only: todo[args.only]}

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

    # two phases, the variants of a phase alternating: the 2^24 single-vector
    # rows of both libraries among themselves (a draw keeps host-side tables
    # of its last shape only, so a 2^24 call that follows another shape pays
    # for them again: that is part of rows b, not of a lone call), then the mixes
    times = {k: [] for k in todo}
    for phase in ([k for k in todo if k.startswith("a_")], [k for k in todo if not k.startswith("a_")]):
        for k in phase:  # warm-up: allocations, job tables, pools
            for _ in range(2):
                one_pass(todo[k][0], todo[k][2])
        for _ in range(args.reps):
            for k in phase:
                fn, calls, lib_path = todo[k]
                times[k].append(one_pass(fn, lib_path) / calls)
    rows = {}
    for k, ts in times.items():
        rows[k] = {"mean_ms": statistics.fmean(ts), "median_ms": statistics.median(ts), "min_ms": min(ts),
                   "max_ms": max(ts), "stdev_ms": statistics.stdev(ts) if len(ts) > 1 else 0.0}
    res["rows"] = rows
    if not args.only:
        m = {k: r["median_ms"] for k, r in rows.items()}
        acc = {"ragged_over_aligned_pooled": m["c_ragged_pooled"] / m["c_aligned_pooled"]}
        base = "_parent" if args.parent_lib else ""
        acc["baseline"] = "parent library" if args.parent_lib else "this library (no --parent-lib)"
        acc["aligned_pooled_over_lone_2e24"] = m["c_aligned_pooled"] / m[f"a_lone_2e24{base}"]
        acc["aligned_bar_1.15_met"] = acc["aligned_pooled_over_lone_2e24"] <= 1.15
        for name in mixes:
            b = rows[f"b_{name}_loop{base}"]
            acc[f"{name}_loop_over_many"] = b["median_ms"] / m[f"c_{name}_pooled"]
            acc[f"{name}_many_below_loop_by_more_than_its_spread"] = (
                rows[f"c_{name}_pooled"]["max_ms"] < b["min_ms"] - (b["max_ms"] - b["min_ms"]))
        if args.parent_lib:
            a0, a1 = rows["a_lone_2e24_parent"], rows["a_lone_2e24"]
            acc["lone_2e24_new_over_parent"] = a1["median_ms"] / a0["median_ms"]
            acc["lone_2e24_within_spread"] = abs(a1["median_ms"] - a0["median_ms"]) <= max(
                a0["max_ms"] - a0["min_ms"], a1["max_ms"] - a1["min_ms"])
        res["acceptance"] = acc
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
