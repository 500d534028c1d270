#!/usr/bin/env python3
"""encode_shares_many against the per-(tensor, row) encode_share_vec loop,
3-of-5, all 5 rows, over the model-like mix of scripts/measure_many.py
(mix_sizes: 127 tensors totalling 2^24 elements, aligned and +-1 ragged).

The inputs are what the split leaves: make_shares_vec_many's per-tensor blocks
of each mix, and one make_shares_vec block of the same 2^24 secrets.  Before
timing, every variant's wires are compared on the device with the loop's
(concatenated, offsets rebased) and the lone calls' with the aligned mix's (the
same elements in the same order); a mismatch ends the run.  Rows, each timed
with device events around one pass that ends in a synchronise, REPS passes
after a warm-up, the variants alternating within this one process:
  a  the per-(tensor, row) encode_share_vec loop over each mix into caller
     buffers, trim=False (635 calls, no read-back: the loop's best form)
  b  encode_shares_many over each mix, caller buffers, trim=False
  b' encode_shares_many over each mix, default buffers, trim=True
  c  five lone encode_share_vec calls on one 2^24 vector (caller buffers,
     trim=False)
The bandwidth-bound rows (b, b', c of both libraries) alternate among
themselves first, then the loops (a): a pass of b that follows 11 ms of the
loop's small kernels runs up to 10 % slower than one that follows another
large pass, which says nothing about b.  With --parent-lib PATH (a build of the parent commit's library)
rows a and c are also taken on that library — the baseline is then not the
code under test.  Writes profiles/r11/encode_many.json and prints it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from measure_many import N_TOTAL, REPS, mix_sizes  # noqa: E402

XS = [1, 2, 3, 4, 5]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libdn_shamir.so built from the parent commit (rows a and c on it too)")
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "encode_many.json"))
    ap.add_argument("--only", help="run one variant REPS times and exit (for a kernel trace), e.g. b_ragged_caller")
    args = ap.parse_args()
    assert args.reps >= 20 or args.only, "at least 20 repetitions"

    sys.path.insert(0, os.path.join(ROOT, "delta-node_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch

    from delta_node.crypto import shamir
    from delta_node.crypto.shamir import _native, codec
    from golden.fixtures import secrets_int64

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    sec = torch.from_numpy(secrets_int64(5, N_TOTAL)).to(dev)
    mixes = {"aligned": mix_sizes(False), "ragged": mix_sizes(True)}
    ss = shamir.SecretShare(3)
    # the blocks kept as allocations of their own (the split's pooled block is reused by the next split)
    blocks = {}
    for name, sizes in mixes.items():
        ss.random.seed(9)
        blocks[name] = [b.clone() for b in ss.make_shares_vec_many(list(torch.split(sec, sizes)), 5)]
    ss.random.seed(9)  # the same draws: the lone vector's rows hold the mixes' elements in the same order
    big = ss.make_shares_vec(sec, 5).clone()
    del sec
    caps = [codec.encoded_capacity(N_TOTAL, x) for x in XS]

    def buffers():
        # (slack: the loop's pieces each start on a 16-byte boundary)
        return ([torch.empty(c + 4096, dtype=torch.uint8, device=dev) for c in caps],
                [torch.empty(N_TOTAL + 1, dtype=torch.int64, device=dev) for _ in XS])

    outs, offs = buffers()  # every timed variant writes here
    res = {"lib": os.path.basename(_native.lib_path()), "parent_lib": args.parent_lib, "reps": args.reps,
           "n_total": N_TOTAL, "tensors": 127, "xs": XS, "threshold": 3}

    def loop(name):
        """encode_share_vec per (tensor, row) into 16-byte aligned pieces of the
        wire buffers (the wide store path for every tensor); the offsets are
        each tensor's own (not rebased, no read-back: nothing but the 635
        calls is timed)."""
        for i, x in enumerate(XS):
            pos = e = 0
            for b, n in zip(blocks[name], mixes[name]):
                cap = codec.encoded_capacity(n, x)
                codec.encode_share_vec(b[i], n, x, trim=False, out=outs[i][pos:pos + cap],
                                       offsets=offs[i][e:e + n + 1])
                pos = (pos + cap + 15) & ~15
                e += n

    def many_caller(name):
        return codec.encode_shares_many(blocks[name], mixes[name], trim=False, outs=outs, offsets=offs)

    def many_default(name):
        return codec.encode_shares_many(blocks[name], mixes[name])

    def lone():
        return [codec.encode_share_vec(big[i], N_TOTAL, x, trim=False, out=outs[i], offsets=offs[i])
                for i, x in enumerate(XS)]

    def reference(name):
        """The loop's wires, concatenated with rebased offsets, on the device: (packed, offsets) per x."""
        want = []
        for i, x in enumerate(XS):
            parts, fo, base = [], [], 0
            for b, n in zip(blocks[name], mixes[name]):
                p, f = codec.encode_share_vec(b[i], n, x)
                parts.append(p)
                fo.append(f[:n] + base)
                base += p.numel()
            fo.append(torch.tensor([base], dtype=torch.int64, device=dev))
            want.append((torch.cat(parts), torch.cat(fo)))
        return want

    def same(got, want, what):
        for i, ((gp, go), (wp, wo)) in enumerate(zip(got, want)):
            total = int(wo[-1])
            if not (torch.equal(go[: N_TOTAL + 1], wo) and torch.equal(gp[:total], wp)):
                sys.exit(f"measure_encode_many: {what}: wire {i} differs from the loop's")

    # correctness first, on this library
    for name in mixes:
        want = reference(name)
        same(many_caller(name), want, f"b_{name}_caller")
        same(many_default(name), want, f"b_{name}_default")
        if name == "aligned":
            same(lone(), want, "c_lone")
            if args.parent_lib:
                with _native.library(args.parent_lib):
                    same(lone(), want, "c_lone_parent")
        del want
    res["outputs_equal_loop"] = True

    def variants(tag, lib_path):
        v = {f"c_lone_5x2e24{tag}": (lone, lib_path)}
        for name in mixes:
            v[f"a_{name}_loop{tag}"] = (lambda name=name: loop(name), lib_path)
            if lib_path is None:
                v[f"b_{name}_caller"] = (lambda name=name: many_caller(name), None)
                v[f"b_{name}_default"] = (lambda name=name: many_default(name), None)
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

    times = {k: [] for k in todo}
    for k, (fn, lib_path) in todo.items():  # warm-up
        one_pass(fn, lib_path)
        one_pass(fn, lib_path)
    for phase in ([k for k in todo if not k.startswith("a_")], [k for k in todo if k.startswith("a_")]):
        for _ in range(args.reps):
            for k in phase:
                times[k].append(one_pass(*todo[k]))
    rows = {}
    for k, ts in times.items():
        rows[k] = {"mean_ms": statistics.fmean(ts), "median_ms": statistics.median(ts), "min_ms": min(ts),
                   "max_ms": max(ts), "stdev_ms": statistics.stdev(ts) if len(ts) > 1 else 0.0}
    res["rows"] = rows
    if not args.only:
        base = "_parent" if args.parent_lib else ""
        acc = {"baseline": "parent library" if args.parent_lib else "this library (no --parent-lib)"}
        lone_med = rows[f"c_lone_5x2e24{base}"]["median_ms"]
        for name in mixes:
            a, b, bd = rows[f"a_{name}_loop{base}"], rows[f"b_{name}_caller"], rows[f"b_{name}_default"]
            acc[f"{name}_many_slowest_below_loop_fastest"] = b["max_ms"] < a["min_ms"]
            acc[f"{name}_loop_over_many"] = a["median_ms"] / b["median_ms"]
            acc[f"{name}_loop_over_many_default"] = a["median_ms"] / bd["median_ms"]
            acc[f"{name}_many_over_lone"] = b["median_ms"] / lone_med
            acc[f"{name}_bar_1.15_met"] = b["median_ms"] / lone_med <= 1.15
        if args.parent_lib:
            c0, c1 = rows["c_lone_5x2e24_parent"], rows["c_lone_5x2e24"]
            acc["lone_new_over_parent"] = c1["median_ms"] / c0["median_ms"]
            acc["lone_within_parent_spread"] = c0["min_ms"] <= c1["median_ms"] <= c0["max_ms"]
        res["acceptance"] = acc
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
