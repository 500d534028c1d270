#!/usr/bin/env python3
"""resolve_records_vec against the route it replaces — decode_share_vec on
every wire, then resolve_shares_vec — on records of the fused split's shares.

Configurations: 3-of-5 with xs {1, 3, 5} and 5-of-9 with xs {1, 3, 5, 7, 9},
each at 2^24 and 2^20 elements, int64 out.  The wires are what a receiver
holds: codec.encode_share_vec of the rows of make_shares_vec.  Before timing,
every row's output is compared with the secrets on the device and the
deferred flags are checked; a mismatch ends the run.  Rows, each timed with
device events around one pass that ends in a synchronise, REPS passes after a
warm-up, the rows of a configuration alternating within this one process:
  a  the parent route as a careful caller runs it: k decode_share_vec into
     caller buffers with a deferred `bad` flag, then resolve_shares_vec
  b  resolve_records_vec with a deferred `bad`
  c  _native.reconstruct_records alone (descriptors and output made beforehand)
  d  a lone resolve_shares_vec on ready vectors, for scale
  e  a lone decode_share_vec of wire 0 into caller buffers
With --parent-lib PATH (a build of the parent commit's library) rows a, d and
e are also taken on that library: the baseline is then not the code under
test, and d / e show whether the untouched kernels still run as they did.
--variant NAME=PATH[:ENV=VALUE[,ENV=VALUE]] adds row c on another build of
this library (a kernel variant, or the tuning build with its knobs set).
Writes profiles/r10/resolve_records.json and prints it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 20
HBM_BYTES_PER_S = 8.0e12
CONFIGS = [("3of5_2e24", 3, 5, [1, 3, 5], 1 << 24), ("3of5_2e20", 3, 5, [1, 3, 5], 1 << 20),
           ("5of9_2e24", 5, 9, [1, 3, 5, 7, 9], 1 << 24), ("5of9_2e20", 5, 9, [1, 3, 5, 7, 9], 1 << 20)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libdn_shamir.so built from the parent commit (rows a, d, e on it too)")
    ap.add_argument("--variant", action="append", default=[],
                    help="NAME=PATH[:ENV=VALUE[,ENV=VALUE]]: row c on that build too")
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--configs", help="comma-separated subset of " + ",".join(c[0] for c in CONFIGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "resolve_records.json"))
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
    variants = []
    for spec in args.variant:
        name, rest = spec.split("=", 1)
        path, _, env = rest.partition(":")
        variants.append((name, path, [tuple(kv.split("=", 1)) for kv in env.split(",")] if env else None))
    res = {"lib": os.path.basename(_native.lib_path()),
           "parent_lib": os.path.basename(args.parent_lib) if args.parent_lib else None, "reps": args.reps,
           "variants": {n: {"lib": os.path.basename(p), "env": e} for n, p, e in variants}, "out": "int64",
           "hbm_bytes_per_s": HBM_BYTES_PER_S, "configs": {}}
    wanted = args.configs.split(",") if args.configs else [c[0] for c in CONFIGS]

    def one_pass(fn, lib_path, env, want=None, flags=()):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for key, value in env or ():
            os.environ[key] = value
        try:
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
        finally:
            for key, _ in env or ():
                del os.environ[key]
        if want is not None and out is not None and not torch.equal(out, want):
            sys.exit("measure_resolve_records: a row does not reconstruct the secrets")
        for f in flags:
            if int(f.sum().item()):
                sys.exit("measure_resolve_records: a row counted bad records")
        return s.elapsed_time(e)

    for cname, t, nsh, xs, n in CONFIGS:
        if cname not in wanted:
            continue
        k = len(xs)
        sec = torch.from_numpy(secrets_int64(5, n)).to(dev)
        ss = shamir.SecretShare(t)
        ss.random.seed(9)
        block = ss.make_shares_vec(sec, nsh)
        vecs = [block[x - 1].clone() for x in xs]
        del block
        wires = []
        for x, v in zip(xs, vecs):
            p, o = codec.encode_share_vec(v, n, x)
            wires.append((p.clone(), o))  # the trimmed view's own allocation
        wire_bytes = [p.numel() for p, _ in wires]
        # caller buffers of the parent route, the outputs, the deferred flags
        dec_out = [torch.empty(field.vec_bytes(n), dtype=torch.uint8, device=dev) for _ in xs]
        dec_xs = [torch.empty(n, dtype=torch.int64, device=dev) for _ in xs]
        flag1 = torch.zeros(1, dtype=torch.int32, device=dev)
        flag2 = torch.zeros(2, dtype=torch.int32, device=dev)
        out_c = torch.empty(n, dtype=torch.int64, device=dev)
        weights = _native.lagrange(xs, t)
        desc = [(p.data_ptr(), p.numel(), o.data_ptr()) for p, o in wires]

        def row_a():
            got = [codec.decode_share_vec(p, o, n, out=b, xs=x, bad=flag1)[0]
                   for (p, o), b, x in zip(wires, dec_out, dec_xs)]
            return ss.resolve_shares_vec(got, xs, n)

        def row_b():
            return ss.resolve_records_vec(wires, xs, n, bad=flag2)

        def row_c():
            _native.reconstruct_records(desc, xs, weights, flag2, out_u64=out_c, n=n)
            return out_c

        def row_d():
            return ss.resolve_shares_vec(vecs, xs, n)

        def row_e():
            codec.decode_share_vec(wires[0][0], wires[0][1], n, out=dec_out[0], xs=dec_xs[0], bad=flag1)

        todo = {"a_decode_then_resolve": (row_a, None, None), "b_resolve_records": (row_b, None, None),
                "c_binding": (row_c, None, None), "d_lone_resolve": (row_d, None, None),
                "e_lone_decode": (row_e, None, None)}
        if args.parent_lib:
            todo.update({"a_decode_then_resolve_parent": (row_a, args.parent_lib, None),
                         "d_lone_resolve_parent": (row_d, args.parent_lib, None),
                         "e_lone_decode_parent": (row_e, args.parent_lib, None)})
        for name, path, env in variants:
            todo[f"c_binding_{name}"] = (row_c, path, env)
        times = {r: [] for r in todo}
        for r, (fn, path, env) in todo.items():  # warm-up and correctness: every row against the secrets
            one_pass(fn, path, env, want=sec, flags=(flag1, flag2))
            one_pass(fn, path, env)
        for _ in range(args.reps):
            for r, (fn, path, env) in todo.items():
                times[r].append(one_pass(fn, path, env))
        if int(flag1.sum().item()) or int(flag2.sum().item()):
            sys.exit("measure_resolve_records: bad records counted during the timed passes")
        rows = {r: {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts),
                    "mean_ms": statistics.fmean(ts)} for r, ts in times.items()}
        bytes_b = sum(wire_bytes) + 8 * k * (n + 1) + 8 * n
        bytes_dec = wire_bytes[0] + 8 * (n + 1) + 66 * n + 8 * n
        bytes_rec = 66 * k * n + 8 * n

        def frac(nbytes, row):
            return nbytes / (rows[row]["median_ms"] * 1e-3) / HBM_BYTES_PER_S

        base = "a_decode_then_resolve_parent" if args.parent_lib else "a_decode_then_resolve"
        acc = {"baseline": "parent library" if args.parent_lib else "this library (no --parent-lib)",
               "a_over_b_median": rows[base]["median_ms"] / rows["b_resolve_records"]["median_ms"],
               "b_slowest_below_a_fastest": rows["b_resolve_records"]["max_ms"] < rows[base]["min_ms"],
               "b_over_d_median": rows["b_resolve_records"]["median_ms"] / rows["d_lone_resolve"]["median_ms"]}
        if args.parent_lib:
            for r in ("d_lone_resolve", "e_lone_decode"):
                p0 = rows[r + "_parent"]
                acc[f"{r}_new_over_parent"] = rows[r]["median_ms"] / p0["median_ms"]
                acc[f"{r}_within_parent_spread"] = p0["min_ms"] <= rows[r]["median_ms"] <= p0["max_ms"]
        res["configs"][cname] = {
            "threshold": t, "shares": nsh, "xs": xs, "n": n, "wire_bytes": wire_bytes, "outputs_equal_secrets": True,
            "rows": rows,
            "bytes": {"b": bytes_b, "decode_one_wire": bytes_dec, "reconstruct": bytes_rec,
                      "a_route": sum(w + 8 * (n + 1) + 74 * n for w in wire_bytes) + bytes_rec},
            "fraction_of_hbm": {"b_resolve_records": frac(bytes_b, "b_resolve_records"),
                                "c_binding": frac(bytes_b, "c_binding"),
                                "e_lone_decode": frac(bytes_dec, "e_lone_decode"),
                                "d_lone_resolve": frac(bytes_rec, "d_lone_resolve")},
            "acceptance": acc}
        del vecs, wires, dec_out, dec_xs, sec
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
