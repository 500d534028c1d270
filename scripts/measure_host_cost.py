#!/usr/bin/env python3
"""Host cost per call of the record, frame and share-vector calls in their
non-synchronising forms: LOOPS calls queued back to back at a small n (the
host is the bottleneck, the device runs behind), wall clock per call, then one
synchronise; the median of REPS such passes per call.

For comparing two revisions of the Python layer on one library file: run it
once per tree, one process each, alternating — `--tree DIR` names a checkout
(or an archive of a commit) that holds delta-node_amd/delta_node, and
DN_SHAMIR_LIB points both at the same built library.  Writes
profiles/r15/host_cost.json and prints the rows."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--tree", default=ROOT, help="the tree whose delta-node_amd/delta_node is measured")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "host_cost.json"))
args = ap.parse_args()
pkg, out = os.path.abspath(args.tree), args.out
sys.path.insert(0, os.path.join(pkg, "delta-node_amd"))
import torch  # noqa: E402

import delta_node  # noqa: E402

assert delta_node.__file__.startswith(pkg), delta_node.__file__
from delta_node.crypto import shamir  # noqa: E402
from delta_node.crypto.shamir import codec  # noqa: E402

dev = torch.device("cuda", 0)
n, LOOPS, REPS = 4096, 300, 15
ss = shamir.SecretShare(3)
ss.random.seed(7)
blk = ss.make_shares_vec(torch.arange(n, dtype=torch.int64, device=dev), 5)
wires = [codec.encode_share_vec(blk[x - 1], n, x) for x in (1, 2, 3)]
frames = [codec.encode_share_frame(blk[x - 1], n, x)[0] for x in (1, 2, 3)]
same = [codec.encode_share_vec(blk[0], n, 1) for _ in range(3)]
bad = torch.zeros(2, dtype=torch.int32, device=dev)
cap = codec.frame_capacity(n, 3)
fbuf = torch.empty(cap + 64, dtype=torch.uint8, device=dev)
fbuf = fbuf[(-fbuf.data_ptr()) % 16:][:cap]
wbuf = torch.empty(codec.encoded_capacity(n, 3), dtype=torch.uint8, device=dev)
offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
offs3 = [torch.empty(n + 1, dtype=torch.int64, device=dev) for _ in range(3)]
acc = torch.zeros_like(blk[0])
CALLS = {
    "encode_share_vec": lambda: codec.encode_share_vec(blk[2], n, 3, trim=False, out=wbuf, offsets=offs),
    "encode_share_frame": lambda: codec.encode_share_frame(blk[2], n, 3, trim=False, out=fbuf, offsets=offs),
    "open_frames_m3": lambda: codec.open_frames(frames, n, [1, 2, 3], offsets=offs3, bad=bad),
    "resolve_records_vec": lambda: ss.resolve_records_vec(wires, [1, 2, 3], n, bad=bad),
    "sum_records_vec": lambda: ss.sum_records_vec(same, 1, n, out=acc, bad=bad),
    "sum_shares_vec": lambda: ss.sum_shares_vec([blk[0], blk[1], blk[2]], signs=[1, -1, 1], out=acc),
    "resolve_shares_vec": lambda: ss.resolve_shares_vec([blk[0], blk[1], blk[2]], [1, 2, 3], n),
}
res = {}
for name, f in CALLS.items():
    for _ in range(50):
        f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        for _ in range(LOOPS):
            f()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        ts.append((t1 - t0) / LOOPS * 1e6)
    res[name] = {"median_us": statistics.median(ts), "min_us": min(ts), "max_us": max(ts)}
    print(f"{name:22s} {res[name]['median_us']:.2f} us (min {min(ts):.2f})", flush=True)
json.dump({"tree": pkg, "n": n, "loops": LOOPS, "reps": REPS, "rows": res}, open(out, "w"), indent=1)
