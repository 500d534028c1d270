"""The tile walk that check_shares_vec and resolve_shares_vec_robust share (csrc/share_rows.hpp rows_walk), made
to stride (MI355X).  A launch has one workgroup per tile up to 16384 tiles, so no other case of the suite takes the
walk's second step.  Here a fresh child process loads the tuning library with DN_GRID_CAP=2 and n = 1025: five
tiles, one live lane in the last, workgroup 0 walking tiles 0, 2, 4.  One odd and one even k per kernel (both tails
of the row loop); one share altered at each of elements 0, 300 and 1024; counts, culprit bytes and values against
the definition in Python integers (share_check_cases.py, share_robust_cases.py).  All exact."""
import os
import random
import subprocess
import sys

import pytest

N = 1025
ALTERED = {0: 0, 300: -1, 1024: 1}  # element: the share moved
CHECK = [(1, 2), (2, 3), (3, 5)]  # (threshold, k)
ROBUST = [(2, 4), (3, 5)]


def child():
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.join(os.path.dirname(here), "delta-node_amd"), here]
    import torch

    import share_check_cases as cases
    import share_robust_cases as robust
    from delta_node.crypto import shamir
    from delta_node.crypto.shamir import _native, field

    P = cases.P
    dev = torch.device("cuda", torch.cuda.current_device())

    def block(t, k):
        rng, xs = random.Random(100 * t + k), tuple(range(1, k + 1))
        out = []
        for e in range(N):
            f = [rng.randrange(P) for _ in range(t)]
            ys = [sum(c * x ** j for j, c in enumerate(f)) % P for x in xs]
            if e in ALTERED:
                ys[ALTERED[e]] = (ys[ALTERED[e]] + 1 + rng.randrange(P - 1)) % P
            out.append(ys)
        return xs, out

    def device_rows(rows, k):
        pad = rows + [[0] * k] * (-N % field.TILE)
        return [torch.from_numpy(field.ints_to_vec([ys[i] for ys in pad])).to(dev) for i in range(k)]

    with _native.library(_native.TUNING_LIB):
        for t, k in CHECK:
            xs, rows = block(t, k)
            marks = [cases.verdict(xs, ys, t) for ys in rows]
            assert [e for e, m in enumerate(marks) if m != cases.CONSISTENT] == sorted(ALTERED), (t, k)
            count, got = shamir.SecretShare(t).check_shares_vec(device_rows(rows, k), xs, N, culprit=True)
            assert count == len(ALTERED) and got.cpu().tolist() == marks, (t, k)
        for t, k in ROBUST:
            xs, rows = block(t, k)
            ref = [robust.want(t, xs, ys) for ys in rows]
            marks = [m for m, _ in ref]
            counts = (sum(m != cases.CONSISTENT for m in marks), sum(m < cases.UNEXPLAINED for m in marks))
            assert counts[0] == len(ALTERED), (t, k)
            vecs = device_rows(rows, k)
            for out in ("field", "int64"):
                res, count, got = shamir.SecretShare(t).resolve_shares_vec_robust(vecs, xs, N, out=out, culprit=True)
                assert count == counts and got.cpu().tolist() == marks, (t, k, out)
                if out == "field":
                    assert field.vec_to_ints(res.cpu().numpy(), N) == [v for _, v in ref], (t, k, out)
                else:
                    assert [v % (1 << 64) for v in res.cpu().tolist()] == [v % (1 << 64) for _, v in ref], (t, k, out)
    print("ok")


@pytest.mark.gpu
def test_two_workgroups_walk_five_tiles():
    env = dict(os.environ, DN_GRID_CAP="2")
    run = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr


if __name__ == "__main__":
    child()
