"""check_shares_vec (MI355X): the count and every culprit byte against the
definition in Python integers, on the rows of share_check_cases.py (a damaged
one at element 0, at both sides of every wave and tile edge and at the last
element); the last tile's padding lanes hold junk that would be counted if it
were read.  Integer arithmetic: every comparison is exact.
"""
import random

import numpy as np
import pytest
import torch

import share_check_cases as cases
from delta_node.crypto import shamir
from delta_node.crypto.shamir import _native, field

pytestmark = pytest.mark.gpu

GUARD = 64


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
@pytest.mark.parametrize("t, xs", cases.CASES)
def test_count_and_culprits_match_the_definition(t, xs, n):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = cases.rows(t, xs)
    verdicts = [cases.verdict(xs, ys, t) for ys in rows]
    want = [verdicts[e % len(rows)] for e in range(n)]
    junk = random.Random(n)  # the padding lanes of the last tile
    block = [rows[e % len(rows)] for e in range(n)] + [[junk.randrange(cases.P) for _ in xs]
                                                       for _ in range(-n % field.TILE)]
    vecs = [torch.from_numpy(field.ints_to_vec([ys[i] for ys in block])).to(dev) for i in range(len(xs))]
    n_bad = sum(w != cases.CONSISTENT for w in want)
    n_found = sum(w < cases.UNEXPLAINED for w in want)
    ss = shamir.SecretShare(t)

    # the method: the read-back forms
    assert ss.check_shares_vec(vecs, xs, n) == n_bad
    count, marks = ss.check_shares_vec(torch.stack(vecs), xs, n, culprit=True)
    assert count == n_bad
    assert marks.dtype == torch.uint8 and marks.cpu().tolist() == want

    # the entry point: counts are added to across two calls, the bytes around culprit stay untouched
    plan = _native.check_plan(xs, t)
    counts = torch.tensor([5, 7], dtype=torch.int32, device=dev)
    buf = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    for _ in range(2):
        _native.check_shares(vecs, plan, counts, buf[GUARD:GUARD + n], n)
    assert counts.cpu().tolist() == [5 + 2 * n_bad, 7 + 2 * n_found]
    host = buf.cpu().numpy()
    assert np.all(host[:GUARD] == 0xA5) and np.all(host[GUARD + n:] == 0xA5)
    assert host[GUARD:GUARD + n].tolist() == want

    # the deferred form under one capture, replayed: no synchronisation, counts added on the device
    bad = torch.zeros(2, dtype=torch.int32, device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        none, g_marks = ss.check_shares_vec(vecs, xs, n, culprit=True, bad=bad)
    assert none is None
    for replay in (1, 2, 3):
        g_marks.fill_(0)
        graph.replay()
        assert bad.cpu().tolist() == [replay * n_bad, replay * n_found]
        assert g_marks.cpu().tolist() == want
