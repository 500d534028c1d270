"""resolve_shares_vec_robust (MI355X): every value, both counts and every culprit byte against the
definition in Python integers (share_robust_cases.py); junk in the last tile's padding lanes.  All exact."""
import functools
import random

import numpy as np
import pytest
import torch

import share_robust_cases as robust
from delta_node.crypto import shamir
from delta_node.crypto.shamir import _native, field

pytestmark = pytest.mark.gpu

GUARD, P = 64, robust.P
SIZES = [1, 63, 64, 65, 255, 256, 257, 513]


@functools.lru_cache(maxsize=None)
def reference(t, xs):
    rows = robust.rows(t, xs)
    return rows, [robust.want(t, xs, ys) for ys in rows]


def device_rows(block, k, dev):
    return [torch.from_numpy(field.ints_to_vec([ys[i] for ys in block])).to(dev) for i in range(k)]


def values(res, out, n):
    return field.vec_to_ints(res.cpu().numpy(), n) if out == "field" else [v % (1 << 64) for v in res.cpu().tolist()]


@pytest.mark.parametrize("out", ["field", "int64"])
@pytest.mark.parametrize("t, xs, n", [(t, xs, n) for t, xs in robust.CASES for n in SIZES]
                         + [(t, xs, 65) for t, xs in robust.MORE])
def test_values_counts_and_culprits_match_the_definition(t, xs, n, out):
    dev = torch.device("cuda", torch.cuda.current_device())
    rows, ref = reference(t, xs)
    junk = random.Random(n)  # the padding lanes of the last tile
    block = [rows[e % len(rows)] for e in range(n)] + [[junk.randrange(P) for _ in xs] for _ in range(-n % field.TILE)]
    vecs = device_rows(block, len(xs), dev)
    marks = [ref[e % len(rows)][0] for e in range(n)]
    want = [ref[e % len(rows)][1] % (P if out == "field" else 1 << 64) for e in range(n)]
    n_bad, n_found = sum(m != 0xFF for m in marks), sum(m < 0xFE for m in marks)
    ss = shamir.SecretShare(t)

    # the method, read-back form
    res, count, got_marks = ss.resolve_shares_vec_robust(torch.stack(vecs), xs, n, out=out, culprit=True)
    assert count == (n_bad, n_found) and got_marks.cpu().tolist() == marks
    got = values(res, out, n)
    assert got == want
    if out == "field":  # where nothing is located: resolve_shares_vec over all k rows, bit for bit
        full = values(ss.resolve_shares_vec(vecs, xs, n, out="field"), out, n)
        assert [(g, m) for g, m in zip(got, marks) if m >= 0xFE] == [(f, m) for f, m in zip(full, marks) if m >= 0xFE]

    # the entry point: counts are added to across two calls, canaries around the culprit bytes and the int64 words
    plan = _native.robust_plan(xs, t)
    counts = torch.tensor([5, 7], dtype=torch.int32, device=dev)
    buf = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    words = torch.full((GUARD + n + GUARD,), -3, dtype=torch.int64, device=dev)
    fe = torch.empty(field.vec_bytes(n), dtype=torch.uint8, device=dev)
    for _ in range(2):
        _native.reconstruct_robust(vecs, plan, counts, fe if out == "field" else None,
                                   words[GUARD:GUARD + n] if out == "int64" else None, buf[GUARD:GUARD + n], n)
    assert counts.cpu().tolist() == [5 + 2 * n_bad, 7 + 2 * n_found]
    host = buf.cpu().numpy()
    assert np.all(host[:GUARD] == 0xA5) and np.all(host[GUARD + n:] == 0xA5) and host[GUARD:GUARD + n].tolist() == marks
    assert torch.all(words[:GUARD] == -3) and torch.all(words[GUARD + n:] == -3)
    assert values(fe if out == "field" else words[GUARD:GUARD + n], out, n) == want


@pytest.mark.parametrize("wire", [2, 0, 4])
def test_a_whole_bad_wire_is_corrected(wire):
    dev = torch.device("cuda", torch.cuda.current_device())
    t, xs, n, rng = 3, (1, 2, 3, 4, 5), 257, random.Random(wire)
    polys = [[rng.randrange(P) for _ in range(t)] for _ in range(n)]
    block = [[sum(c * x ** j for j, c in enumerate(f)) % P for x in xs] for f in polys]
    for ys in block:
        ys[wire] = (ys[wire] + 1 + rng.randrange(P - 1)) % P  # a random field element that is not the share
    res, count, marks = shamir.SecretShare(t).resolve_shares_vec_robust(device_rows(block, 5, dev), xs, n, out="field",
                                                                        culprit=True)
    assert count == (n, n) and marks.cpu().tolist() == [wire] * n
    assert values(res, "field", n) == [f[0] for f in polys]


def test_the_deferred_form_under_one_capture():
    dev = torch.device("cuda", torch.cuda.current_device())
    t, xs, n = 3, (1, 3, 4, 7, 9), 257
    rows, ref = reference(t, xs)
    vecs = device_rows([rows[e % len(rows)] for e in range(n)] + [[0] * 5] * (-n % field.TILE), 5, dev)
    ss = shamir.SecretShare(t)
    eager, count, eager_marks = ss.resolve_shares_vec_robust(vecs, xs, n, out="field", culprit=True)
    assert values(eager, "field", n) == [ref[e % len(rows)][1] for e in range(n)]
    bad = torch.zeros(2, dtype=torch.int32, device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res, none, marks = ss.resolve_shares_vec_robust(vecs, xs, n, out="field", culprit=True, bad=bad)
    assert none is None
    for replay in (1, 2, 3):
        res.fill_(0)
        marks.fill_(0)
        graph.replay()
        assert bad.cpu().tolist() == [replay * count[0], replay * count[1]]
        assert values(res, "field", n) == values(eager, "field", n) and torch.equal(marks, eager_marks)
