"""resolve_shares_vec_robust / resolve_records_vec_robust with errors=2 (MI355X): every value, both counts and
every culprit byte against robust2_cases' elements — clean, every single share, EVERY pair, a triple —
whose values are Python Lagrange interpolants.  Integer arithmetic: every comparison is exact."""
import pytest
import torch

import robust2_cases as cases
from delta_node.crypto import shamir
from delta_node.crypto.shamir import codec, field

pytestmark = pytest.mark.gpu

P, N = cases.P, cases.N


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def device_rows(rows, k):
    pad = [[0] * k] * (-len(rows) % field.TILE)
    return [torch.from_numpy(field.ints_to_vec([ys[i] for ys in rows + pad])).to(dev()) for i in range(k)]


def values(res, out, n=N):
    return field.vec_to_ints(res.cpu().numpy(), n) if out == "field" else [v % (1 << 64) for v in res.cpu().tolist()]


def expected(t, xs, out):
    rows, marks, vals = cases.block(t, xs)
    count = (sum(m != 0xFF for m in marks), sum(m < 0xFE for m in marks))
    return rows, marks, [v % (P if out == "field" else 1 << 64) for v in vals], count


@pytest.mark.parametrize("out", ["int64", "field"])
@pytest.mark.parametrize("t, xs", cases.SETS)
def test_shares_values_counts_and_culprits(t, xs, out):
    rows, marks, want, count = expected(t, xs, out)
    vecs, ss = device_rows(rows, len(xs)), shamir.SecretShare(t)
    res, got_count, got_marks = ss.resolve_shares_vec_robust(vecs, xs, N, out=out, culprit=True, errors=2)
    assert (got_marks.cpu().tolist(), got_count) == (marks, count) and values(res, out) == want
    # errors=1 on the same inputs: today's verdicts and values (a pair is unexplained, the all-rows interpolant)
    one, count1, marks1 = ss.resolve_shares_vec_robust(vecs, xs, N, out=out, culprit=True, errors=1)
    assert marks1.cpu().tolist() == [m if m < 16 or m >= 0xFE else 0xFE for m in marks]
    assert count1 == (count[0], sum(m < 16 for m in marks))
    full = [cases.interpolate(xs, ys) % (P if out == "field" else 1 << 64) for ys in rows]
    assert values(one, out) == [w if m < 16 or m == 0xFF else f for w, f, m in zip(want, full, marks)]


@pytest.mark.parametrize("out", ["int64", "field"])
@pytest.mark.parametrize("t, xs", cases.SETS[1:])
def test_records_values_counts_and_culprits(t, xs, out):
    rows, marks, want, count = expected(t, xs, out)
    wires = [codec.encode_share_vec(v, N, x) for v, x in zip(device_rows(rows, len(xs)), xs)]
    res, got_count, got_marks = shamir.SecretShare(t).resolve_records_vec_robust(wires, xs, N, out=out, culprit=True,
                                                                                 errors=2)
    assert (got_marks.cpu().tolist(), got_count) == (marks, count) and values(res, out) == want


@pytest.mark.parametrize("form", ["shares", "records"])
def test_the_deferred_form_under_one_capture_with_no_call_before_it(form):
    t, xs = 3, (2, 3, 5, 6, 8, 9, 12)  # a set no other call of this process has planned
    rows, marks, want, count = expected(t, xs, "field")
    vecs, ss = device_rows(rows, len(xs)), shamir.SecretShare(t)
    bad, rec = (torch.zeros(2, dtype=torch.int32, device=dev()) for _ in range(2))
    wires = [codec.encode_share_vec(v, N, x) for v, x in zip(vecs, xs)] if form == "records" else None
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        if form == "shares":
            res, none, got = ss.resolve_shares_vec_robust(vecs, xs, N, out="field", culprit=True, bad=bad, errors=2)
        else:
            res, none, got = ss.resolve_records_vec_robust(wires, xs, N, out="field", culprit=True, bad=bad,
                                                           bad_records=rec, errors=2)
    assert none is None
    for replay in (1, 2, 3):
        res.fill_(0)
        got.fill_(0)
        graph.replay()
        assert bad.tolist() == [replay * count[0], replay * count[1]] and rec.tolist() == [0, 0]
        assert values(res, "field") == want and got.cpu().tolist() == marks


@pytest.mark.parametrize("damage", ["truncated", "garbled"])
def test_damaged_wires_are_survived(damage):
    """Two whole wires cut short (every record from the cut on is unrepresentable: y = 0), or one wire whose
    records all claim a y of 69 bytes, next to a second wire with wrong shares."""
    t, xs, n = 5, tuple(range(1, 10)), N
    clean = [ys for ys, m in zip(*cases.block(t, xs)[:2]) if m == 0xFF]
    rows = [list(clean[e % len(clean)]) for e in range(n)]
    secrets = [cases.interpolate(xs[:t], ys[:t]) for ys in rows]
    i, j = 2, 7
    for ys in rows:
        ys[j] = (ys[j] + 1) % P
    wires = [list(codec.encode_share_vec(v, n, x)) for v, x in zip(device_rows(rows, 9), xs)]
    if damage == "truncated":
        for w in (i, j):
            cut = int(wires[w][1][40].item())  # elements 40 .. n - 1 of both wires lose their records
            wires[w][0], wires[w][1] = wires[w][0][:cut].clone(), torch.clamp(wires[w][1], max=cut)
        marks = [j] * 40 + [16 + j * (j - 1) // 2 + i] * (n - 40)
    else:
        wires[i] = [torch.tensor([1, xs[i], 1] + [0] * 68, dtype=torch.uint8, device=dev()).repeat(n),
                    torch.arange(n + 1, dtype=torch.int64, device=dev()) * 71]
        marks = [16 + j * (j - 1) // 2 + i] * n
    ss, rec = shamir.SecretShare(t), torch.zeros(2, dtype=torch.int32, device=dev())
    wires = [tuple(w) for w in wires]
    res, count, got = ss.resolve_records_vec_robust(wires, xs, n, out="field", culprit=True, bad_records=rec, errors=2)
    assert (got.cpu().tolist(), count) == (marks, (n, n)) and values(res, "field", n) == secrets
    plain = torch.zeros(2, dtype=torch.int32, device=dev())
    ss.resolve_records_vec(wires, xs, n, out="field", bad=plain)
    assert rec.tolist() == plain.tolist() and rec[0].item() > 0
