"""The robust reconstruct's reference and rows (host and GPU tests): the
DEFINITION in Python integers on share_check_cases' rows — the interpolant of
the shares without the located one, else of all k."""
import share_check_cases as cases

P = cases.P
# the r >= 2 sets of share_check_cases, then odd divisors up to 59535 and k = 16
CASES = [c for c in cases.CASES if len(c[1]) - c[0] >= 2]
MORE = [(3, (2, 5, 11, 13, 16)), (12, tuple(range(1, 17)))]


def want(t, xs, ys):
    """(culprit byte, value) the definition gives one element's shares."""
    v = cases.verdict(xs, ys, t)
    pts = [(x, y) for i, (x, y) in enumerate(zip(xs, ys)) if i != v]
    return v, cases.interpolate(pts, 0)


def rows(t, xs):
    """share_check_cases' nine rows, then secrets 0 and p - 1 under a located error."""
    k, out = len(xs), cases.rows(t, xs)
    for secret, i, delta in ((0, 0, 5), (P - 1, k - 1, P - 7)):
        f = [secret] + [(i + 2) * (j + 3) for j in range(t - 1)]  # a polynomial with f(0) = secret
        ys = [sum(c * x ** j for j, c in enumerate(f)) % P for x in xs]
        ys[i] = (ys[i] + delta) % P
        out.append(ys)
    return out
