"""numpy restatement of dpvo_amd.long_term.match_descriptors (csrc/match.hip).

`match_ref(a, b, ...)` works in `dtype` (float32 as the kernel does, or
float64 for a reference that is exact to ~1e-16): similarity, squared
distances, the best and second-best of every row and column (smaller d2, then
the lower index), mutual agreement, the ratio test against r2 = float32(ratio^2)
and the distance cap float32(max_dist^2).  With inputs whose products and
sums are exact in fp32 (entries in {-1, 0, 1} / 8) the float32 result does not
depend on the order of any sum, so the kernel must reproduce it bit for bit.

`match_loops` is the same thing as a plain double loop, the check of the
vectorised restatement."""
import numpy as np


def top2(d2):
    """(best index, best value, second value) along axis 1; ties -> lower index;
    second = +inf with one column."""
    n = d2.shape[0]
    best = np.argmin(d2, axis=1)  # first occurrence: the lower index
    bd = d2[np.arange(n), best]
    rest = d2.copy()
    rest[np.arange(n), best] = np.inf
    sec = rest.min(axis=1) if d2.shape[1] > 1 else np.full(n, np.inf, d2.dtype)
    return best, bd, sec


def stats(a, b, dtype=np.float32):
    a = np.asarray(a).astype(dtype)
    b = np.asarray(b).astype(dtype)
    sim = a @ b.T
    na = (a * a).sum(1, dtype=dtype)
    nb = (b * b).sum(1, dtype=dtype)
    d2 = np.maximum((na[:, None] + nb[None, :]) - dtype(2) * sim, dtype(0))
    return d2, top2(d2), top2(np.ascontiguousarray(d2.T))


def match_ref(a, b, ratio=0.8, max_dist=np.inf, n0=None, n1=None, dtype=np.float32):
    """-> dict(partner0, partner1, matches, dist2, count, row=(j, d, s), col=(i, d, s), r2, md2)
    over the valid rows a[:n0], b[:n1]; the outputs have the full sizes."""
    N0, N1 = a.shape[0], b.shape[0]
    n0 = N0 if n0 is None else min(max(int(n0), 0), N0)
    n1 = N1 if n1 is None else min(max(int(n1), 0), N1)
    r2 = dtype(np.float32(ratio * ratio))
    with np.errstate(over="ignore"):
        md2 = dtype(np.float32(max_dist * max_dist))
    K = min(N0, N1)
    out = dict(partner0=np.full(N0, -1, np.int64), partner1=np.full(N1, -1, np.int64),
               matches=np.full((K, 2), -1, np.int64), dist2=np.full(K, -1, np.float32), count=0,
               r2=r2, md2=md2, row=None, col=None)
    if n0 == 0 or n1 == 0:
        return out
    _, (rj, rd, rs), (ci, cd, cs) = stats(a[:n0], b[:n1], dtype)
    with np.errstate(invalid="ignore"):
        rok = (rd <= r2 * rs) & (rd <= md2)
        cok = (cd <= r2 * cs) & (cd <= md2)
    k = 0
    for i in range(n0):
        j = rj[i]
        if rok[i] and cok[j] and ci[j] == i:
            out["partner0"][i] = j
            out["partner1"][j] = i
            out["matches"][k] = (i, j)
            out["dist2"][k] = rd[i]
            k += 1
    out.update(count=k, row=(rj, rd, rs), col=(ci, cd, cs))
    return out


def match_loops(a, b, ratio=0.8, max_dist=np.inf):
    """The definition as loops over (i, j), float32 -> (partner0, partner1, [(i, j, d2)])."""
    f = np.float32
    a, b = np.asarray(a, f), np.asarray(b, f)
    N0, N1 = len(a), len(b)
    r2 = f(ratio * ratio)
    with np.errstate(over="ignore"):
        md2 = f(max_dist * max_dist)
    d2 = np.zeros((N0, N1), f)
    for i in range(N0):
        for j in range(N1):
            sim, na, nb = f(0), f(0), f(0)
            for d in range(a.shape[1]):
                sim = f(sim + f(a[i, d] * b[j, d]))
                na = f(na + f(a[i, d] * a[i, d]))
                nb = f(nb + f(b[j, d] * b[j, d]))
            d2[i, j] = max(f(f(na + nb) - f(f(2) * sim)), f(0))

    def best(row):
        bi, bd, sd = -1, f(np.inf), f(np.inf)
        for j, v in enumerate(row):
            if v < bd:  # strictly smaller: an equal value keeps the lower index
                bi, bd, sd = j, v, bd
            elif v < sd:
                sd = v
        return bi, bd, sd

    rows = [best(d2[i]) for i in range(N0)]
    cols = [best(d2[:, j]) for j in range(N1)]
    p0, p1, pairs = [-1] * N0, [-1] * N1, []
    for i, (j, d, s) in enumerate(rows):
        ci, cd, cs = cols[j]
        if ci == i and d <= f(r2 * s) and cd <= f(r2 * cs) and d <= md2:
            p0[i], p1[j] = j, i
            pairs.append((i, j, d))
    return p0, p1, pairs
