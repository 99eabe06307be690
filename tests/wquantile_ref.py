"""The definition of the weighted posterior quantiles (amortizer.weighted_draw_quantiles, csrc/train_wquantile.hip) in pure Python
integers and NumPy float64, one (set, column, probability) at a time; independent of torch.  Test infrastructure only: nothing in
the product imports it.

  quantize     log weights -> the integer weights W = rint(exp(log_w - m) 2^36), m the largest finite log_w of the set
  python tests/wquantile_ref.py   writes tests/golden/flow_wquantile.npz: the weighted MEDIAN of the posterior that
               tests/flow_importance_ref.py's yardstick estimates (its data set, its N_REF prior draws under its seed, weight =
               likelihood), per column, by the rule above on float64 weights -- with the yardstick's own mean, sd and effective size
               recomputed beside it (they must equal tests/golden/flow_importance.npz's)
  reference    theta float32 [B, S, D] and integer weights [B, S] -> (quantiles [B, K, D] float64, order [B, K, 2, D] float32,
               n_positive [B])
"""
import bisect
import os
import sys

import numpy as np

ONE = 2 ** 36
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "flow_wquantile.npz")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def quantize(log_w):
    """[B, S] (or [S]) float64 -> int64 of the same shape: NumPy's exp."""
    lw = np.asarray(log_w, dtype=np.float64)
    out = np.zeros(lw.shape, dtype=np.int64)
    for b, row in enumerate(lw.reshape(-1, lw.shape[-1])):
        fin = np.isfinite(row)
        if fin.any():
            m = row[fin].max()
            out.reshape(-1, lw.shape[-1])[b, fin] = np.rint(np.exp(row[fin] - m) * float(ONE)).astype(np.int64)
    return out


def reference(theta, weights, probs):
    theta = np.asarray(theta, dtype=np.float32)
    W = np.asarray(weights)
    assert W.dtype == np.int64 and W.shape == theta.shape[:2]
    B, S, D = theta.shape
    K = len(probs)
    quant, order, n_pos = np.full((B, K, D), np.nan), np.full((B, K, 2, D), np.nan, dtype=np.float32), np.zeros(B, dtype=np.int64)
    inside = np.isfinite(theta).all(axis=-1) & (W >= 1)
    for b in range(B):
        rows = np.flatnonzero(inside[b])
        n = n_pos[b] = len(rows)
        if n == 0:
            continue
        for d in range(D):
            vals = theta[b, rows, d] + np.float32(0.0)                                   # (-0 -> +0)
            o = sorted(range(n), key=lambda i: (vals[i], rows[i]))                       # by value, ties by row index
            xs = [vals[i] for i in o]
            ws = [int(W[b, rows[i]]) for i in o]                                         # Python integers: exact
            c, run = [], 0
            for w in ws:
                run += w
                c.append(2 * run - w - ws[0])
            T, cf = c[-1], [float(v) for v in c]                                         # (exact: every c <= 2^53)
            assert c[0] == 0 and T <= 2 ** 53 and all(c[i + 1] - c[i] == ws[i] + ws[i + 1] for i in range(n - 1))
            for j, p in enumerate(probs):
                h = np.float64(p) * np.float64(T)
                k = bisect.bisect_right(cf, float(h)) - 1                                # the largest k with (double) c_k <= h
                if k == n - 1:
                    a = e = xs[k]
                    g = np.float64(0.0)
                else:
                    a, e = xs[k], xs[k + 1]
                    g = (h - np.float64(c[k])) / np.float64(ws[k] + ws[k + 1])
                order[b, j, 0, d], order[b, j, 1, d] = a, e
                quant[b, j, d] = np.float64(a) + (np.float64(e) - np.float64(a)) * g
    return quant, order, n_pos


def check(res, theta, weights, probs):
    """res: weighted_draw_quantiles' dictionary (tensors) for theta (numpy float32) and the integer weights: order equal as numbers
    (-0 == +0), quantiles bit for bit, n_positive equal."""
    quant, order, n_pos = reference(theta, weights, probs)
    got_q, got_o, got_n = (res[k].cpu().numpy() for k in ("quantiles", "order", "n_positive"))
    assert got_q.dtype == np.float64 and got_o.dtype == np.float32 and got_n.dtype == np.int64
    assert got_q.shape == quant.shape and got_o.shape == order.shape and np.array_equal(got_n, n_pos), (got_n, n_pos)
    assert np.array_equal(got_o, order, equal_nan=True)
    assert np.array_equal(bits(got_q), bits(quant)), np.nanmax(np.abs(got_q - quant))


def skewed_log_w(rng, B, S):
    """Random skewed log weights: a heavy right tail (a few draws carry most of the mass), an offset per set, some zero weights."""
    lw = rng.normal(-700.0, 3.0, size=(B, S)) + rng.exponential(2.0, size=(B, S)) + rng.normal(0.0, 50.0, size=(B, 1))
    lw[rng.random((B, S)) < 0.05] = -np.inf
    if S > 2:
        lw[:, 0] = np.where(np.isfinite(lw[:, 0]), lw[:, 0], -700.0)                     # (not every weight zero)
    return lw


def crafted_cases():
    """(name, theta float32 [B, S, D], log_w float64 [B, S]): the rows a weighted selection goes wrong on."""
    rng = np.random.default_rng(23)
    ties = rng.choice(np.array([-1.5, 0.25, 0.25000003, 7.0], dtype=np.float32), size=(2, 300, 3))
    ties_w = np.log(rng.choice([1.0, 3.0, 1e-3, 250.0], size=(2, 300)))                  # tie order visible: the last of a group's weight
    zeros = rng.choice(np.array([0.0, -0.0, 1e-3, -1e-3], dtype=np.float32), size=(1, 129, 2), p=[.4, .4, .1, .1])
    zeros_w = rng.normal(size=(1, 129))
    bad = rng.normal(size=(2, 150, 4)).astype(np.float32)
    bad[0, 3, 1], bad[0, 77, 2], bad[0, 149, 0], bad[1, 0, 3] = np.nan, np.inf, -np.inf, np.nan
    bad_w = rng.normal(size=(2, 150))
    odd = rng.normal(size=(1, 70, 2)).astype(np.float32)
    odd_w = rng.normal(size=(1, 70))
    odd_w[0, 5], odd_w[0, 6], odd_w[0, 7], odd_w[0, 69] = -np.inf, np.inf, np.nan, np.inf
    none = rng.normal(size=(2, 66, 3)).astype(np.float32)
    none_w = np.full((2, 66), -np.inf)
    none_w[1, ::2] = np.nan
    none_w[0, 0], none[0, 0, 1] = 0.0, np.nan                                            # the only weight belongs to a row that is not finite
    dom = rng.normal(size=(2, 200, 3)).astype(np.float32)
    dom_w = rng.uniform(-80.0, -40.0, size=(2, 200))
    dom_w[0, 41], dom_w[1, 199] = 0.0, 3.0
    span = rng.normal(size=(1, 257, 2)).astype(np.float32)
    span_w = np.log(2.0) * rng.integers(0, 31, size=(1, 257)).astype(np.float64)         # weights over a factor of 2^30
    span_w[0, 3], span_w[0, 100] = 0.0, 30.0 * np.log(2.0)
    return [("ties with different weights", ties, ties_w), ("zeros", zeros, zeros_w), ("nan / inf components", bad, bad_w),
            ("log_w -inf, +inf, nan", odd, odd_w), ("all-zero sets", none, none_w), ("one dominating weight", dom, dom_w),
            ("weights over 2^30", span, span_w)]


def weighted_median_float(x, u):
    """The rule with float64 weights u > 0 (a yardstick: no integers, NumPy's sums): per column of x [n, D] the value at h = T / 2."""
    out = np.empty(x.shape[1])
    for d in range(x.shape[1]):
        o = np.argsort(x[:, d], kind="stable")
        xs, ws = x[o, d], u[o]
        c = 2.0 * np.cumsum(ws) - ws - ws[0]
        out[d] = np.interp(0.5 * c[-1], c, xs)
    return out


def main():
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import flow_importance_ref as F
    from bayesflow_nddms_amd import priors
    g = np.load(F.GOLDEN)
    trials = g["trials"].astype(np.float64)
    theta = priors.basic_prior_matrix(F.N_REF, seed=2).astype(np.float64)                # posterior_from_the_prior's draws
    live = np.flatnonzero(theta[:, 3] < trials[:, 0].min())
    ll = F.log_lik_basic(theta[live], trials)
    keep = np.isfinite(ll)
    live, ll = live[keep], ll[keep]
    u = np.exp(ll - ll.max())
    x = theta[live]
    sw = u.sum()
    mean = (u[:, None] * x).sum(0) / sw
    sd = np.sqrt((u[:, None] * x ** 2).sum(0) / sw - mean ** 2)
    ess = sw * sw / (u * u).sum()
    assert np.allclose(mean, g["mean"], rtol=1e-9) and np.allclose(sd, g["sd"], rtol=1e-9) and np.isclose(ess, float(g["ess"]), rtol=1e-9)
    pos = u > 0
    median = weighted_median_float(x[pos], u[pos])
    print("median", median, "\nmean", mean, "\nsd", sd, "ess", ess, "of", F.N_REF)
    np.savez(GOLDEN, median=median, mean=mean, sd=sd, ess=ess, n_ref=F.N_REF)


if __name__ == "__main__":
    main()
