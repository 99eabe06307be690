"""Pareto-smoothed importance weights in NumPy float64, one data set at a time: the definition amortizer.pareto_smooth and
csrc/train_psis.hip are held to (tests/test_flow_psis_cpu.py, tests/test_gpu_flow_psis.py).  Test infrastructure only: nothing in the
product imports it.

  tail_size, k_threshold   M(S) and the diagnostic's bar
  psis                     the definition; `order` chooses how its sums run ("forward", "reversed", "fsum")
  tolerances               the bars of the approximate parts: 1000 x what the three orders differ by on the tests' own inputs
  crafted_cases            the sets at which a smoothing kernel goes wrong
  check                    a result (dict of arrays, as pareto_smooth returns) against the definition
"""
import functools
import math

import numpy as np

LOG_DBL_MIN = -708.3964185322641
SIZES = (1, 4, 24, 25, 26, 64, 65, 257, 1000, 4097, 10_000)
SCALES = (0.3, 1.0, 3.0, 10.0, 30.0)


def tail_size(S):
    """M = min(ceil(S / 5), ceil(3 sqrt(S))), in integers."""
    return min((S + 4) // 5, math.isqrt(9 * S - 1) + 1)


def k_threshold(S):
    return min(1.0 - 1.0 / math.log10(S), 0.7) if S > 1 else -math.inf


def _sum(v, order):
    v = np.asarray(v, np.float64)
    if order == "fsum":
        return np.float64(math.fsum(v.tolist())) if np.all(np.isfinite(v)) else v.sum()
    return np.cumsum(v if order == "forward" else v[::-1])[-1]          # (cumsum: one term after the other)


def fit(y, order="forward"):
    """Zhang and Stephens' estimator with the PSIS prior on the sorted exceedances y [n] -> (pareto_k, sigma)."""
    with np.errstate(all="ignore"):
        n = len(y)
        m_est = 30 + math.isqrt(n)
        j = np.arange(1, m_est + 1, dtype=np.float64)
        yq = y[int(math.floor(n / 4.0 + 0.5)) - 1]
        bj = (1.0 - np.sqrt(m_est / (j - 0.5))) / (3.0 * yq) + 1.0 / y[n - 1]
        kj = np.array([_sum(np.log1p(-b * y), order) / n for b in bj])
        Lj = n * (np.log(-bj / kj) - kj - 1.0)
        wj = np.array([1.0 / _sum(np.exp(Lj - L), order) for L in Lj])
        wj = wj / _sum(wj, order)
        b = _sum(bj * wj, order)
        k_raw = _sum(np.log1p(-b * y), order) / n
        return np.float64((n * k_raw + 5.0) / (n + 10.0)), np.float64(-k_raw / b)


def psis(lw, M=None, order="forward"):
    """log weights [S] -> {"pareto_k", "sigma", "cutoff", "n_tail", "log_w" [S], "rows": the tail's rows by rank}."""
    lw = np.asarray(lw, np.float64)
    S = lw.shape[0]
    M = tail_size(S) if M is None else M
    out = lw.copy()
    res = {"pareto_k": np.float64(np.inf), "sigma": np.float64(np.nan), "cutoff": np.float64(LOG_DBL_MIN), "n_tail": 0, "log_w": out,
           "rows": np.zeros(0, np.int64)}
    fin = np.isfinite(lw)
    if not fin.any():
        return res
    m = lw[fin].max()
    x = np.full(S, -np.inf)
    x[fin] = lw[fin] - m
    c = np.sort(x)[S - M - 1] if S - M - 1 >= 0 else -np.inf
    cutoff = max(c, LOG_DBL_MIN)
    rows = np.nonzero(x > cutoff)[0]
    rows = rows[np.argsort(x[rows], kind="stable")]                     # ascending by value, ties by row index
    n = len(rows)
    res.update(cutoff=np.float64(cutoff), n_tail=n, rows=rows)
    if n <= 4:
        return res
    e_c = np.exp(cutoff)
    y = np.exp(x[rows]) - e_c
    k, sigma = fit(y, order)
    res.update(pareto_k=k, sigma=sigma)
    if not (np.isfinite(k) and np.isfinite(sigma) and sigma > 0.0):
        return res
    with np.errstate(all="ignore"):
        p = (np.arange(n) + 0.5) / n
        q = -sigma * np.log1p(-p) if k == 0.0 else sigma * np.expm1(-k * np.log1p(-p)) / k
        out[rows] = m + np.minimum(np.log(q + e_c), 0.0)
    return res


def batch(lw, order="forward"):
    """psis of every row of lw [B, S], stacked as amortizer.pareto_smooth stacks them."""
    rs = [psis(row, order=order) for row in np.asarray(lw, np.float64)]
    out = {k: np.array([r[k] for r in rs]) for k in ("pareto_k", "sigma", "cutoff", "n_tail")}
    out["log_w"] = np.stack([r["log_w"] for r in rs])
    return out


def gaussian_log_w(S, s, seed):
    return np.random.default_rng(seed).normal(0.0, s, S)


def grid():
    """The definition test's inputs: (S, s, log weights [S])."""
    return [(S, s, gaussian_log_w(S, s, 1000 * i + j)) for i, S in enumerate(SIZES) for j, s in enumerate(SCALES)]


def _rel(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


@functools.lru_cache(maxsize=None)
def tolerances():
    """(bar for pareto_k, absolute; bar for sigma and the smoothed values, relative to max(1, |value|)): 1000 x the largest difference the
    definition shows against itself under the three summation orders on grid()'s inputs."""
    dk, dv = 0.0, 0.0
    for _, _, lw in grid():
        a = psis(lw, order="forward")
        if not np.isfinite(a["pareto_k"]):
            continue
        for order in ("reversed", "fsum"):
            b = psis(lw, order=order)
            dk = max(dk, abs(float(a["pareto_k"] - b["pareto_k"])))
            dv = max(dv, float(_rel(a["sigma"], b["sigma"])), float(_rel(a["log_w"], b["log_w"]).max()))
    return 1000.0 * dk, 1000.0 * dv


def crafted_cases():
    """name -> (log weights [S] float64, what must hold: a dict of n_tail, finite (is pareto_k), changed (are rows rewritten))."""
    rng = np.random.default_rng(11)
    ninf = -np.inf
    cases = {}
    cases["equal weights"] = (np.full(100, -3.25), dict(n_tail=0, finite=False, changed=False))
    one = np.full(50, ninf)
    one[17] = 2.5
    cases["one positive weight"] = (one, dict(n_tail=1, finite=False, changed=False))
    for n in (5, 6):
        lw = np.full(200, ninf)
        lw[rng.choice(200, n, replace=False)] = rng.normal(0.0, 1.0, n)
        # (M = 40: the rank S - M - 1 holds -inf, the floor applies, and all n finite rows but none else are the tail)
        cases[f"exactly {n} finite weights"] = (lw, dict(n_tail=n, finite=True, changed=None))
    big = rng.normal(-745.0, 1.0, 300)
    big[150] += 800.0
    cases["one weight e^800 above the rest"] = (big, dict(n_tail=1, finite=False, changed=False))
    mixed = rng.normal(0.0, 2.0, 400)
    mixed[[3, 50, 399]] = np.nan
    mixed[[7, 90]] = np.inf
    mixed[[0, 11, 200, 201]] = ninf
    cases["nan, +inf and -inf entries"] = (mixed, dict(n_tail=tail_size(400), finite=True, changed=True))
    tie = rng.normal(0.0, 1.0, 500)
    srt = np.sort(tie)
    M = tail_size(500)
    tie[tie == srt[500 - M]] = srt[500 - M - 1]                          # the lowest tail value now equals the cutoff: it leaves the tail
    cases["a tie straddling the cutoff"] = (tie, dict(n_tail=M - 1, finite=True, changed=True))
    inside = rng.normal(0.0, 1.0, 500)
    o = np.argsort(inside)
    inside[o[-5]] = inside[o[-6]] = inside[o[-7]]                        # three equal values inside the tail, at scattered rows
    inside[o[-30]] = inside[o[-31]]
    cases["ties inside the tail"] = (inside, dict(n_tail=None, finite=True, changed=True))
    # S = 100, M = 20: the largest weight at 0, the other 19 tail values at -1e-3 and the cutoff one ulp (2e-19) below them -- another
    # double with the same exp, so y = exp(x) - exp(cutoff) is 0 up to the quartile and beyond: 1 / (3 y_q) is not finite
    flat = rng.normal(-5.0, 0.1, 100)
    flat[79] = -1e-3 - np.spacing(1e-3)
    flat[80:99] = -1e-3
    flat[99] = 0.0
    cases["no exp difference at the quartile"] = (flat, dict(n_tail=20, finite=False, changed=False))
    return cases


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def check(got, lw, label=""):
    """got: pareto_smooth's result on lw [B, S] as NumPy arrays.  The exact parts equal the definition exactly -- n_tail, cutoff, which
    rows changed, the bits of the rows that did not; a pareto_k that is not finite is the same non-finite value -- and the approximate
    parts are within tolerances().  -> (largest |k - ref|, largest relative difference of sigma and the smoothed values)."""
    lw = np.asarray(lw, np.float64)
    tol_k, tol_v = tolerances()
    worst_k, worst_v = 0.0, 0.0
    assert got["log_w"].shape == lw.shape and got["log_w"].dtype == np.float64, label
    for b in range(lw.shape[0]):
        ref = psis(lw[b])
        tag = (label, b)
        assert int(got["n_tail"][b]) == ref["n_tail"], (tag, int(got["n_tail"][b]), ref["n_tail"])
        assert got["cutoff"][b] == ref["cutoff"], (tag, got["cutoff"][b], ref["cutoff"])
        k, rk = float(got["pareto_k"][b]), float(ref["pareto_k"])
        out = got["log_w"][b]
        changed = np.zeros(lw.shape[1], bool)
        if np.isfinite(rk) and np.isfinite(ref["sigma"]) and ref["sigma"] > 0.0:
            changed[ref["rows"]] = True
        assert same_bits(out[~changed], lw[b][~changed]), tag
        if not np.isfinite(rk):
            assert not np.isfinite(k) and (np.isnan(k) == np.isnan(rk)) and (np.isnan(k) or k == rk), (tag, k, rk)
            continue
        assert np.isfinite(k) and abs(k - rk) <= tol_k, (tag, k, rk, tol_k)
        worst_k = max(worst_k, abs(k - rk))
        dv = float(_rel(got["sigma"][b], ref["sigma"]))
        if changed.any():
            dv = max(dv, float(_rel(out[changed], ref["log_w"][changed]).max()))
        assert dv <= tol_v, (tag, dv, tol_v)
        worst_v = max(worst_v, dv)
    return worst_k, worst_v
