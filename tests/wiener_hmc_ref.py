"""Yardsticks of the batched HMC sampler's statistics tests (csrc/nddm_wiener_hmc.h), in float64 numpy, none of them the code under test:
the basic_ddm_dc posterior of the reference's JAGS model on the sampler's support, its likelihood by tests/wiener_ref.py.  Test
infrastructure only: nothing in the product imports it.

  two free columns (drift, boundary; beta, tau, dc fixed): posterior mean and sd by tensor-grid quadrature of exp(log prior + log
      likelihood), the Jacobian-free density in theta, the grid refined until the moments move by less than 1e-4 sd;
  five free columns, N = 10 trials: self-normalised importance sampling from the prior restricted to the sampler's support (dc >= 0.05,
      tau < T = the smallest response time), weights = the likelihood; the draw count is raised until the effective size is >= 20 000.
Both are computed once per session and shared (functools.lru_cache).  Their values are also recorded in tests/golden/wiener_hmc_yardsticks.json
(`python tests/wiener_hmc_ref.py` writes it; tests/test_wiener_hmc_host.py recomputes both and compares), which is what the GPU tests read:
the importance sampler takes a quarter of a minute of CPU time."""
import functools
import json
import os

import numpy as np

import wiener_ref as W

# signed response times (sign = choice), fixed literals: 20 trials for the two-column case, 10 for the five-column one
Y20 = [0.446, 0.595, 0.492, -0.516, 0.509, 0.943, -0.362, 0.39, 0.538, 0.359, -0.472, 1.343, -0.384, 0.397, 0.458, -0.408, 0.49, 0.432, 1.253,
       0.719]
Y10 = [-0.567, -0.671, -1.06, -0.706, -0.5, 0.577, -0.458, 0.568, -0.385, 0.479]
FIXED_2D = {"beta": 0.5, "tau": 0.2, "dc": 1.0}
DC_MIN = 0.05


def log_g(u, w):
    """wiener_ref.log_g with its series cut where their next term is below 1e-30 of the sum (u < 1: 8 image pairs, next exponent -(2 * 9 - 1)^2 / 2;
    u >= 1: 12 terms, next exponent -168 pi^2 / 2): the same numbers at a tenth of the cost (tests/test_wiener_hmc_host.py compares them)."""
    u, w = np.broadcast_arrays(np.asarray(u, np.float64), np.asarray(w, np.float64))
    small = u < 1.0
    out = np.empty(u.shape)
    if np.any(small):
        out[small] = W.log_g_small(u[small], w[small], K=8)
    if np.any(~small):
        out[~small] = W.log_g_large(u[~small], w[~small], K=12)
    return out


def as_data(y):
    """signed response times -> [N, 2] = (rt, choice)"""
    y = np.asarray(y, np.float64)
    return np.stack([np.abs(y), np.sign(y)], 1).astype(np.float32)


def loglik(y, v, a, beta, tau, s, chunk=200_000):
    """sum over the trials of log f, parameters broadcast to one flat shape [M] -> [M] (float64; -inf where a trial has rt <= tau)"""
    y = np.asarray(as_data(y), np.float64)           # (the float32 values the sampler reads)
    v, a, beta, tau, s = np.broadcast_arrays(*(np.asarray(x, np.float64) for x in (v, a, beta, tau, s)))
    out = np.zeros(v.shape)
    for i0 in range(0, v.size, chunk):
        sl = slice(i0, i0 + chunk)
        acc = np.zeros(v[sl].shape)
        for rt, ch in y:
            t = rt - tau[sl]
            ok = t > 0
            lf = np.full(t.shape, -np.inf)
            if ok.any():
                lf[ok] = W.log_f(t[ok], ch > 0, a[sl][ok], v[sl][ok], beta[sl][ok], s[sl][ok], lg=log_g)
            acc += lf
        out[sl] = acc
    return out


def _grid_moments(n):
    v = np.linspace(-6.0, 6.0, n)
    a = np.linspace(0.05, 5.0, n)
    V, A = np.meshgrid(v, a, indexing="ij")
    lp = -0.125 * V * V - 2.0 * (A - 1.0) ** 2 + loglik(Y20, V.ravel(), A.ravel(), FIXED_2D["beta"], FIXED_2D["tau"], FIXED_2D["dc"]).reshape(V.shape)
    w = np.exp(lp - lp.max())
    w[[0, -1], :] *= 0.5
    w[:, [0, -1]] *= 0.5                                               # trapezoid rule
    w /= w.sum()
    m = np.array([(w * V).sum(), (w * A).sum()])
    sd = np.sqrt(np.array([(w * V * V).sum(), (w * A * A).sum()]) - m * m)
    return m, sd


@functools.lru_cache(maxsize=None)
def yardstick_2d():
    """-> (mean [2], sd [2], the grid size, the last refinement's largest move in sd) for (drift, boundary)"""
    n = 81
    m, sd = _grid_moments(n)
    while True:
        n = 2 * n - 1
        m2, sd2 = _grid_moments(n)
        move = float(max(np.max(np.abs(m2 - m) / sd2), np.max(np.abs(sd2 - sd) / sd2)))
        m, sd = m2, sd2
        if move < 1e-4:
            return m, sd, n, move
        assert n < 2000


def _truncnorm(rng, mu, sg, lo, hi, n):
    out = np.empty(n)
    k = 0
    while k < n:
        x = rng.normal(mu, sg, 2 * (n - k) + 16)
        x = x[(x > lo) & (x < hi)][:n - k]
        out[k:k + x.size] = x
        k += x.size
    return out


@functools.lru_cache(maxsize=None)
def yardstick_5d(block=400_000, need=20_000.0):
    """-> (mean [5], sd [5], the effective sample size, the draws) in (drift, boundary, beta, tau, dc)"""
    rng = np.random.default_rng(77)
    T = min(1.5, float(np.min(np.abs(as_data(Y10)[:, 0]))))
    th, lw = [], []
    while True:
        p = np.stack([rng.normal(0.0, 2.0, block), _truncnorm(rng, 1.0, 0.5, 0.0, 10.0, block), rng.beta(2.0, 2.0, block),
                      _truncnorm(rng, 0.5, 0.25, 0.0, T, block), _truncnorm(rng, 1.0, 0.5, DC_MIN, 10.0, block)], 1)
        th.append(p)
        lw.append(loglik(Y10, p[:, 0], p[:, 1], p[:, 2], p[:, 3], p[:, 4]))
        l = np.concatenate(lw)
        w = np.exp(l - l.max())
        ess = float(w.sum() ** 2 / (w * w).sum())
        if ess >= need:
            break
        assert len(th) < 40
    x = np.concatenate(th)
    w /= w.sum()
    m = (w[:, None] * x).sum(0)
    sd = np.sqrt((w[:, None] * (x - m) ** 2).sum(0))
    return m, sd, ess, x.shape[0]


RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wiener_hmc_yardsticks.json")


def recorded():
    """The recorded yardsticks -> {'two': (mean, sd), 'five': (mean, sd), 'five_ess': float, 'five_draws': int}"""
    with open(RECORD) as f:
        r = json.load(f)
    return {"two": (np.array(r["two_mean"]), np.array(r["two_sd"])), "five": (np.array(r["five_mean"]), np.array(r["five_sd"])),
            "five_ess": r["five_ess"], "five_draws": r["five_draws"], "two_grid": r["two_grid"], "two_last_move_sd": r["two_last_move_sd"]}


if __name__ == "__main__":
    m2, s2, n2, mv = yardstick_2d()
    m5, s5, ess, n5 = yardstick_5d()
    with open(RECORD, "w") as f:
        json.dump({"two_mean": m2.tolist(), "two_sd": s2.tolist(), "two_grid": n2, "two_last_move_sd": mv, "five_mean": m5.tolist(),
                   "five_sd": s5.tolist(), "five_ess": ess, "five_draws": n5}, f, indent=1)
        f.write("\n")
