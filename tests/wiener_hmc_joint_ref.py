"""Yardsticks of the joint sampler's statistics tests (csrc/nddm_wiener_hmc_joint.h), in float64 numpy over tests/wiener_ref.py (through
tests/wiener_hmc_ref.py's loglik), none of them the code under test.  Test infrastructure only: nothing in the product imports it.

The model: participant p has basic_ddm_dc's posterior (wiener_hmc_ref.py), ext_p ~ N(alpha_p, sigma), and sigma ~ N(3, 1) on (0, 10) is
shared.  It factorises: with f_p(alpha) = prior(alpha) int L_p(v, alpha) prior(v) dv,
    p(sigma) ~ prior(sigma) prod_p int f_p(alpha) N(ext_p; alpha, sigma) dalpha,
and the moments of alpha_p and v_p are those of their conditionals given sigma, averaged under p(sigma): a nested quadrature, linear in P.

  (a) drift and boundary free plus sigma; beta, tau, dc fixed at FIXED_2D; P = 4 participants of N = 20 trials: the (v, alpha) grid and the
      sigma grid are refined together until every moment moves by less than 1e-4 sd;
  (b) five free columns, sigma FIXED at 0.3, P = 2 participants of N = 10 trials: per participant, self-normalised importance sampling as
      wiener_hmc_ref.yardstick_5d, the boundary drawn from the product of its prior and the ext term -- a normal of precision 4 + 1 / 0.09,
      truncated to (0, 10) -- and the weights the likelihood; effective size >= 20 000 each.
Both are computed once per session (functools.lru_cache) and recorded in tests/golden/wiener_hmc_joint_yardsticks.json (`python
tests/wiener_hmc_joint_ref.py` writes it; tests/test_wiener_hmc_joint_host.py recomputes and compares); the GPU tests read the record."""
import functools
import json
import os

import numpy as np

import wiener_hmc_ref as R

# signed response times (sign = choice), fixed literals
Y20 = (R.Y20,
       [1.187, 0.541, 0.5, -0.467, -0.534, -0.625, -0.427, 0.581, -0.544, 0.739, 0.669, -0.849, 0.702, -0.449, -0.455, 0.915, 0.42, 0.562, 0.497,
        0.569],
       [-0.701, 0.502, -0.395, -0.355, 0.383, 0.495, 0.365, -0.512, 0.418, 0.468, 0.766, -0.305, 0.297, -0.4, -0.333, 0.684, -0.391, 0.456, 0.604,
        -0.544],
       [0.375, 0.622, -0.504, 0.728, -0.351, 0.432, -0.503, 0.402, -0.612, 0.789, 0.765, 0.758, 0.802, -0.923, -0.718, 0.852, 0.428, 0.696, 0.659,
        -0.487])
EXT_A = (2.4, -0.3, 1.1, 0.2)
Y10 = (R.Y10, [0.502, 0.653, 0.578, -1.327, 0.551, 0.549, 0.326, -0.694, -0.398, 0.611])
EXT_B = (1.2, 0.7)
SIGMA_B = 0.3
FIXED_2D = R.FIXED_2D
A_LO, A_HI, V_HI = 0.02, 5.0, 6.0           # the (v, alpha) box: the prior-times-likelihood mass beyond it is below 1e-12


def _participant_grids(y, n):
    """-> (alpha grid [n], f0, f1, f2 [n]: the sums over v of v^m prior(v) L(v, alpha), times prior(alpha), trapezoid weights included)"""
    v = np.linspace(-V_HI, V_HI, n)
    a = np.linspace(A_LO, A_HI, n)
    V, A = np.meshgrid(v, a, indexing="ij")
    lp = -0.125 * V * V - 2.0 * (A - 1.0) ** 2 + R.loglik(y, V.ravel(), A.ravel(), FIXED_2D["beta"], FIXED_2D["tau"], FIXED_2D["dc"]).reshape(V.shape)
    w = np.exp(lp - lp.max())
    w[[0, -1], :] *= 0.5
    w[:, [0, -1]] *= 0.5
    return a, w.sum(0), (w * V).sum(0), (w * V * V).sum(0)


def _moments_a(n, ns, ext):
    """-> (mean [2 P + 1], sd [2 P + 1]) in the order (v_0, alpha_0, v_1, alpha_1, ..., sigma) from n grid points a side and ns of sigma"""
    sg = (np.arange(ns) + 0.5) * (10.0 / ns)                            # midpoint rule on (0, 10): the integrand vanishes at 0
    logp = -0.5 * (sg - 3.0) ** 2
    cond = []
    for y, e in zip(Y20, ext):
        a, f0, f1, f2 = _participant_grids(y, n)
        k = np.exp(-0.5 * ((e - a[None, :]) / sg[:, None]) ** 2) / sg[:, None]        # N(ext; alpha, sigma) [ns, n] up to 1 / sqrt(2 pi)
        g = k @ f0
        with np.errstate(divide="ignore", invalid="ignore"):            # (a sigma so small that the kernel underflows has p(sigma) = 0)
            logp = logp + np.log(g)
            cond.append(tuple(np.where(g > 0, x / g, 0.0) for x in (k @ f1, k @ f2, k @ (f0 * a), k @ (f0 * a * a))))
    w = np.exp(logp - logp.max())
    w /= w.sum()
    m, s = [], []
    for v1, v2, a1, a2 in cond:
        for x1, x2 in ((v1, v2), (a1, a2)):
            mu = float((w * x1).sum())
            m.append(mu)
            s.append(float(np.sqrt((w * x2).sum() - mu * mu)))
    mu = float((w * sg).sum())
    m.append(mu)
    s.append(float(np.sqrt((w * sg * sg).sum() - mu * mu)))
    return np.array(m), np.array(s)


@functools.lru_cache(maxsize=None)
def yardstick_a(ext=EXT_A):
    """-> (mean [9], sd [9], the grid size, the sigma grid size, the last refinement's largest move in sd)"""
    n, ns = 81, 500
    m, sd = _moments_a(n, ns, ext)
    while True:
        n, ns = 2 * n - 1, 2 * ns
        m2, sd2 = _moments_a(n, ns, ext)
        move = float(max(np.max(np.abs(m2 - m) / sd2), np.max(np.abs(sd2 - sd) / sd2)))
        m, sd = m2, sd2
        if move < 1e-4:
            return m, sd, n, ns, move
        assert n < 1500


@functools.lru_cache(maxsize=None)
def yardstick_b(block=400_000, need=20_000.0):
    """-> (mean [2, 5], sd [2, 5], the effective sizes [2], the draws [2]) in (drift, boundary, beta, tau, dc) per participant"""
    out = []
    for i, (y, e) in enumerate(zip(Y10, EXT_B)):
        rng = np.random.default_rng(177 + i)
        T = min(1.5, float(np.min(np.abs(R.as_data(y)[:, 0]))))
        prec = 4.0 + 1.0 / SIGMA_B ** 2
        mu = (4.0 * 1.0 + e / SIGMA_B ** 2) / prec
        th, lw = [], []
        while True:
            p = np.stack([rng.normal(0.0, 2.0, block), R._truncnorm(rng, mu, prec ** -0.5, 0.0, 10.0, block), rng.beta(2.0, 2.0, block),
                          R._truncnorm(rng, 0.5, 0.25, 0.0, T, block), R._truncnorm(rng, 1.0, 0.5, R.DC_MIN, 10.0, block)], 1)
            th.append(p)
            lw.append(R.loglik(y, p[:, 0], p[:, 1], p[:, 2], p[:, 3], p[:, 4]))
            l = np.concatenate(lw)
            w = np.exp(l - l.max())
            ess = float(w.sum() ** 2 / (w * w).sum())
            if ess >= need:
                break
            assert len(th) < 40
        x = np.concatenate(th)
        w /= w.sum()
        m = (w[:, None] * x).sum(0)
        out.append((m, np.sqrt((w[:, None] * (x - m) ** 2).sum(0)), ess, x.shape[0]))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), [o[2] for o in out], [o[3] for o in out]


RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wiener_hmc_joint_yardsticks.json")


def recorded():
    """The recorded yardsticks -> {'a': (mean [9], sd [9]), 'b': (mean [2, 5], sd [2, 5]), 'b_ess': [2], ...}"""
    with open(RECORD) as f:
        r = json.load(f)
    return {"a": (np.array(r["a_mean"]), np.array(r["a_sd"])), "b": (np.array(r["b_mean"]), np.array(r["b_sd"])), "b_ess": r["b_ess"],
            "b_draws": r["b_draws"], "a_grid": r["a_grid"], "a_sigma_grid": r["a_sigma_grid"], "a_last_move_sd": r["a_last_move_sd"]}


if __name__ == "__main__":
    ma, sa, n, ns, mv = yardstick_a()
    mb, sb, ess, nb = yardstick_b()
    with open(RECORD, "w") as f:
        json.dump({"a_mean": ma.tolist(), "a_sd": sa.tolist(), "a_grid": n, "a_sigma_grid": ns, "a_last_move_sd": mv, "b_mean": mb.tolist(),
                   "b_sd": sb.tolist(), "b_ess": ess, "b_draws": nb}, f, indent=1)
        f.write("\n")
    print(ma, sa, n, ns, mv, mb, sb, ess, nb)
