"""Float64 yardstick of the GRADIENT of the single-trial model's marginal log-likelihood (csrc/nddm_wiener_marginal_grad.h, DESIGN.md
section 16): the gradient of wiener_marginal_ref.log_lik in the eight parameter columns, by differentiation under the integral on the
yardstick's own composite rule.  Test infrastructure only: nothing in the product imports it.  tests/test_wiener_marginal_grad_host.py pins it
against Richardson-extrapolated central differences of wiener_marginal_ref.log_lik itself.

One trial: log L = outside(z; mu, sd, sigma1, gamma) + log int e^{l(x)} dx, l = log h(a = e^x) + x + log N(a; m, tau^2), so
    d/dtheta log L = d/dtheta outside + E[d/dtheta l],   E over the normalised integrand on the rule's nodes
(the window ends where the integrand is e^-90 of its peak: it is not differentiated).  At fixed x the boundary a is fixed, so
    d/d(drift, beta, ter, dc) l = the partials of log h in the basic model's columns (v, beta, tau, s) at boundary a: wiener_grad_ref.trial_grad
        for a response; for a timeout, Richardson-extrapolated central differences, per node, of wiener_marginal_ref.log_h in (drift, beta, dc)
        (d/dter = 0: t_censor is a constant of the call)
    d/d(mu, sd, sigma1, gamma) l = (a - m) / tau^2 dm/dtheta + ((a - m)^2 / tau^3 - 1 / tau) dtau/dtheta
with m and tau differentiated in the yardstick's own precision form (tau^2 = 1 / P, m = B / P, P = 1 / sd^2 + gamma^2 / sigma1^2,
B = mu / sd^2 + gamma z / sigma1^2) -- not in the form the header's chain rule uses, so that the two are independent restatements.
"""
import numpy as np
from scipy.special import log_ndtr

import wiener_grad_ref as G
import wiener_marginal_ref as M

COLUMNS = ("drift", "mu_alpha", "beta", "ter", "std_alpha", "dc", "sigma1", "gamma")
FD_STEP = 1e-3            # relative step of the per-node differences of log S (1e-4 leaves their rounding noise at 8e-8 on the box)
CONVERGED = 1e-7          # the rule and the rule with twice the panels agree to this, of max(1, |d|), in every column (responses agree to
                          # 1e-11; a timeout's per-node differences carry log_h's rounding noise over the step, 2.5e-8 at the most on the box)

# The device tests' bars, per row set, in units of scale_j (the sum over a row's trials of |per-trial d/dtheta_j log L|): 4 x the largest error
# of the header's own code compiled for the host over the POOL rows of the set, one trial per row, rounded up to one significant digit
# (tools/wiener_marginal_grad_host.py, profiles/r16_wiener_marginal_grad_host.json: 0.0050 on prior_rows, row 192's dc column, and 0.047 on
# box, row 90's sigma1 column -- both rows where the column's derivative crosses zero, |d| = 0.036 and 0.016 beside columns of order 1 and
# 1e3: with ONE trial per row scale_j is the derivative itself; the 99th percentiles are 2.8e-4 and 2.5e-4 at the most)
DEVICE_BAR = {"prior_rows": 0.02, "box": 0.2}


def _window(f, t, m, tau, p):
    """wiener_marginal_ref.log_lik's integration window: two scans of the widest window float64 can hold."""
    lo = np.full(t.shape, np.log(1e-6))
    hi = np.log(np.maximum(m, 0.0) + 40.0 * tau + 1e3 * p[:, 5] * (1.0 + np.sqrt(t) + np.abs(p[:, 0] / p[:, 5]) * t))
    for _ in range(2):
        x = lo[:, None] + (hi - lo)[:, None] * np.arange(M.SCAN)[None, :] / (M.SCAN - 1.0)
        L = f(x)
        inb = L >= L.max(1)[:, None] - 1.5 * M.BAND
        first, last = np.argmax(inb, 1), M.SCAN - 1 - np.argmax(inb[:, ::-1], 1)
        rows = np.arange(t.size)
        lo, hi = x[rows, np.maximum(first - 2, 0)], x[rows, np.minimum(last + 2, M.SCAN - 1)]
    return lo, hi


def _nodes(lo, hi, panels):
    g, wt = M._gl(M.NODES)
    edges = lo[:, None] + (hi - lo)[:, None] * np.arange(panels + 1)[None, :] / panels
    c, r = 0.5 * (edges[:, 1:] + edges[:, :-1]), 0.5 * (edges[:, 1:] - edges[:, :-1])
    x = (c[:, :, None] + r[:, :, None] * g[None, None, :]).reshape(lo.size, -1)
    lw = np.log(np.broadcast_to(r[:, :, None] * wt[None, None, :], (lo.size, panels, M.NODES)).reshape(lo.size, -1))
    return x, lw


def _richardson(f, x, h):
    cd = lambda s: (f(x + s) - f(x - s)) / (2.0 * s)
    return (4.0 * cd(0.5 * h) - cd(h)) / 3.0


def dlog_survival(t, a, drift, beta, dc):
    """Partials of wiener_marginal_ref.log_h's timeout branch, log P(T > t | a / dc, drift / dc, beta), in (drift, beta, dc), arrays of one
    shape: Richardson-extrapolated central differences in float64."""
    code = np.zeros(a.shape)
    h = lambda dr, b, s: M.log_h(a, t, code, dr, b, s)
    d_v = _richardson(lambda v: h(v, beta, dc), drift, FD_STEP * np.maximum(np.abs(drift), dc))
    d_b = _richardson(lambda b: h(drift, b, dc), beta, FD_STEP * np.minimum(beta, 1.0 - beta))
    d_s = _richardson(lambda s: h(drift, beta, s), dc, FD_STEP * dc)
    return d_v, d_b, d_s


def _dlog_h(a, t, code, drift, beta, dc):
    """Partials of log h at boundary a in (drift, beta, ter, dc): [..., 4]."""
    out = np.zeros(a.shape + (4,))
    r = code != 0
    if np.any(r):
        pb = np.stack([drift[r], a[r], beta[r], np.zeros(r.sum()), dc[r]], -1)
        g = G.trial_grad(True, pb, t[r], code[r] > 0)
        out[r] = g[:, [0, 2, 3, 4]]
    c = ~r
    if np.any(c):
        d_v, d_b, d_s = dlog_survival(t[c], a[c], drift[c], beta[c], dc[c])
        out[c] = np.stack([d_v, d_b, np.zeros(c.sum()), d_s], -1)
    return out


def _gaussian_partials(p, z):
    """(dm/dtheta [n, 4], dtau/dtheta [n, 4], d outside/dtheta [n, 4]) in theta = (mu, sd, sigma1, gamma), from the precision form."""
    drift, mu, beta, ter, sd, dc, s1, g = M.columns(p)
    P = 1.0 / sd ** 2 + g * g / s1 ** 2
    B = mu / sd ** 2 + g * z / s1 ** 2
    m = B / P
    zero = np.zeros_like(mu)
    dP = np.stack([zero, -2.0 / sd ** 3, -2.0 * g * g / s1 ** 3, 2.0 * g / s1 ** 2], -1)
    dB = np.stack([1.0 / sd ** 2, -2.0 * mu / sd ** 3, -2.0 * g * z / s1 ** 3, z / s1 ** 2], -1)
    dm = (dB - m[:, None] * dP) / P[:, None]
    dtau = -0.5 * P[:, None] ** -1.5 * dP
    s2m = s1 * s1 + g * g * sd * sd
    ds2m = np.stack([zero, 2.0 * g * g * sd, 2.0 * s1, 2.0 * g * sd * sd], -1)
    dz = z - g * mu
    ddz = np.stack([-g, zero, zero, -mu], -1)
    x = mu / sd
    mills = np.exp(-0.5 * x * x - 0.5 * np.log(2.0 * np.pi) - log_ndtr(x))
    dx = np.stack([1.0 / sd, -mu / sd ** 2, zero, zero], -1)
    dout = (-0.5 / s2m + dz * dz / (2.0 * s2m * s2m))[:, None] * ds2m - (dz / s2m)[:, None] * ddz - mills[:, None] * dx
    return dm, dtau, dout


def grad_log_lik(p, y, z, t_censor, check=True):
    """The yardstick: float64 gradient of wiener_marginal_ref.log_lik per row, p [n, 8], y [n], z [n] (one trial per row) -> [n, 8] in
    COLUMNS' order.  A response at or below ter gives NaN.  check: the rule with half the panels must agree (AssertionError otherwise)."""
    p, y, z = np.asarray(p, np.float64), np.asarray(y, np.float64), np.asarray(z, np.float64)
    t, code = M.trial_parts(p, y, t_censor)
    out = np.full(y.shape + (8,), np.nan)
    keep = t > 0
    if not np.any(keep):
        return out
    p, t, code, z = p[keep], t[keep], code[keep], z[keep]
    m, tau, _ = M.gaussian_parts(p, z)
    f = lambda x: M._integrand(x, p, t, code, m, tau)
    lo, hi = _window(f, t, m, tau, p)
    dm, dtau, dout = _gaussian_partials(p, z)
    res = []
    for panels in ((M.PANELS, 2 * M.PANELS) if check else (2 * M.PANELS,)):
        x, lw = _nodes(lo, hi, panels)
        L = f(x) + lw
        W = np.exp(L - L.max(1)[:, None])
        W /= W.sum(1)[:, None]
        a = np.exp(x)
        bc = lambda v: np.broadcast_to(v[:, None], x.shape).ravel()
        dh = _dlog_h(a.ravel(), bc(t), bc(code), bc(p[:, 0]), bc(p[:, 2]), bc(p[:, 5])).reshape(x.shape + (4,))
        eh = np.einsum("nk,nkj->nj", W, dh)                             # E[d/d(drift, beta, ter, dc) log h]
        d = a - m[:, None]
        e_m = np.sum(W * d, 1) / tau ** 2
        e_t = np.sum(W * d * d, 1) / tau ** 3 - 1.0 / tau
        gs = e_m[:, None] * dm + e_t[:, None] * dtau + dout            # (mu, sd, sigma1, gamma)
        res.append(np.stack([eh[:, 0], gs[:, 0], eh[:, 1], eh[:, 2], gs[:, 1], eh[:, 3], gs[:, 2], gs[:, 3]], -1))
    if check:
        err = np.abs(res[0] - res[1]) / np.maximum(1.0, np.abs(res[1]))
        bad = ~(err.max(1) < CONVERGED)
        assert not np.any(bad), f"the gradient yardstick's rule has not converged on rows {np.flatnonzero(bad)[:8]}: {err.max(1)[bad][:8]}"
    out[keep] = res[-1]
    return out


def pairs_grad(p32, y32, z32, t_censor, check=True):
    """The yardstick on every (row, trial) pair: p32 [R, 8], y32 / z32 [R, K] -> float64 per-trial gradients [R, K, 8]."""
    R, K = y32.shape
    p, y, z = M.as_f64(np.repeat(p32, K, 0), y32.reshape(-1), z32.reshape(-1))
    return grad_log_lik(p, y, z, t_censor, check).reshape(R, K, 8)


def fd_grad(p, y, z, t_censor, rel=2e-3):
    """Richardson-extrapolated central differences of wiener_marginal_ref.log_lik in every column, from relative steps `rel` and `rel` / 2;
    ter's step is scaled to the decision time |y| - ter (t_censor for a timeout: log L does not depend on ter there)."""
    p, y, z = np.asarray(p, np.float64), np.asarray(y, np.float64), np.asarray(z, np.float64)
    out = np.empty(p.shape)
    for j in range(8):
        scale = np.where(y == 0, float(t_censor or 1.0), np.abs(y) - p[:, 3]) if j == 3 else np.abs(p[:, j])

        def cd(step):
            hi, lo = p.copy(), p.copy()
            hi[:, j] += step
            lo[:, j] -= step
            return (M.log_lik(hi, y, z, t_censor) - M.log_lik(lo, y, z, t_censor)) / (2.0 * step)
        h = rel * scale
        out[:, j] = (4.0 * cd(0.5 * h) - cd(h)) / 3.0
    return out
