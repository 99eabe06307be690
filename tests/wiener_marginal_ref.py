"""Float64 yardstick of the single-trial model's marginal log-likelihood (csrc/nddm_wiener_marginal.h).  Test
infrastructure only: nothing in the product imports it.

One trial (choicert y, z1 z) of NDDM_SINGLE_TRIAL with drift, mu_alpha, beta, ter, std_alpha, dc, sigma1, gamma:
    a ~ N(mu_alpha, std_alpha^2) given a > 0;  z ~ N(gamma a, sigma1^2);  |y| - ter the first passage of the eta = 0 Wiener process with
    a' = a / dc, v' = drift / dc, w = beta on the boundary the sign of y names;  y == 0: no passage before t_censor.
N(z; gamma a, sigma1^2) N(a; mu, sd^2) = N(z; gamma mu, sigma1^2 + gamma^2 sd^2) N(a; m, tau^2), tau^2 = 1 / (1 / sd^2 + gamma^2 / sigma1^2),
m = tau^2 (mu / sd^2 + gamma z / sigma1^2), so
    log L = log N(z; gamma mu, sigma1^2 + gamma^2 sd^2) - log Phi(mu / sd) + log int_0^inf h(a) N(a; m, tau^2) da
with h(a) = f_W(|y| - ter | a / dc, drift / dc, beta) (wiener_ref.log_f) for a response and P(T > t_censor | ...) for a timeout
(1 - wiener_cdf_ref.cdf of both boundaries; the survival series where that difference has lost its digits).

log_lik: the integral in x = log a by a composite Gauss-Legendre rule on the band where the log integrand is within 1.5 BAND of its largest
value, found by two scans of the widest window float64 can hold; the rule is repeated with twice the panels and the two must agree to 1e-9
(AssertionError otherwise: a row the yardstick cannot score does not belong in a row set).
scheme_log_lik: the SHIPPED quadrature (three zoom passes of 32 Gauss-Legendre nodes in x from the hull window) restated in float64 on the
same integrand: what the rule itself costs, apart from float32.
"""
import functools

import numpy as np
from scipy.special import log_ndtr

import wiener_cdf_ref as C
import wiener_ref as W

BAND = 60.0               # the yardstick integrates where the log integrand is within 1.5 BAND of its maximum (e^-90 of the peak beyond)
SCAN = 2000               # points of each scan
PANELS, NODES = 24, 40    # the composite rule, and twice the panels for its own check
CONVERGED = 1e-9

# the device tests' bars: 4 x the largest float32 error of the header on the host over POOL rows of the set, rounded up to one significant
# digit (tools/wiener_marginal_host.py, profiles/r13_wiener_marginal_host.json: 4.6e-5 on prior_rows; 9.1e-4 on box, at log L = -4978)
DEVICE_BAR = {"prior_rows": 2e-4, "box": 4e-3}

# the shipped scheme's constants (csrc/nddm_wiener_marginal.h)
K_NODES, PASSES, ZOOM_BAND, L_TAU, C_CUT, S_SIGMAS = 32, 3, 20.7, 6.5, 60.0, 6.0


def _lg(u, w):
    """wiener_ref's standard density with the terms float64 needs and no more (k = -12..12 below u = 1, 1..20 above: the next terms are
    below e^-280 of the first)."""
    u, w = np.broadcast_arrays(np.asarray(u, np.float64), np.asarray(w, np.float64))
    small = u < 1.0
    out = np.empty(u.shape)
    if np.any(small):
        out[small] = W.log_g_small(u[small], w[small], K=12)
    if np.any(~small):
        out[~small] = W.log_g_large(u[~small], w[~small], K=20)
    return out


def _log_survival(t, a, v, beta, s):
    """log P(T > t) over both boundaries, arrays of one shape: log(1 - F_lower - F_upper) where that keeps ten digits, the survival series
    (wiener_ref.survival's, the first exponent taken out) below."""
    F = C.cdf(t, False, a, v, beta, s, nodes=1) + C.cdf(t, True, a, v, beta, s, nodes=1)
    S = 1.0 - F
    ok = S >= 1e-6
    ap, vp = a / s, v / s
    k = np.arange(1, 61, dtype=np.float64).reshape((-1,) + (1,) * ap.ndim)
    kk = np.pi ** 2 / (2.0 * ap * ap)
    lam1 = vp * vp / 2.0 + kk
    with np.errstate(all="ignore"):
        tot = 0.0
        d0l, d0u = -ap * vp * beta, ap * vp * (1.0 - beta)
        mx = np.maximum(d0l, d0u)
        for w, d0 in ((beta, d0l), (1.0 - beta, d0u)):
            tot = tot + np.exp(d0 - mx) * np.sum(k * np.sin(k * np.pi * w) * np.exp(-kk * (k * k - 1.0) * t) / (vp * vp / 2.0 + kk * k * k), axis=0)
        series = -lam1 * t + mx + np.log(np.pi / (ap * ap)) + np.log(np.maximum(tot, 1e-300))
        return np.where(ok, np.log(np.where(ok, S, 1.0)), series)


def log_h(a, t, code, drift, beta, dc):
    """log h(a), arrays of one shape: code 1 / -1 a response on the upper / lower boundary at decision time t, 0 a timeout at t."""
    out = np.empty(a.shape)
    r = code != 0
    if np.any(r):
        out[r] = W.log_f(t[r], code[r] > 0, a[r], drift[r], beta[r], dc[r], lg=_lg)
    if np.any(~r):
        c = ~r
        out[c] = _log_survival(t[c], a[c], drift[c], beta[c], dc[c])
    return out


def columns(p):
    p = np.asarray(p, np.float64)
    return tuple(p[:, j] for j in range(8))


def gaussian_parts(p, z):
    """float64 (m, tau, the log of everything outside the integral) per row."""
    drift, mu, beta, ter, sd, dc, s1, g = columns(p)
    s2m = s1 * s1 + g * g * sd * sd
    tau2 = sd * sd * s1 * s1 / s2m
    m = (mu * s1 * s1 + g * z * sd * sd) / s2m
    outside = -0.5 * np.log(2.0 * np.pi * s2m) - (z - g * mu) ** 2 / (2.0 * s2m) - log_ndtr(mu / sd)
    return m, np.sqrt(tau2), outside


def trial_parts(p, y, t_censor):
    """(decision time, code) of choicert y: code 1 / -1 / 0 as log_h takes them."""
    ter = np.asarray(p, np.float64)[:, 3]
    code = np.sign(y)
    t = np.where(code == 0, np.nan if t_censor is None else float(t_censor), np.abs(y) - ter)
    return t, code


def _integrand(x, p, t, code, m, tau):
    """log of h(a) N(a; m, tau^2) a at a = e^x, x [n, k]."""
    drift, mu, beta, ter, sd, dc, s1, g = columns(p)
    a = np.exp(x)
    bc = lambda v: np.broadcast_to(v[:, None], x.shape)
    lh = log_h(a.ravel(), bc(t).ravel(), bc(code).ravel(), bc(drift).ravel(), bc(beta).ravel(), bc(dc).ravel()).reshape(x.shape)
    return lh + x - (a - m[:, None]) ** 2 / (2.0 * tau[:, None] ** 2) - np.log(tau[:, None]) - 0.5 * np.log(2.0 * np.pi)


def _gl(n):
    return np.polynomial.legendre.leggauss(n)


def _composite(lo, hi, panels, f):
    """log of the integral of e^{f(x)} over [lo, hi] per row by `panels` panels of NODES Gauss-Legendre nodes, log-sum-exp."""
    g, wt = _gl(NODES)
    edges = lo[:, None] + (hi - lo)[:, None] * np.arange(panels + 1)[None, :] / panels
    c, r = 0.5 * (edges[:, 1:] + edges[:, :-1]), 0.5 * (edges[:, 1:] - edges[:, :-1])
    x = (c[:, :, None] + r[:, :, None] * g[None, None, :]).reshape(lo.size, -1)
    L = f(x) + np.log(np.broadcast_to((r[:, :, None] * wt[None, None, :]), (lo.size, panels, NODES)).reshape(lo.size, -1))
    M = L.max(1)
    return M + np.log(np.sum(np.exp(L - M[:, None]), 1))


def log_lik(p, y, z, t_censor):
    """The yardstick: float64 log L per row, p [n, 8], y [n], z [n] (one trial per row).  A response at or below ter gives -inf."""
    p, y, z = np.asarray(p, np.float64), np.asarray(y, np.float64), np.asarray(z, np.float64)
    t, code = trial_parts(p, y, t_censor)
    out = np.full(y.shape, -np.inf)
    keep = t > 0
    if not np.any(keep):
        return out
    p, t, code, z = p[keep], t[keep], code[keep], z[keep]
    m, tau, outside = gaussian_parts(p, z)
    f = lambda x: _integrand(x, p, t, code, m, tau)
    lo, hi = np.full(t.shape, np.log(1e-6)), np.log(np.maximum(m, 0.0) + 40.0 * tau + 1e3 * p[:, 5] * (1.0 + np.sqrt(t) + np.abs(p[:, 0] / p[:, 5]) * t))
    for _ in range(2):                                                  # two scans: the band of the second is the integration window
        x = lo[:, None] + (hi - lo)[:, None] * np.arange(SCAN)[None, :] / (SCAN - 1.0)
        L = f(x)
        inb = L >= L.max(1)[:, None] - 1.5 * BAND
        first, last = np.argmax(inb, 1), SCAN - 1 - np.argmax(inb[:, ::-1], 1)
        rows = np.arange(t.size)
        lo, hi = x[rows, np.maximum(first - 2, 0)], x[rows, np.minimum(last + 2, SCAN - 1)]
    I1, I2 = _composite(lo, hi, PANELS, f), _composite(lo, hi, 2 * PANELS, f)
    bad = ~(np.abs(I1 - I2) < CONVERGED)
    assert not np.any(bad), f"the yardstick's rule has not converged on rows {np.flatnonzero(bad)[:8]}: {np.abs(I1 - I2)[bad][:8]}"
    out[keep] = outside + I2
    return out


def scheme_window(p, t, code, m, tau):
    """The shipped pass-1 window in a: the hull of h's own support and the Gaussian's."""
    drift, mu, beta, ter, sd, dc, s1, g = columns(p)
    vp = drift / dc
    st = np.sqrt(t)
    c_lo = dc * np.pi * np.sqrt(t / (2.0 * C_CUT))
    w = np.where(code > 0, 1.0 - beta, beta)
    nu = np.where(code > 0, -vp, vp)
    c_hi_resp = dc * (np.maximum(-nu * t, 0.0) + np.sqrt(2.0 * C_CUT * t)) / w
    c_hi_cens = dc * np.maximum((vp * t + S_SIGMAS * st) / (1.0 - beta), (-vp * t + S_SIGMAS * st) / beta)
    mp = np.maximum(m, 0.0)
    hi = np.where(code == 0, np.maximum(mp, c_hi_cens) + L_TAU * tau, np.maximum(c_hi_resp, mp + L_TAU * tau))
    # the lower end: h rises as e^{-pi^2 t / (2 a'^2)} there, so a cut q is good when some r > q has the product e^{C} larger.  r = c_lo, with
    # what the Gaussian (E) and the drift term (D) can give back between q and r added to the exponent; or the Gaussian's own end where its
    # centre lies in h's rising part (m <= c_lo)
    below = m <= c_lo
    E = np.where(below, ((c_lo - m) ** 2 - np.minimum(m, 0.0) ** 2) / (2.0 * tau * tau), 0.0)
    D = (c_lo / dc) * np.abs(vp)
    lo = c_lo * np.sqrt(C_CUT / (2.0 * C_CUT + E + D))
    lo = np.where(below, np.maximum(lo, m - L_TAU * tau), lo)
    return lo, hi


def scheme_log_lik(p, y, z, t_censor):
    """The shipped scheme in float64 (module docstring)."""
    p, y, z = np.asarray(p, np.float64), np.asarray(y, np.float64), np.asarray(z, np.float64)
    t, code = trial_parts(p, y, t_censor)
    dead = ~(t > 0)
    t = np.where(dead, 1e-30, t)
    m, tau, outside = gaussian_parts(p, z)
    lo, hi = scheme_window(p, t, code, m, tau)
    xl, xh = np.log(lo), np.log(hi)
    g, wt = _gl(K_NODES)
    rows = np.arange(t.size)
    for ps in range(PASSES):
        xc, xr = 0.5 * (xh + xl), 0.5 * (xh - xl)
        x = xc[:, None] + xr[:, None] * g[None, :]
        L = _integrand(x, p, t, code, m, tau)
        M = L.max(1)
        if ps == PASSES - 1:
            break
        inb = L >= M[:, None] - ZOOM_BAND
        first, last = np.argmax(inb, 1), K_NODES - 1 - np.argmax(inb[:, ::-1], 1)
        nxl = np.where(first == 0, xl, x[rows, np.maximum(first - 1, 0)])
        nxh = np.where(last == K_NODES - 1, xh, x[rows, np.minimum(last + 1, K_NODES - 1)])
        xl, xh = nxl, nxh
    out = outside + M + np.log(np.sum(wt[None, :] * np.exp(L - M[:, None]), 1)) + np.log(xr)
    return np.where(dead, -np.inf, out)


# ---------------------------------------------------------------------------------------------------------------------------------------
# row sets: (float32 params [n, 8], float32 y [n], float32 z [n], t_censor)

PRIOR_T_CENSOR = 4.0
BOX_T_CENSOR = 2.0


def _simulate(p, rng, dt=1e-3, cap=PRIOR_T_CENSOR):
    """One trial per row by Euler-Maruyama at 1 ms in NumPy: (choicert, z1); a path that has not ended at the cap is a timeout (0)."""
    drift, mu, beta, ter, sd, dc, s1, g = columns(p)
    n = drift.size
    a = rng.normal(mu, sd)
    for _ in range(200):
        redo = ~(a > 0)
        if not np.any(redo):
            break
        a[redo] = rng.normal(mu[redo], sd[redo])
    assert np.all(a > 0)
    x = beta * a
    done = np.zeros(n, bool)
    y = np.zeros(n)
    sq = np.sqrt(dt)
    for k in range(1, int(round(cap / dt)) + 1):
        x = x + drift * dt + dc * sq * rng.standard_normal(n)
        up, lw = ~done & (x >= a), ~done & (x <= 0)
        y[up] = ter[up] + k * dt
        y[lw] = -(ter[lw] + k * dt)
        done |= up | lw
    z = rng.normal(g * a, s1)
    return y, z


POOL = 1500               # rows each set is drawn with, whatever n is asked for: the first n of them are the same rows for every n


@functools.lru_cache(maxsize=None)
def _prior_pool(seed):
    from bayesflow_nddms_amd import priors
    rows = priors.single_prior_matrix(POOL + POOL // 10 + 64, seed=seed)
    rows = rows[(rows[:, 5] >= 0.05) & (rows[:, 4] >= 0.02) & (rows[:, 6] >= 0.02)]
    assert rows.shape[0] >= POOL
    p32 = rows[:POOL]
    y, z = _simulate(p32.astype(np.float64), np.random.default_rng(seed + 1))
    return p32, y.astype(np.float32), z.astype(np.float32)


def prior_rows(n, seed=13):
    """The model's prior (priors.single_prior_matrix, gamma = 1) with dc >= 0.05, std_alpha >= 0.02 and sigma1 >= 0.02, the first n <= POOL
    such rows, each with one trial simulated from its own parameters; timeouts at the 4 s cap are kept as censored trials."""
    assert n <= POOL
    p32, y, z = _prior_pool(seed)
    return p32[:n], y[:n], z[:n], PRIOR_T_CENSOR


def _box_trials(pd, rng, censored=0.25):
    """The box's rule for one trial per row of float64 parameters pd: (y, z)."""
    n = pd.shape[0]
    z = pd[:, 7] * pd[:, 1] + rng.uniform(-4, 4, n) * np.sqrt(pd[:, 6] ** 2 + pd[:, 7] ** 2 * pd[:, 4] ** 2)
    t = np.exp(rng.uniform(np.log(0.02), np.log(3.0), n))
    sign = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    y = np.where(rng.random(n) < censored, 0.0, sign * (pd[:, 3] + t))
    return y, z


@functools.lru_cache(maxsize=None)
def _box_pool(seed):
    n = POOL
    rng = np.random.default_rng(seed)
    drift, mu, beta, ter = rng.uniform(-4, 4, n), rng.uniform(0.5, 2.5, n), rng.uniform(0.1, 0.9, n), rng.uniform(0.1, 0.5, n)
    sd, dc = rng.uniform(0.05, 1.0, n), rng.uniform(0.5, 1.5, n)
    s1 = np.where(rng.random(n) < 1.0 / 3.0, rng.uniform(0.02, 0.2, n), rng.uniform(0.2, 3.0, n))
    g = rng.choice([0.5, 1.0, 2.0], n)
    p32 = np.stack([drift, mu, beta, ter, sd, dc, s1, g], 1).astype(np.float32)
    y, z = _box_trials(p32.astype(np.float64), rng)
    return p32, y.astype(np.float32), z.astype(np.float32)


def box(n, seed=17):
    """Data that do NOT come from the row's own parameters, the first n <= POOL rows: drift in [-4, 4], mu_alpha in [0.5, 2.5], beta in [0.1,
    0.9], ter in [0.1, 0.5], std_alpha in [0.05, 1], dc in [0.5, 1.5]; z within +-4 marginal standard deviations of gamma mu, gamma in {0.5,
    1, 2}, a third of the rows with sigma1 in [0.02, 0.2] (the rest up to 3), decision times log-uniform in [0.02, 3] s on either
    boundary, a quarter of the trials censored at 2 s."""
    assert n <= POOL
    p32, y, z = _box_pool(seed)
    return p32[:n], y[:n], z[:n], BOX_T_CENSOR


SETS = {"prior_rows": prior_rows, "box": box}


def more_trials(name, p32, K, seed=23):
    """K further trials per row of p32, drawn as the set `name` draws its one: float32 (y [R, K], z [R, K])."""
    pd = np.repeat(p32.astype(np.float64), K, 0)
    rng = np.random.default_rng(seed)
    y, z = _simulate(pd, rng) if name == "prior_rows" else _box_trials(pd, rng)
    return y.astype(np.float32).reshape(-1, K), z.astype(np.float32).reshape(-1, K)


def pairs_log_lik(p32, y32, z32, t_censor):
    """The yardstick on every (row, trial) pair: p32 [R, 8], y32 / z32 [R, K] -> float64 [R, K]."""
    R, K = y32.shape
    p, y, z = as_f64(np.repeat(p32, K, 0), y32.reshape(-1), z32.reshape(-1))
    return log_lik(p, y, z, t_censor).reshape(R, K)


def as_f64(p32, y32, z32):
    """The float32 inputs as the kernel reads them, in float64; the decision time is the kernel's float32 |y| - ter."""
    p = p32.astype(np.float64)
    t32 = (np.abs(y32) - p32[:, 3]).astype(np.float32)
    y = np.sign(y32.astype(np.float64)) * (t32.astype(np.float64) + p[:, 3])
    return p, y, z32.astype(np.float64)
