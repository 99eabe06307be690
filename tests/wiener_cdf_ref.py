"""Float64 yardstick of the Wiener first-passage DISTRIBUTION function, P(T <= t, boundary), written from the published formulas:
the large-time eigenfunction series and the small-time series of Gondan, Blurton & Kesselmeier (2014), with the drift ~ N(nu, eta^2)
integrated out (Blurton, Kesselmeier & Gondan 2017 for the small-time form).  Test infrastructure only: nothing in the product imports it.

Conventions are those of tests/wiener_ref.py (csrc/nddm_wiener.h): the lower boundary takes (v', w = beta), the upper one (-v', 1 - beta);
a' = a/s, v' = v/s, eta' = eta/s; t = rt - tau, u = t / a'^2.  Below a, v, eta are the scaled ones, D = 1 + eta^2 t and
    d(t) = (eta^2 a^2 w^2 - 2 a v w - v^2 t) / (2 D)            (the density's drift exponent; -v a w - v^2 t / 2 at eta = 0).

Small time.  Every product of the published eta = 0 form, e^{-vaw - v^2 t/2} phi(r/sqrt t) M((r -+ vt)/sqrt t), is an exponential times
an erfc, 1/2 e^{-v (aw +- r)} erfc((r -+ vt) / sqrt(2t)), and its expectation over v ~ N(nu, eta^2) is again one (complete the square;
E Phi(p + qV) = Phi((p + q m) / sqrt(1 + q^2 eta^2))):
    1/2 e^{E} erfc(x),   A: c = aw + r, x = (r - t (v - c eta^2)) / sqrt(2 t D)      E = -c v + c^2 eta^2 / 2
                         B: c = aw - r, x = (r + t (v - c eta^2)) / sqrt(2 t D)
with E - x^2 = d(t) - r^2 / (2t) for both, so each is 1/2 e^{d - r^2/(2t)} erfcx(x) (x < 0: e^{E} - 1/2 e^{d - r^2/(2t)} erfcx(-x), E <= 0
there) and nothing overflows.  No quadrature.

Large time.  e^{-vaw - v^2 t/2} N(v; nu, eta^2) = D^{-1/2} e^{d(t)} N(v; mu_t, s_t^2), mu_t = (nu - a w eta^2) / D, s_t^2 = eta^2 / D, so
    F(t) = P_lo - (2 pi / a^2) D^{-1/2} e^{d(t)} sum_k k sin(k pi w) e^{-k^2 pi^2 t / (2a^2)} E_{v ~ N(mu_t, s_t^2)} [1 / (v^2 + k^2 pi^2 / a^2)]
and the expectation is taken by Gauss-Hermite quadrature on nodes mu_t + s_t z_i.  The integrand's poles lie k pi / a from the real
axis and s_t <= 1 / sqrt(t): at u >= 0.375 the Gaussian is at most 0.52 pole distances wide, where the rule converges geometrically
(a rule on the PRIOR N(nu, eta^2) instead, up to eta a / pi = 2.4 pole distances wide, is off by 1e-4 at 96 nodes).
P_lo with eta > 0 has no closed form; it is F_small(t1) + (P_lo - F_large)(t1) at the switch point t1, where both forms hold.
"""
import numpy as np
from scipy.special import erfcx

import wiener_ref as W  # noqa: F401  (the density's yardstick: same conventions; the tests integrate it)

SMALL_TERMS = 30          # j = 0..30 of the small-time series
LARGE_TERMS = 300         # k = 1..300 of the large-time series
U_SWITCH = 1.0            # small-time series below, large-time at and above
NODES = 96                # Gauss-Hermite nodes of the large-time form's expectation over the drift


def p_lower(a, v, w):
    """P(lower boundary) at a fixed drift v: (1 - e^{-2va(1-w)}) / (e^{2vaw} - e^{-2va(1-w)}), the exponents kept negative; 1 - w at v = 0."""
    a, v, w = np.broadcast_arrays(*(np.asarray(x, np.float64) for x in (a, v, w)))
    m = 2.0 * np.abs(v) * a
    tiny = m < 1e-12
    ms = np.where(tiny, 1.0, m)
    with np.errstate(all="ignore"):
        r = np.expm1(-ms * (1.0 - w)) / np.expm1(-ms)
        pos = np.exp(-ms * w) * r
    return np.where(tiny, 1.0 - w, np.where(v > 0, pos, r))


def _drift_exponent(t, a, v, w, eta):
    D = 1.0 + eta * eta * t
    return (eta * eta * a * a * w * w - 2.0 * a * v * w - v * v * t) / (2.0 * D), D


def small_time(t, a, v, w, eta, J=SMALL_TERMS):
    """sum_{j<=J} (-1)^j (A_j + B_j), closed form in eta (module docstring); arrays of one shape, t > 0."""
    d, D = _drift_exponent(t, a, v, w, eta)
    e2 = eta * eta
    rs = 1.0 / np.sqrt(2.0 * t * D)
    out = np.zeros(t.shape)
    for j in range(J + 1):
        r = a * (j + w) if j % 2 == 0 else a * (j + 1.0 - w)
        with np.errstate(over="ignore"):
            eg = np.exp(0.5 * (d - r * r / (2.0 * t)))                  # e^{G/2}: e^{G} erfcx(x) <= 2 although e^{G} may be large
            term = np.zeros(t.shape)
            for c, sg in ((a * w + r, 1.0), (a * w - r, -1.0)):
                x = (r - sg * t * (v - c * e2)) * rs
                E = np.where(x < 0, -c * v + 0.5 * c * c * e2, -np.inf)
                term += np.where(x < 0, -1.0, 1.0) * (eg * (eg * erfcx(np.abs(x)))) + 2.0 * np.exp(E)
        if not np.any(term):                                            # every later term is exactly 0 as well
            break
        out += (0.5 if j % 2 == 0 else -0.5) * term
    return out


def _nodes(n):
    x, wt = np.polynomial.hermite.hermgauss(n)
    return np.sqrt(2.0) * x, wt / np.sqrt(np.pi)                        # of N(0, 1)


def large_time_tail(t, a, v, w, eta, K=LARGE_TERMS, nodes=NODES):
    """P_lo - F(t) = P(T > t, lower boundary): the series above; arrays of one shape, t > 0.  eta = 0 rows: the nodes all sit on v."""
    d, D = _drift_exponent(t, a, v, w, eta)
    z, wt = _nodes(nodes)
    vi = ((v - a * w * eta * eta) / D)[..., None] + (eta / np.sqrt(D))[..., None] * z
    out = np.zeros(t.shape)
    for k in range(1, K + 1):
        kk = (k * np.pi / a) ** 2
        term = k * np.sin(k * np.pi * w) * np.exp(d - 0.5 * kk * t) * ((1.0 / (vi * vi + kk[..., None])) @ wt)
        if k > 1 and not np.any(term):
            break
        out += term
    return 2.0 * np.pi / (a * a) / np.sqrt(D) * out


def P_lower(a, v, w, eta=0.0, J=SMALL_TERMS, K=LARGE_TERMS, u_switch=U_SWITCH, nodes=NODES):
    """P(lower boundary), drift ~ N(v, eta^2), scaled parameters: closed form at eta = 0, else both series at the switch point."""
    a, v, w, eta = (np.array(x, np.float64) for x in np.broadcast_arrays(a, v, w, eta))
    t1 = u_switch * a * a
    return np.where(eta > 0, small_time(t1, a, v, w, eta, J) + large_time_tail(t1, a, v, w, eta, K, nodes), p_lower(a, v, w))


def F_lower(t, a, v, w, eta=0.0, J=SMALL_TERMS, K=LARGE_TERMS, u_switch=U_SWITCH, nodes=NODES):
    """P(T <= t, lower boundary), drift ~ N(v, eta^2) (scaled parameters); 0 for t <= 0."""
    t, a, v, w, eta = (np.array(x, np.float64) for x in np.broadcast_arrays(t, a, v, w, eta))
    out = np.zeros(t.shape)
    small = (t > 0) & (t < u_switch * a * a)
    large = (t > 0) & ~small
    if np.any(small):
        out[small] = small_time(t[small], a[small], v[small], w[small], eta[small], J)
    if np.any(large):
        sel = lambda x: x[large]
        out[large] = P_lower(sel(a), sel(v), sel(w), sel(eta), J, K, u_switch, nodes) - large_time_tail(sel(t), sel(a), sel(v), sel(w), sel(eta), K, nodes)
    return out


def cdf(t, upper, a, v, beta, s=1.0, eta=0.0, **scheme):
    """P(T <= t, the boundary named) in the model's natural parameters; `scheme`: J, K, u_switch, nodes of a truncated scheme."""
    a, v, beta, s, eta = (np.asarray(x, np.float64) for x in (a, v, beta, s, eta))
    ap, vp, ep = a / s, v / s, eta / s
    upper = np.asarray(upper, bool)
    return F_lower(t, ap, np.where(upper, -vp, vp), np.where(upper, 1.0 - beta, beta), ep, **scheme)


def p_upper(a, v, beta, s=1.0, eta=0.0, **scheme):
    """P(upper boundary) in the model's natural parameters, eta integrated."""
    a, v, beta, s, eta = (np.asarray(x, np.float64) for x in (a, v, beta, s, eta))
    return P_lower(a / s, -v / s, 1.0 - beta, eta / s, **scheme)


def signed_cdf(y, a, v, beta, tau, s=1.0, eta=0.0):
    """G(y) = P(signed RT <= y): P_lo - F_lo(-y - tau) for y < 0, P_lo + F_up(y - tau) for y > 0."""
    y = np.asarray(y, np.float64)
    p_lo = 1.0 - p_upper(a, v, beta, s, eta)
    return np.where(y < 0, p_lo - cdf(-y - tau, False, a, v, beta, s, eta), p_lo + cdf(y - tau, True, a, v, beta, s, eta))


# the scheme csrc/nddm_wiener_cdf.h evaluates (WCDF_SMALL_J, WCDF_LARGE_K, WIENER_U_STAR, WCDF_NODES), for float64 restatements
SHIPPED = dict(J=3, K=4, u_switch=0.375, nodes=16)


def accuracy_rows(n, basic=False, seed=11):
    """The rows of the accuracy tests, drawn as tests/test_gpu_wiener.py draws its pointwise rows: u in [1e-3, 50] log-uniform plus a
    quarter in [0.3, 0.5], nu in [-5, 5], a in [0.5, 2.5], beta in [0.02, 0.98], eta = 0 for 30 % and else U(0, 3), both boundaries;
    basic: s in [0.8, 1.3] and no eta.  -> (float32 params [n, P], float32 rt [n], upper [n] bool, float64 t = the kernel's float32
    rt - tau)."""
    rng = np.random.default_rng(seed)
    u = np.concatenate([np.exp(rng.uniform(np.log(1e-3), np.log(50.0), n - n // 4)), rng.uniform(0.3, 0.5, n // 4)])
    nu, a, beta, tau = rng.uniform(-5, 5, n), rng.uniform(0.5, 2.5, n), rng.uniform(0.02, 0.98, n), rng.uniform(0.0, 0.5, n)
    eta = np.where(rng.random(n) < 0.3, 0.0, rng.uniform(0, 3, n))
    up = rng.random(n) < 0.5
    if basic:
        s = rng.uniform(0.8, 1.3, n)
        p32 = np.stack([nu, a, beta, tau, s], 1).astype(np.float32)
    else:
        s = np.ones(n)
        p32 = np.stack([nu, a, beta, tau, eta, s], 1).astype(np.float32)
    ap = p32[:, 1].astype(np.float64) / p32[:, -1].astype(np.float64)
    rt32 = (p32[:, 3].astype(np.float64) + u * ap ** 2).astype(np.float32)
    t = (rt32 - p32[:, 3]).astype(np.float32).astype(np.float64)
    return p32, rt32, up, t


def _basic_prior_rows(n, seed, dc_min=0.05):
    """The first n rows of priors.basic_prior_matrix(seed) with dc >= dc_min (99.5 % of the draws; a / dc up to 28-39 and |v| / dc up to
    80-96 on 20 000 of them, by the seed).  Below it the quotients grow without bound: DESIGN section 10."""
    from bayesflow_nddms_amd import priors
    rows = priors.basic_prior_matrix(n + n // 20 + 64, seed=seed)
    rows = rows[rows[:, 4] >= dc_min]
    assert rows.shape[0] >= n
    return rows[:n]


def prior_rows(n, basic=False, seed=11):
    """accuracy_rows on the parameters the two models draw, with the same draw of u and of the boundary.  basic: rows of
    priors.basic_prior_matrix with dc >= 0.05.  alpha_not_scaled: the first half rows of priors.alpha_ns_prior_matrix (Varsigma in
    [0.8, 1.4], Eta in [0, 2]), the second half accuracy_rows' box with Varsigma ~ U(0.5, 2.0) in place of 1.  Returns what
    accuracy_rows returns."""
    from bayesflow_nddms_amd import priors
    rng = np.random.default_rng(seed)
    u = np.concatenate([np.exp(rng.uniform(np.log(1e-3), np.log(50.0), n - n // 4)), rng.uniform(0.3, 0.5, n // 4)])
    up = rng.random(n) < 0.5
    if basic:
        p32 = _basic_prior_rows(n, seed)
    else:
        h = n // 2
        m = n - h
        nu, a, beta, tau = rng.uniform(-5, 5, m), rng.uniform(0.5, 2.5, m), rng.uniform(0.02, 0.98, m), rng.uniform(0.0, 0.5, m)
        eta = np.where(rng.random(m) < 0.3, 0.0, rng.uniform(0, 3, m))
        box = np.stack([nu, a, beta, tau, eta, rng.uniform(0.5, 2.0, m)], 1).astype(np.float32)
        p32 = np.concatenate([priors.alpha_ns_prior_matrix(h, seed=seed), box])
        rng.shuffle(u)                                                  # (the quarter in [0.3, 0.5] falls on both halves)
    ap = p32[:, 1].astype(np.float64) / p32[:, -1].astype(np.float64)
    rt32 = (p32[:, 3].astype(np.float64) + u * ap ** 2).astype(np.float32)
    t = (rt32 - p32[:, 3]).astype(np.float32).astype(np.float64)
    return p32, rt32, up, t


S_FLOOR = 1e-3            # log_survival is the yardstick where S >= S_FLOOR; below it, wiener_ref.mp_log_survival (tests/golden/wiener_survival.npz)


def log_survival(t, a, v, beta, s=1.0):
    """log P(T > t) of the eta = 0 process as log1p(-(F_lower + F_upper)) of the distribution function above, which does not cancel at
    small u as the survival series does: -> (log S, ok), ok where S >= S_FLOOR (float64 keeps 12 digits of S there); NaN elsewhere.
    t <= 0 gives 0."""
    t, a, v, beta, s = (np.array(x, np.float64) for x in np.broadcast_arrays(t, a, v, beta, s))
    F = cdf(t, False, a, v, beta, s) + cdf(t, True, a, v, beta, s)
    ok = 1.0 - F >= S_FLOOR
    with np.errstate(all="ignore"):
        return np.where(ok, np.log1p(-np.where(ok, F, 0.0)), np.nan), ok


CENSOR_TIMES = 16         # increasing times per row of the censoring tests


def _times(p32, t):
    """float32 rt = tau + t [R, m] and the kernel's t = rt - tau in float32, as float64."""
    rt32 = (p32[:, 3:4].astype(np.float64) + t).astype(np.float32)
    return rt32, (rt32 - p32[:, 3:4]).astype(np.float32).astype(np.float64)


def censor_sets(n_prior=5000, n_box=2000, seed=5, with_fixture=True):
    """The rows of the censoring tests, basic_ddm_dc, CENSOR_TIMES increasing times each: name -> (float32 params [R, 5], float32 rt
    [R, 16], float64 t = the kernel's float32 rt - tau).  `prior_1s` / `prior_4s`: prior_rows' basic rows at k / 16 of a 1 s and a 4 s
    horizon (dt .01 x 100 and x 400 steps); `box`: the shipped tests' box (nu +-5, a .5-2.5, beta .02-.98, tau 0-.5, dc .8-1.3) at 16 sorted
    draws of u log-uniform in [1e-3, 50]; `fixture`: tests/golden/wiener_survival.npz's own rows."""
    rows = _basic_prior_rows(n_prior, seed)
    k = np.arange(1, CENSOR_TIMES + 1, dtype=np.float64)[None, :] / CENSOR_TIMES
    out = {"prior_1s": (rows,) + _times(rows, 1.0 * k + 0.0 * rows[:, :1]), "prior_4s": (rows,) + _times(rows, 4.0 * k + 0.0 * rows[:, :1])}
    rng = np.random.default_rng(seed + 1)
    box = np.stack([rng.uniform(-5, 5, n_box), rng.uniform(0.5, 2.5, n_box), rng.uniform(0.02, 0.98, n_box), rng.uniform(0.0, 0.5, n_box),
                    rng.uniform(0.8, 1.3, n_box)], 1).astype(np.float32)
    u = np.sort(np.exp(rng.uniform(np.log(1e-3), np.log(50.0), (n_box, CENSOR_TIMES))), axis=1)
    ap = box[:, 1].astype(np.float64) / box[:, 4].astype(np.float64)
    out["box"] = (box,) + _times(box, u * ap[:, None] ** 2)
    if with_fixture:
        import os
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wiener_survival.npz"))
        out["fixture"] = (g["params"], g["rt"], (g["rt"] - g["params"][:, 3:4]).astype(np.float32).astype(np.float64))
    return out


# the four rows of the censoring defect's report (drift, a, beta, tau, dc) and their decision times: the float32 large-time series gave
# NaN, +9.3, +15.7 and -0.16 for log S = -0.000000, -2.507289, -0.009398 and -6.160853
REPORTED_ROWS = np.array([[0.5261412, 1.9813986, 0.4452605, 0.4539135, 0.1136013], [1.6254113, 1.6473216, 0.1531147, 0.3260034, 0.1724049],
                          [0.1823803, 1.2271703, 0.1858106, 0.4585065, 0.0559113], [0.2977207, 1.4949200, 0.4268077, 0.1464299, 0.0596928]], np.float32)
REPORTED_T = np.array([1.0, 1.0, 4.0, 4.0])
REPORTED_RT = np.array([1.4539136, 1.3260034, 4.4585066, 4.1464300], np.float32)
REPORTED_LOG_S = np.array([-0.000000, -2.507289, -0.009398, -6.160853])


def row_columns(p32, basic=False):
    """float64 (a, v, beta, tau, s, eta) of float32 parameter rows in either model's order."""
    p = p32.astype(np.float64)
    if basic:
        return p[:, 1], p[:, 0], p[:, 2], p[:, 3], p[:, 4], np.zeros(p.shape[0])
    return p[:, 1], p[:, 0], p[:, 2], p[:, 3], p[:, 5], p[:, 4]
