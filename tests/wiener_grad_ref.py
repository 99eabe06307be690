"""Float64 yardstick of the GRADIENT of the Wiener first-passage log density: analytic derivatives of wiener_ref.log_f with respect to
each model's parameter columns, from the many-term series (wiener_ref.SMALL_TERMS / LARGE_TERMS), and the per-column condition scale
scale_j = sum over trials |per-trial d/dtheta_j log f| that errors of a row's gradient are measured against.  Test infrastructure only:
nothing in the product imports it.  tests/test_wiener_grad_host.py pins it against finite differences of wiener_ref.log_f.

Conventions are wiener_ref's (csrc/nddm_wiener.h): the lower boundary takes (v', w = beta), the upper one (-v', 1 - beta); a' = a/s,
v' = v/s, eta' = eta/s; t = rt - tau, u = t / a'^2.  Written as the quotient rule gives them, term by term, NOT in the simplified form
the header evaluates (csrc/nddm_wiener_grad.h), so that the two are independent restatements.
"""
import numpy as np

import wiener_ref as W

# The accuracy bar of a float32 gradient, per column, in units of scale_j: 4 x the largest error of the header's own code compiled for the
# host over the priors' rows (0.0152; tools/wiener_grad_host.py, profiles/r12_wiener_grad_host.json), rounded up to one significant digit.
# The factor covers the hardware transcendentals' last ulp.
BAR_B = 0.07
NU_CLIP = 5.0             # alpha_not_scaled's Nu is clipped to +-5 (wiener_row)
COLUMNS = {True: ("v", "a", "beta", "tau", "s"), False: ("Nu", "Alpha", "Beta", "Tau", "Eta", "Varsigma")}


def dlog_g_small(u, w, K=W.SMALL_TERMS):
    """(d/du, d/dw) of wiener_ref.log_g_small."""
    u, w = np.broadcast_arrays(np.asarray(u, np.float64), np.asarray(w, np.float64))
    k = np.arange(-K, K + 1, dtype=np.float64).reshape((-1,) + (1,) * u.ndim)
    x = w + 2.0 * k
    e = np.exp(-(x * x - w * w) / (2.0 * u))
    s1 = np.sum(x * e, axis=0)
    return -1.5 / u + np.sum(x ** 3 * e, axis=0) / (2.0 * u * u * s1), np.sum((1.0 - x * x / u) * e, axis=0) / s1


def dlog_g_large(u, w, K=W.LARGE_TERMS):
    """(d/du, d/dw) of wiener_ref.log_g_large."""
    u, w = np.broadcast_arrays(np.asarray(u, np.float64), np.asarray(w, np.float64))
    k = np.arange(1, K + 1, dtype=np.float64).reshape((-1,) + (1,) * u.ndim)
    e = np.exp(-(k * k - 1.0) * np.pi ** 2 * u / 2.0)
    s1 = np.sum(k * np.sin(k * np.pi * w) * e, axis=0)
    return (-np.pi ** 2 / 2.0 * np.sum(k ** 3 * np.sin(k * np.pi * w) * e, axis=0) / s1,
            np.pi * np.sum(k * k * np.cos(k * np.pi * w) * e, axis=0) / s1)


def dlog_g(u, w):
    """(d/du, d/dw) of wiener_ref.log_g, each series where wiener_ref sums it."""
    u, w = (np.array(x) for x in np.broadcast_arrays(np.asarray(u, np.float64), np.asarray(w, np.float64)))
    small = u < 1.0
    gu, gw = np.empty(u.shape), np.empty(u.shape)
    if np.any(small):
        gu[small], gw[small] = dlog_g_small(u[small], w[small])
    if np.any(~small):
        gu[~small], gw[~small] = dlog_g_large(u[~small], w[~small])
    return gu, gw


def dlog_g_fixed_trip(u, w, u_star=W.U_STAR):
    """The header's scheme in float64: 5 small-time terms below u_star, 3 large-time terms at and above."""
    u, w = np.broadcast_arrays(np.asarray(u, np.float64), np.asarray(w, np.float64))
    with np.errstate(all="ignore"):
        su, sw = dlog_g_small(u, w, K=2)
        lu, lw = dlog_g_large(u, w, K=3)
    return np.where(u < u_star, su, lu), np.where(u < u_star, sw, lw)


def natural(t, a, v, w, eta, dg=dlog_g):
    """Partials of wiener_ref.log_f_lower(t, a, v, w, eta) in (t, a, v, w, eta): five arrays."""
    t, a, v, w, eta = np.broadcast_arrays(*(np.asarray(x, np.float64) for x in (t, a, v, w, eta)))
    gu, gw = dg(t / (a * a), w)
    e2 = eta * eta
    D = 1.0 + e2 * t
    N = e2 * a * a * w * w - 2.0 * a * v * w - v * v * t                # drift = N / (2D) - 1/2 log D
    d_t = gu / (a * a) + (-v * v) / (2.0 * D) - N * e2 / (2.0 * D * D) - e2 / (2.0 * D)
    d_a = gu * (-2.0 * t / a ** 3) - 2.0 / a + (2.0 * e2 * a * w * w - 2.0 * v * w) / (2.0 * D)
    d_v = (-2.0 * a * w - 2.0 * v * t) / (2.0 * D)
    d_w = gw + (2.0 * e2 * a * a * w - 2.0 * a * v) / (2.0 * D)
    d_eta = (2.0 * eta * a * a * w * w) / (2.0 * D) - N * (2.0 * eta * t) / (2.0 * D * D) - eta * t / D
    return d_t, d_a, d_v, d_w, d_eta


def trial_grad(basic, p, t, upper, dg=dlog_g):
    """Per-trial gradient of log f in the model's parameter columns: p [..., P] float64 (basic: v, a, beta, tau, s; else Nu, Alpha, Beta,
    Tau, Eta, Varsigma), t = rt - tau and `upper` broadcasting against p[..., 0] -> [..., P]."""
    p = np.asarray(p, np.float64)
    v, a, beta, s = p[..., 0], p[..., 1], p[..., 2], p[..., 4 if basic else 5]
    eta = np.zeros_like(v) if basic else p[..., 4]
    clipped = np.zeros(v.shape, bool) if basic else np.abs(v) > NU_CLIP
    v = v if basic else np.clip(v, -NU_CLIP, NU_CLIP)
    upper = np.asarray(upper, bool)
    sg = np.where(upper, -1.0, 1.0)
    ap, vp, ep = a / s, v / s, eta / s
    d_t, d_a, d_v, d_w, d_eta = natural(t, ap, sg * vp, np.where(upper, 1.0 - beta, beta), ep, dg)
    d_v, d_w = sg * d_v, sg * d_w                                       # in (v', beta)
    d_s = -(ap * d_a + vp * d_v + ep * d_eta) / s
    cols = [np.where(clipped, 0.0, d_v / s), d_a / s, d_w, -d_t] + ([d_s] if basic else [d_eta / s, d_s])
    return np.stack(np.broadcast_arrays(*cols), -1)


def row_grad(basic, p, t, upper, dg=dlog_g):
    """A row's gradient and its condition scale: p [R, P], t and upper [R, N] -> (grad [R, P], scale [R, P]), the sum over the row's trials
    of the per-trial gradients and of their absolute values."""
    g = trial_grad(basic, np.asarray(p, np.float64)[:, None, :], t, upper, dg)
    return g.sum(1), np.abs(g).sum(1)


def log_f_of_params(basic, p, rt, upper):
    """wiener_ref.log_f as a function of the model's parameter columns and the response time (what finite differences are taken of)."""
    p = np.asarray(p, np.float64)
    v = p[..., 0] if basic else np.clip(p[..., 0], -NU_CLIP, NU_CLIP)
    return W.log_f(rt - p[..., 3], upper, p[..., 1], v, p[..., 2], p[..., 4 if basic else 5], 0.0 if basic else p[..., 4])
