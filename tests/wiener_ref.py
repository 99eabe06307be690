"""Float64 yardstick of the Wiener first-passage density, written from the published formulas (Navarro & Fuss 2009 for the two
series of the standard density; Ratcliff 1978 / Blurton et al. 2017 for the drift ~ N(nu, eta^2) integrated out; the large-time
first-passage survival series of the same process).  Test infrastructure only: nothing in the product imports it.

Conventions are the library's (csrc/nddm_wiener.h): the evidence starts at beta*a and drifts toward the upper boundary; the lower
boundary takes (v', w = beta), the upper one (-v', 1 - beta); a' = a/s, v' = v/s, eta' = eta/s; t = rt - tau, u = t / a'^2.
"""
import numpy as np

SMALL_TERMS = 60          # k = -60..60 of the small-time series
LARGE_TERMS = 200         # k = 1..200 of the large-time series
U_STAR = 0.375            # the library's switch between its fixed-trip sums (WIENER_U_STAR)


def log_g_small(u, w, K=SMALL_TERMS):
    """log of (2 pi u^3)^-1/2 sum_{k=-K..K} (w + 2k) exp(-(w + 2k)^2 / (2u)), the k = 0 exponent taken out."""
    u, w = np.broadcast_arrays(np.asarray(u, np.float64), np.asarray(w, np.float64))
    k = np.arange(-K, K + 1, dtype=np.float64).reshape((-1,) + (1,) * u.ndim)
    x = w + 2.0 * k
    s = np.sum(x * np.exp(-(x * x - w * w) / (2.0 * u)), axis=0)
    return -0.5 * np.log(2.0 * np.pi * u ** 3) - w * w / (2.0 * u) + np.log(s)


def log_g_large(u, w, K=LARGE_TERMS):
    """log of pi sum_{k=1..K} k exp(-k^2 pi^2 u / 2) sin(k pi w), the k = 1 exponent taken out."""
    u, w = np.broadcast_arrays(np.asarray(u, np.float64), np.asarray(w, np.float64))
    k = np.arange(1, K + 1, dtype=np.float64).reshape((-1,) + (1,) * u.ndim)
    s = np.sum(k * np.exp(-(k * k - 1.0) * np.pi ** 2 * u / 2.0) * np.sin(k * np.pi * w), axis=0)
    return np.log(np.pi) - np.pi ** 2 * u / 2.0 + np.log(s)


def log_g(u, w):
    """The standard density from whichever full series is numerically safe in float64 at u (both converge everywhere)."""
    u, w = np.broadcast_arrays(np.asarray(u, np.float64), np.asarray(w, np.float64))
    small = u < 1.0
    out = np.empty(u.shape)
    if np.any(small):
        out[small] = log_g_small(u[small], w[small])
    if np.any(~small):
        out[~small] = log_g_large(u[~small], w[~small])
    return out


def log_g_fixed_trip(u, w, u_star=U_STAR):
    """The library's scheme in float64: 5 small-time terms (k = -2..2) below u_star, 3 large-time terms (k = 1..3) at and above."""
    u, w = np.broadcast_arrays(np.asarray(u, np.float64), np.asarray(w, np.float64))
    with np.errstate(all="ignore"):
        small = log_g_small(u, w, K=2)
        large = log_g_large(u, w, K=3)
    return np.where(u < u_star, small, large)


def log_f_lower(t, a, v, w, eta=0.0, lg=log_g):
    """log density of hitting the LOWER boundary at decision time t, scaled parameters (a', v', w, eta'), drift ~ N(v, eta^2)."""
    t, a, v, w, eta = (np.asarray(x, np.float64) for x in (t, a, v, w, eta))
    e2 = eta * eta
    drift = (e2 * a * a * w * w - 2.0 * a * v * w - v * v * t) / (2.0 * (1.0 + e2 * t)) - 0.5 * np.log1p(e2 * t)
    return lg(t / (a * a), w) - 2.0 * np.log(a) + drift


def log_f(t, upper, a, v, beta, s=1.0, eta=0.0, lg=log_g):
    """log density of decision time t on the upper (upper=True) or lower boundary in the model's natural parameters."""
    a, v, beta, s, eta = (np.asarray(x, np.float64) for x in (a, v, beta, s, eta))
    ap, vp, ep = a / s, v / s, eta / s
    upper = np.asarray(upper, bool)
    return np.where(upper, log_f_lower(t, ap, -vp, 1.0 - beta, ep, lg), log_f_lower(t, ap, vp, beta, ep, lg))


def p_upper(a, v, beta, s=1.0):
    """Probability of the upper boundary, eta = 0 (closed form)."""
    ap, vp = a / s, v / s
    if abs(vp) < 1e-12:
        return beta
    return np.expm1(-2.0 * vp * ap * beta) / np.expm1(-2.0 * vp * ap)


def survival(t, a, v, beta, s=1.0, K=LARGE_TERMS):
    """P(T > t) of the eta = 0 process over both boundaries: the large-time survival series
    sum_{sides} (pi / a'^2) e^{-a' v w} sum_k k sin(k pi w) e^{-lambda_k t} / lambda_k,  lambda_k = v'^2/2 + k^2 pi^2 / (2 a'^2)."""
    ap, vp = a / s, v / s
    k = np.arange(1, K + 1, dtype=np.float64)
    lam = vp * vp / 2.0 + k * k * np.pi ** 2 / (2.0 * ap * ap)
    tot = 0.0
    for w, nu in ((beta, vp), (1.0 - beta, -vp)):
        tot += np.pi / ap ** 2 * np.exp(-ap * nu * w) * np.sum(k * np.sin(k * np.pi * w) * np.exp(-lam * t) / lam)
    return tot


def log_survival(t, a, v, beta, s=1.0):
    """log P(T > t), the e^{-lambda_1 t} factor taken out so that long censoring times do not underflow.  The series only: in float64 its
    terms cancel once a'|v'|w exceeds about 36 at small u (inf or nan beyond), so it serves the wide-boundary rows of the priors no
    better than the kernel's float32 did.  The yardstick that is right there is wiener_cdf_ref.log_survival (1 - F_lower - F_upper where
    S >= 1e-3) and mp_log_survival below it."""
    ap, vp = a / s, v / s
    k = np.arange(1, LARGE_TERMS + 1, dtype=np.float64)
    lam = vp * vp / 2.0 + k * k * np.pi ** 2 / (2.0 * ap * ap)
    tot = 0.0
    for w, nu in ((beta, vp), (1.0 - beta, -vp)):
        tot += np.pi / ap ** 2 * np.exp(-ap * nu * w) * np.sum(k * np.sin(k * np.pi * w) * np.exp(-(lam - lam[0]) * t) / lam)
    return -lam[0] * t + np.log(tot)


def mp_g(u, w, small, K=400, dps=60):
    """Either series at high precision (mpmath): the spot checks at extreme arguments."""
    import mpmath as mp
    mp.mp.dps = dps
    u, w = mp.mpf(u), mp.mpf(w)
    if small:
        s = mp.fsum((w + 2 * k) * mp.exp(-(w + 2 * k) ** 2 / (2 * u)) for k in range(-K, K + 1))
        return mp.log(s / mp.sqrt(2 * mp.pi * u ** 3))
    s = mp.fsum(k * mp.exp(-k * k * mp.pi ** 2 * u / 2) * mp.sin(k * mp.pi * w) for k in range(1, K + 1))
    return mp.log(mp.pi * s)


def mp_log_survival(t, a, v, beta, s=1.0, extra_digits=30):
    """log P(T > t) from the large-time survival series at the precision the series needs (mpmath): its terms are up to e^{a'|v'|} large
    and must cancel down to S ~ e^{-a'|v'|w - v'^2 t / 2} and, at small u, to e^{-1/(2u)} of their size, so the working precision is
    sized by a'|v'| + v'^2 t / 2 + pi^2 u / 2 + 1 / (2u) (at a fixed 50 digits the sum comes out negative on the priors' rows), and the
    number of terms by e^{-k^2 pi^2 u / 2} falling below that precision."""
    import mpmath as mp
    ap, vp = float(a) / float(s), float(v) / float(s)
    u = float(t) / (ap * ap)
    need = ap * abs(vp) + vp * vp * float(t) / 2.0 + np.pi ** 2 * u / 2.0 + 1.0 / (2.0 * u)
    dps = int(extra_digits + need / np.log(10.0)) + 1
    K = int(np.sqrt(2.0 * dps * np.log(10.0) / (np.pi ** 2 * u))) + 10
    with mp.workdps(dps):
        t_, a_, v_, b_ = mp.mpf(float(t)), mp.mpf(float(a)) / mp.mpf(float(s)), mp.mpf(float(v)) / mp.mpf(float(s)), mp.mpf(float(beta))
        kk = mp.pi ** 2 / (2 * a_ * a_)
        tot = mp.mpf(0)
        for w, nu in ((b_, v_), (1 - b_, -v_)):
            tot += mp.exp(-a_ * nu * w) * mp.fsum(k * mp.sin(k * mp.pi * w) * mp.exp(-(nu * nu / 2 + k * k * kk) * t_) / (nu * nu / 2 + k * k * kk)
                                                  for k in range(1, K + 1))
        return float(mp.log(mp.pi / (a_ * a_) * tot))
