"""Float64 yardstick of the gradient of a basic_ddm_dc row that holds CENSORED TIMEOUTS (choice 0), NDDM_WIENER_CENSORED's quantity
(csrc/nddm_wiener_grad.h): a response contributes wiener_grad_ref.trial_grad, a timeout at rt the partials of
log S(rt - tau) = wiener_cdf_ref.log_survival in the model's columns (v, a, beta, tau, s).  Test infrastructure only: nothing in the
product imports it.  tests/test_wiener_censored_host.py pins it against central differences of log S.

A timeout's partials, not in the form the header evaluates:
    v, beta, s      wiener_marginal_grad_ref.dlog_survival: Richardson-extrapolated central differences of the float64 log S
    a               log S depends on (a / s, v / s, beta) alone, so a d/da + v d/dv + s d/ds = 0:  d/da = -(v d/dv + s d/ds) / a
    tau             t = rt - tau:  d/dtau = -d/dt log S = +(f_lower(t) + f_upper(t)) / S(t), from wiener_ref.log_f and the same log S
A timeout with t <= 0 is log 1 = 0 with a zero gradient.  `ok`: where wiener_cdf_ref.log_survival is the yardstick (S >= 1e-3).
The scale of a column is the sum over the row's trials, timeouts included, of |per-trial partial|.
"""
import json
import os

import numpy as np

import wiener_cdf_ref as C
import wiener_grad_ref as G
import wiener_marginal_grad_ref as MG
import wiener_marginal_ref as M
import wiener_ref as W

COLUMNS = G.COLUMNS[True]

# The accuracy bar of the float32 gradient of rows with timeouts, per column, in units of scale_j.  The header's own code compiled for the
# host (tools/wiener_grad_host.py --censored, profiles/r22_wiener_censored_host.json) over wiener_cdf_ref.censor_sets()'s prior_1s,
# prior_4s and box rows, 160 trials per row of which 16 (10 %) are timeouts at the set's times, measured 6.7e-7 of scale_j at the most
# (prior_1s, the beta column; prior_4s 6.7e-7, box 4.3e-7): below wiener_grad_ref.BAR_B, so by the rule the bar IS BAR_B (0.07), as for rows
# without timeouts.  The responses lend those rows most of their scale; the same rows' 16 timeouts ALONE (reported by the tool, not part
# of the rule) measured 3.5e-5 of their own scale at the most (prior_1s, the tau column).
HOST_MAX_ERR = 6.7e-7
BAR = G.BAR_B

TRIALS_PER_ROW = 160      # of the host survey's rows
CENSORED_PER_ROW = C.CENSOR_TIMES


def log_survival(p, t):
    """log S(t) of rows p [..., 5] (v, a, beta, tau, s) at decision times t broadcasting against p[..., 0]: (values, ok)."""
    p = np.asarray(p, np.float64)
    v, a, beta, s, t = (np.array(x, np.float64) for x in np.broadcast_arrays(p[..., 0], p[..., 1], p[..., 2], p[..., 4], t))
    pos = t > 0
    tt = np.where(pos, t, 1.0)
    ls = M._log_survival(tt, a, v, beta, s)
    _, ok = C.log_survival(tt, a, v, beta, s)
    return np.where(pos, ls, 0.0), ok | ~pos


def timeout_grad(p, t):
    """Per-timeout gradient of log S(t = rt - tau) in (v, a, beta, tau, s): p [..., 5], t broadcasting against p[..., 0] -> [..., 5]."""
    p = np.asarray(p, np.float64)
    v, a, beta, s, t = (np.array(x, np.float64) for x in np.broadcast_arrays(p[..., 0], p[..., 1], p[..., 2], p[..., 4], t))
    shape = t.shape
    v, a, beta, s, t = (x.reshape(-1) for x in (v, a, beta, s, t))
    pos = t > 0
    out = np.zeros(t.shape + (5,))
    if np.any(pos):
        vv, aa, bb, ss, tt = v[pos], a[pos], beta[pos], s[pos], t[pos]
        d_v, d_b, d_s = MG.dlog_survival(tt, aa, vv, bb, ss)
        d_a = -(vv * d_v + ss * d_s) / aa
        ls = M._log_survival(tt, aa, vv, bb, ss)
        with np.errstate(all="ignore"):
            d_tau = np.exp(W.log_f(tt, False, aa, vv, bb, ss) - ls) + np.exp(W.log_f(tt, True, aa, vv, bb, ss) - ls)
        out[pos] = np.stack([d_v, d_a, d_b, d_tau, d_s], -1)
    return out.reshape(shape + (5,))


def trial_grad(p, t, code):
    """Per-trial gradient: p [..., 5], t = rt - tau and code (1 upper, -1 lower, 0 a timeout) broadcasting against p[..., 0] -> [..., 5]."""
    p = np.asarray(p, np.float64)
    t, code = np.broadcast_arrays(np.asarray(t, np.float64), np.asarray(code, np.float64))
    cens = code == 0
    with np.errstate(all="ignore"):
        resp = G.trial_grad(True, p, np.where(cens, 1.0, t), code > 0)
    full = np.broadcast_shapes(resp.shape[:-1], t.shape)
    resp = np.broadcast_to(resp, full + (5,))
    cens = np.broadcast_to(cens, full)
    out = np.array(resp)
    if np.any(cens):
        pb = np.broadcast_to(p, full + (5,))
        out[cens] = timeout_grad(pb[cens], np.broadcast_to(t, full)[cens])
    return out


def row_grad(p, t, code):
    """A row's gradient and its condition scale: p [R, 5], t and code [R, N] -> (grad [R, 5], scale [R, 5])."""
    g = trial_grad(np.asarray(p, np.float64)[:, None, :], t, code)
    return g.sum(1), np.abs(g).sum(1)


def fd_timeout_grad(p, rt, rel=2e-3):
    """Richardson-extrapolated central differences of log S(rt - tau) in every column of p [n, 5] (what timeout_grad is pinned against);
    tau's step is scaled to the decision time."""
    p, rt = np.asarray(p, np.float64), np.asarray(rt, np.float64)
    f = lambda x: log_survival(x, rt - x[:, 3])[0]
    out = np.empty(p.shape)
    for j in range(5):
        scale = rt - p[:, 3] if j == 3 else np.maximum(np.abs(p[:, j]), p[:, 4] if j == 0 else 0.0)
        if j == 2:
            scale = np.minimum(p[:, 2], 1.0 - p[:, 2])

        def cd(step):
            hi, lo = p.copy(), p.copy()
            hi[:, j] += step
            lo[:, j] -= step
            return (f(hi) - f(lo)) / (2.0 * step)
        h = rel * scale
        out[:, j] = (4.0 * cd(0.5 * h) - cd(h)) / 3.0
    return out


def censored_rows(p32, rt_c32, seed=3, n=TRIALS_PER_ROW):
    """The host survey's and the tests' rows: to each row of a wiener_cdf_ref.censor_sets() set (p32 [R, 5], its 16 censoring times
    rt_c32 [R, 16]) n - 16 responses at u = t / a'^2 log-uniform in [0.02, 3] on either boundary, the timeouts spread among them (every
    tenth trial).  Where the yardstick's `ok` fails for a time of the row, that slot repeats one of the row's ok times (they are a prefix:
    S falls with t); rows with no ok time are left out.  -> (rows used [R'] indices, float32 data [R', n, 2], float64 t [R', n] = the
    kernel's float32 rt - tau, code [R', n])."""
    rng = np.random.default_rng(seed)
    R, m = rt_c32.shape
    p = p32.astype(np.float64)
    tc = (rt_c32 - p32[:, 3:4]).astype(np.float32).astype(np.float64)
    _, ok = log_survival(p[:, None, :], tc)
    k = ok.sum(1)
    rows = np.flatnonzero(k > 0)
    idx = np.arange(m)[None, :] % np.maximum(k, 1)[:, None]
    okt = np.where(ok, rt_c32, np.float32(np.inf))
    okt = np.sort(okt, 1)                                               # the ok times first
    rt_c = np.take_along_axis(okt, idx, 1)
    ap = p[:, 1] / p[:, 4]
    u = np.exp(rng.uniform(np.log(0.02), np.log(3.0), (R, n)))
    rt = (p[:, 3:4] + u * ap[:, None] ** 2).astype(np.float32)
    code = np.where(rng.random((R, n)) < 0.5, 1.0, -1.0)
    slots = np.arange(m) * (n // m) + (n // m) // 2
    rt[:, slots] = rt_c
    code[:, slots] = 0.0
    data = np.stack([rt, code], -1).astype(np.float32)[rows]
    t = (data[..., 0] - p32[rows, 3:4]).astype(np.float32).astype(np.float64)
    return rows, data, t, data[..., 1].astype(np.float64)


# ---- the sampler's statistics tests with timeouts (csrc/nddm_wiener_hmc.h under NDDM_WIENER_CENSORED) ---------------
# wiener_hmc_ref's two cases with timeouts added: Y20 + four timeouts at rt = 1.5 (drift, boundary free; beta .5, tau .2, dc 1 fixed), by
# grid quadrature, and Y10 + two timeouts at rt = 1.2 (all five free), by importance sampling from the prior -- the posterior's tau limit
# T = min(1.5, the smallest rt OF THE RESPONSES).  Recorded in tests/golden/wiener_censored_hmc_yardsticks.json (`python
# tests/wiener_censored_ref.py` writes it; tests/test_wiener_censored_hmc_host.py recomputes the grid and compares).
TIMEOUTS_2D = (1.5, 1.5, 1.5, 1.5)
TIMEOUTS_5D = (1.2, 1.2)


def with_timeouts(y, rt_c):
    """signed response times and censoring times -> float32 [N, 2] = (rt, choice), the timeouts (choice 0) last"""
    import wiener_hmc_ref as HR
    return np.concatenate([HR.as_data(y), np.stack([np.asarray(rt_c, np.float32), np.zeros(len(rt_c), np.float32)], 1)])


def censored_loglik(y, rt_c, v, a, beta, tau, s):
    """wiener_hmc_ref.loglik of the responses plus the sum over the timeouts of log S(rt_c - tau), parameters flat [M] -> [M]"""
    import wiener_hmc_ref as HR
    v, a, beta, tau, s = (np.array(x) for x in np.broadcast_arrays(*(np.asarray(x, np.float64) for x in (v, a, beta, tau, s))))
    out = HR.loglik(y, v, a, beta, tau, s)
    for rt in np.asarray(rt_c, np.float32).astype(np.float64):
        t = rt - tau
        pos = t > 0
        ls = np.zeros(t.shape)
        if pos.any():
            ls[pos] = M._log_survival(t[pos], a[pos], v[pos], beta[pos], s[pos])
        out = out + ls
    return out


def _grid_moments(n, rt_c):
    import wiener_hmc_ref as HR
    v = np.linspace(-6.0, 6.0, n)
    a = np.linspace(0.05, 5.0, n)
    V, A = np.meshgrid(v, a, indexing="ij")
    f = HR.FIXED_2D
    lp = -0.125 * V * V - 2.0 * (A - 1.0) ** 2 + censored_loglik(HR.Y20, rt_c, V.ravel(), A.ravel(), f["beta"], f["tau"], f["dc"]).reshape(V.shape)
    w = np.exp(lp - lp.max())
    w[[0, -1], :] *= 0.5
    w[:, [0, -1]] *= 0.5                                               # trapezoid rule
    w /= w.sum()
    m = np.array([(w * V).sum(), (w * A).sum()])
    sd = np.sqrt(np.array([(w * V * V).sum(), (w * A * A).sum()]) - m * m)
    return m, sd


def yardstick_2d(rt_c=TIMEOUTS_2D):
    """-> (mean [2], sd [2], the grid size, the last refinement's largest move in sd) for (drift, boundary) given Y20 and timeouts at rt_c"""
    n = 81
    m, sd = _grid_moments(n, rt_c)
    while True:
        n = 2 * n - 1
        m2, sd2 = _grid_moments(n, rt_c)
        move = float(max(np.max(np.abs(m2 - m) / sd2), np.max(np.abs(sd2 - sd) / sd2)))
        m, sd = m2, sd2
        if move < 1e-4:
            return m, sd, n, move
        assert n < 2000


def yardstick_5d(rt_c=TIMEOUTS_5D, block=400_000, need=20_000.0):
    """-> (mean [5], sd [5], the effective sample size, the draws) in (drift, boundary, beta, tau, dc) given Y10 and timeouts at rt_c"""
    import wiener_hmc_ref as HR
    rng = np.random.default_rng(78)
    T = min(1.5, float(np.min(np.abs(HR.as_data(HR.Y10)[:, 0]))))       # the responses alone
    th, lw = [], []
    while True:
        p = np.stack([rng.normal(0.0, 2.0, block), HR._truncnorm(rng, 1.0, 0.5, 0.0, 10.0, block), rng.beta(2.0, 2.0, block),
                      HR._truncnorm(rng, 0.5, 0.25, 0.0, T, block), HR._truncnorm(rng, 1.0, 0.5, HR.DC_MIN, 10.0, block)], 1)
        th.append(p)
        lw.append(censored_loglik(HR.Y10, rt_c, p[:, 0], p[:, 1], p[:, 2], p[:, 3], p[:, 4]))
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


RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wiener_censored_hmc_yardsticks.json")


def recorded():
    """The recorded yardsticks -> {'two': (mean, sd), 'two_without': (mean, sd) of Y20 alone, 'five': (mean, sd), 'five_ess', ...}"""
    with open(RECORD) as f:
        r = json.load(f)
    out = {k: (np.array(r[k + "_mean"]), np.array(r[k + "_sd"])) for k in ("two", "two_without", "five")}
    out.update({k: r[k] for k in ("two_grid", "two_last_move_sd", "five_ess", "five_draws")})
    return out


if __name__ == "__main__":
    m2, s2, n2, mv = yardstick_2d()
    m0, s0, _, _ = yardstick_2d(())
    assert np.all(np.abs(m2 - m0) / s2 > 0.5)                          # a sampler that ignored the timeouts cannot pass
    m5, s5, ess, n5 = yardstick_5d()
    assert ess >= 20_000
    with open(RECORD, "w") as f:
        json.dump({"two_mean": m2.tolist(), "two_sd": s2.tolist(), "two_grid": n2, "two_last_move_sd": mv, "two_without_mean": m0.tolist(),
                   "two_without_sd": s0.tolist(), "five_mean": m5.tolist(), "five_sd": s5.tolist(), "five_ess": ess, "five_draws": n5}, f, indent=1)
        f.write("\n")
