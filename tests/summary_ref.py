"""The fused summaries (summary_stats[B, 10], include/nddm.h) recomputed EXACTLY from the trials of the same launch: NumPy and Python
integers, no GPU, no oracle.

The time columns of a summary are sums of integers: a responding trial's |column 0| is fmaf(float(k), tscale, tau) with the integer time
k (the step index, or 1/256 step with the bridge), so k is recovered from the float32 output bit for bit, sum k and sum k^2 are formed in
integers, mean and variance as exact rationals, and one rounding to float64 gives the reference.  The kernel (finalize_summary,
csrc/nddm_sim.h) computes in float64 from the same integer sums and rounds once to float32: the bound of columns 3-6 is 1 float32 ulp
of the reference (half an ulp for the rounding, the rest for the float64 arithmetic before it).  The z columns are fixed-point sums
(sum z in 2^-32, sum z^2 in 2^-24, every term truncated towards zero, then a float32 rounding):
    |mean_z - ref| <= 2^-32 + ulp32(ref) / 2          |var_z - ref| <= 2^-24 + 2 |mean_z| 2^-32 + ulp32(ref) / 2
Counts and column 9 are exact."""
from fractions import Fraction

import numpy as np

M_BASIC, M_SINGLE, M_ALT, M_ALPHA_NS, M_EXPLICIT = 0, 1, 2, 3, 4
TAU_COL = {M_BASIC: 3, M_SINGLE: 3, M_ALT: 3, M_ALPHA_NS: 3, M_EXPLICIT: 2}
HAS_Z = (M_SINGLE, M_ALT)
C_TIMEOUT, C_UPPER, C_LOWER, C_INVALID = 0, 1, 2, 3          # the staged result's code (csrc/nddm_sim.h: flush_set)


def tscale_of(dt, bridge):
    """Seconds per unit of the integer time, in the float32 arithmetic of the launch (A.tscale)."""
    dt = np.float32(dt)
    return np.float32(dt * np.float32(1.0 / 256.0)) if bridge else dt


def _fma32_exact(k, tscale, tau):
    """float32(k * tscale + tau) with ONE rounding (to nearest, ties to even), by rational arithmetic; k < 2^24."""
    x = Fraction(int(k)) * Fraction(float(tscale)) + Fraction(float(tau))
    if x == 0:
        return np.float32(0.0)
    assert x > 0
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    assert Fraction(2) ** e <= x < Fraction(2) ** (e + 1) and e >= -126
    q = x / Fraction(2) ** (e - 23)
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (n & 1)):
        n += 1
    return np.float32(float(Fraction(n) * Fraction(2) ** (e - 23)))


def recover(model, params, trials, dt, bridge):
    """(k int64 [B, N], code int8 [B, N], known bool [B, N]): the integer time and the result code of every trial.  k is `known` for
    every responding trial (and for the basic model's timeouts, whose time is written too); a responding trial whose k cannot be found
    is an AssertionError."""
    p = np.asarray(params, np.float32)
    t = np.asarray(trials, np.float32)
    B, N = t.shape[:2]
    c0 = t[..., 0]
    if model == M_BASIC:
        ch = t[..., 1]
        assert np.all((ch == 1) | (ch == -1) | (ch == 0)), "basic: column 1 is a choice"
        code = np.where(ch == 1, C_UPPER, np.where(ch == -1, C_LOWER, C_TIMEOUT)).astype(np.int8)
        want = np.ones((B, N), bool)
    else:
        code = np.where(c0 > 0, C_UPPER, np.where(c0 < 0, C_LOWER, C_TIMEOUT)).astype(np.int8)
        if model == M_EXPLICIT:
            code[np.isnan(c0)] = C_INVALID
        else:
            assert not np.isnan(c0).any(), "only the explicit-boundary model has invalid trials"
        want = (code == C_UPPER) | (code == C_LOWER)
    ts, tau = tscale_of(dt, bridge), p[:, TAU_COL[model]]
    x32 = np.abs(np.where(want, c0, np.float32(0.0))).astype(np.float32)
    # k is unique when neighbouring k give float32 values well apart
    assert 4.0 * float(np.spacing(x32.max(initial=np.float32(0)))) < float(ts), "ulp(rt) is not below tscale: k would not be unique"
    ts64, tau64 = np.float64(ts), tau.astype(np.float64)[:, None]
    k0 = np.rint((x32.astype(np.float64) - tau64) / ts64).astype(np.int64)
    k = np.zeros((B, N), np.int64)
    found = ~want
    for d in (0, -1, 1):
        cand = np.maximum(k0 + d, 0)
        assert cand.max(initial=0) < (1 << 24), "float(k) would round"
        emu = (cand.astype(np.float32).astype(np.float64) * ts64 + tau64).astype(np.float32)      # the fma, up to a double rounding
        hit = ~found & (emu.view(np.uint32) == x32.view(np.uint32))
        k[hit] = cand[hit]
        found |= hit
    for b, j in zip(*np.nonzero(~found)):          # the float64 emulation rounded twice: decide those by exact arithmetic
        for d in (0, -1, 1):
            kk = max(int(k0[b, j]) + d, 0)
            if _fma32_exact(kk, ts, p[b, TAU_COL[model]]).view(np.uint32) == x32[b, j].view(np.uint32):
                k[b, j] = kk
                found[b, j] = True
                break
    assert found.all(), f"{int((~found).sum())} responding trials have no integer time, first at {tuple(np.argwhere(~found)[0])}"
    return k, code, want


def check_codes(codes, k, code, known):
    """The 2-byte wire format (k | code << 14) says the same as the float pairs."""
    c = np.asarray(codes).view(np.uint16).astype(np.int64)
    assert np.array_equal(c >> 14, code.astype(np.int64)), "codes >> 14 differs from the choice of the float pairs"
    assert np.array_equal((c & 0x3fff)[known], k[known]), "codes & 0x3fff differs from the integer time of the float pairs"


def _moments(ks, ts, tau):
    """(mean, population variance) of tau + ts * k as float64, exact up to the final rounding; NaN for no trials."""
    n = int(ks.size)
    if n == 0:
        return np.nan, np.nan
    assert int(ks.max()) ** 2 * n < (1 << 62)
    s1, s2 = int(ks.sum(dtype=np.int64)), int((ks * ks).sum(dtype=np.int64))
    fts, ftau = Fraction(float(ts)), Fraction(float(tau))
    return float(ftau + fts * Fraction(s1, n)), float(fts * fts * Fraction(n * s2 - s1 * s1, n * n))


def summary_from_trials(model, params_f32, trials_f32, dt, bridge, n_trials, codes=None):
    """float64 [B, 10]: the summary row of every set, from that launch's own trials (f32 [B, n_trials, 2])."""
    p = np.asarray(params_f32, np.float32)
    t = np.asarray(trials_f32, np.float32)
    assert t.shape == (p.shape[0], n_trials, 2)
    k, code, known = recover(model, p, t, dt, bridge)
    if codes is not None:
        check_codes(codes, k, code, known)
    ts = tscale_of(dt, bridge)
    ref = np.zeros((p.shape[0], 10), np.float64)
    for b in range(p.shape[0]):
        up, lo = code[b] == C_UPPER, code[b] == C_LOWER
        n_up, n_lo = int(up.sum()), int(lo.sum())
        n_miss = n_trials - n_up - n_lo
        ref[b, 0:3] = n_up, n_lo, n_miss
        tau = p[b, TAU_COL[model]]
        ref[b, 3:5] = _moments(k[b][up | lo], ts, tau)
        ref[b, 5:7] = _moments(k[b][up], ts, tau)
        if model in HAS_Z:
            z = t[b, :, 1].astype(np.float64)
            ref[b, 7], ref[b, 8] = z.mean(), z.var()
        ref[b, 9] = np.float64(np.float32((n_up + 0.5 * n_miss) / n_trials))
    return ref


def ulp32(x):
    """Spacing of float32 at |x| (float64 array in, float64 out; NaN stays NaN)."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def z_bounds(ref):
    """(bound of |mean_z - ref|, bound of |var_z - ref|) [B] from the fixed-point format."""
    bm = 2.0 ** -32 + 0.5 * ulp32(ref[:, 7])
    bv = 2.0 ** -24 + 2.0 * np.abs(ref[:, 7]) * 2.0 ** -32 + 0.5 * ulp32(ref[:, 8])
    return bm, bv


def check_summary(model, summary_f32, ref, label=""):
    """Hold a float32 summary [B, 10] to the reference.  Returns dict(ulp=worst distance of columns 3-6 in float32 ulps of the reference,
    mean_z / var_z = worst ratio of the z errors to their bounds)."""
    s32 = np.asarray(summary_f32, np.float32)
    s = s32.astype(np.float64)
    assert s.shape == ref.shape
    for c in (0, 1, 2, 9):
        assert np.array_equal(s[:, c], ref[:, c]), (label, "column", c, np.nonzero(s[:, c] != ref[:, c])[0][:5])
    worst = 0.0
    for c in (3, 4, 5, 6):
        assert np.array_equal(np.isnan(s[:, c]), np.isnan(ref[:, c])), (label, "NaN pattern of column", c)
        ok = ~np.isnan(ref[:, c])
        d = np.abs(s[ok, c] - ref[ok, c])
        zero = ref[ok, c] == 0
        assert np.all(d[zero] == 0), (label, "column", c, "an exact 0 is required")
        u = d[~zero] / ulp32(ref[ok, c][~zero])
        if u.size:
            worst = max(worst, float(u.max()))
            assert u.max() <= 1.0, (label, "column", c, "ulps", float(u.max()), "row", int(np.nonzero(ok)[0][~zero][u.argmax()]))
    out = {"ulp": worst, "mean_z": 0.0, "var_z": 0.0}
    if model in HAS_Z:
        bm, bv = z_bounds(ref)
        rm, rv = np.abs(s[:, 7] - ref[:, 7]) / bm, np.abs(s[:, 8] - ref[:, 8]) / bv
        out["mean_z"], out["var_z"] = float(rm.max()), float(rv.max())
        assert rm.max() <= 1.0, (label, "mean_z: ratio to its bound", float(rm.max()), "row", int(rm.argmax()))
        assert rv.max() <= 1.0, (label, "var_z: ratio to its bound", float(rv.max()), "row", int(rv.argmax()))
    else:
        assert np.all(s32[:, 7:9].view(np.uint32) == 0), (label, "z columns of a model without z")
    for c in (4, 6, 8):
        assert np.all((s[:, c] >= 0) | np.isnan(s[:, c])), (label, "negative variance in column", c, float(np.nanmin(s[:, c])))
    assert not np.isnan(s[:, 7:10]).any(), label
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# The rows both test files run: the edge rows of each model, then rows from the reference's priors (tests/prior_util.py).
#   a  all timeouts (columns 3-6 NaN, column 9 = 0.5)      b  all upper, tau = 0      c  (almost) all lower
#   d  slow, a share of timeouts                           e  the 16-bit flush path's worst case: at dt = .001 every trial answers
#      with k ~ 16070..16320, 8 trials per lane at 512 trials per tile: the largest sums of squares a 32-bit lane accumulator meets
# Models with an external datum carry the z corners in the same rows: (sigma1, gamma) = (1, 1), (5, 2), (.001, .001), (1e-5, 0), (1, 1).
BASIC_EDGE = np.array([[0, 50, .5, .3, .01], [9, .6, .5, 0, 1], [-9, 2, .9, .2, 1], [.2, 2.5, .5, .3, .6], [1, 32.4, .5, .2, .01]], np.float32)
ROW_E = 4
N_EDGE = 5
SHAPES = ((0.01, 400.0), (0.001, 4000.0), (0.001, 16383.0), (0.001, 16384.0), (0.01, 0.0))
BRIDGE_SHAPES = ((0.01, 400.0), (0.001, 4000.0), (0.004, 1001.0))
MODEL_NAMES = {M_BASIC: "basic", M_SINGLE: "single", M_ALT: "alt", M_ALPHA_NS: "alpha_ns", M_EXPLICIT: "explicit"}


def edge_rows(model):
    e = BASIC_EDGE
    drift, a, beta, tau, dc = (e[:, i] for i in range(5))
    z = np.array([[1, 1], [5, 2], [.001, .001], [1e-5, 0], [1, 1]], np.float32)
    if model == M_BASIC:
        return e.copy()
    if model == M_SINGLE:        # drift, mu_alpha, beta, ter, std_alpha, dc, sigma1, gamma: the boundary of rows a and e is not spread
        std = np.array([0, .05, .1, .3, 0], np.float32)
        return np.stack([drift, a, beta, tau, std, dc, z[:, 0], z[:, 1]], axis=1)
    if model == M_ALT:           # drift, alpha, beta, ter, std_dc, mu_dc, sigma1, gamma
        std = np.array([0, .1, .1, .05, 0], np.float32)
        return np.stack([drift, a, beta, tau, std, dc, z[:, 0], z[:, 1]], axis=1)
    if model == M_ALPHA_NS:      # Nu, Alpha, Beta, Tau, Eta, Varsigma
        eta = np.array([0, .5, .5, 1, 0], np.float32)
        return np.stack([drift, a, beta, tau, eta, dc], axis=1)
    return np.stack([drift, beta, tau, dc], axis=1)          # explicit: drift, beta, ter, dc; the boundaries come from rows_and_bounds


def rows_and_bounds(model, n_trials, n_prior=27, seed=11, invalid=False):
    """(params f32 [5 + n_prior, P], bounds f32 [B, n_trials] or None).  invalid: the explicit model's row d has every 7th boundary
    negative (those trials are NaN, counted missing and left out of the moments); such bounds only pass as a device tensor."""
    import prior_util
    if model == M_BASIC:
        pr = prior_util.basic_prior(n_prior, seed)
    elif model in (M_SINGLE, M_ALT):
        pr = prior_util.single_prior(n_prior, seed, gamma=1.0)
        pr[:, 7] = np.random.default_rng(seed).uniform(0.0, 2.0, n_prior).astype(np.float32)
        if model == M_ALT:
            pr[:, 4] = np.minimum(pr[:, 4], 1.0)
    elif model == M_ALPHA_NS:
        pr = prior_util.alpha_ns_prior(n_prior, seed)
    else:
        pr = prior_util.basic_prior(n_prior, seed)[:, [0, 2, 3, 4]]
    p = np.concatenate([edge_rows(model), pr]).astype(np.float32)
    bounds = None
    if model == M_EXPLICIT:
        bounds = np.abs(np.random.default_rng(seed + 1).normal(1.2, 0.4, size=(p.shape[0], n_trials))).astype(np.float32)
        bounds[:N_EDGE] = BASIC_EDGE[:, 1:2]
        if invalid:
            bounds[3, ::7] = -bounds[3, ::7]
    return p, bounds
