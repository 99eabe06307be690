"""The rows, the Kolmogorov-Smirnov distance and the checks that the CPU and the GPU tests of simulratcliff's two rules share
(tests/test_ratcliff_domain_host.py: oracle section D; tests/test_gpu_ratcliff_domain.py: nddm_simulratcliff).

Rule 1: an invalid parameter row is not simulated -- every trial (NaN, NaN), the summary that of n_trials missing trials.
Rule 2: a trial that reaches the attempt cap or the sphere cap is (NaN, NaN) and counted in n_missing, nowhere else."""
from itertools import product

import numpy as np

import wiener_cdf_ref as ref

# columns: Nu, Alpha, Beta, Tau, Eta, Varsigma
GOOD_ROW = (1.0, 1.2, 0.5, 0.3, 1.0, 1.0)


def _row(**kw):
    r = dict(zip(("Nu", "Alpha", "Beta", "Tau", "Eta", "Varsigma"), GOOD_ROW))
    r.update(kw)
    return [r[k] for k in ("Nu", "Alpha", "Beta", "Tau", "Eta", "Varsigma")]


# what engine.simulratcliff refuses for host arrays, one defect per row
INVALID_ROWS = np.array([_row(Alpha=np.nan), _row(Alpha=-1.0), _row(Beta=1.5), _row(Varsigma=0.0), _row(Eta=np.inf), _row(Nu=np.nan),
                         _row(Varsigma=np.nan), _row(Tau=np.nan)], np.float32)

# Beta .5, Tau .3, Eta 0: G = radius Nu / (D pi) on the first sphere climbs past the point (~7) where no attempt can be accepted
LADDER_ROWS = np.array([[5, 1.4, .5, .3, 0, .6], [5, 1.6, .5, .3, 0, .6], [5, 1.8, .5, .3, 0, .6], [5, 2.0, .5, .3, 0, .6],
                        [5, 2.0, .5, .3, 0, .5]], np.float32)
LADDER_G = (6.2, 7.1, 8.0, 8.8, 12.7)

# the corners of the generator's box (alpha_not_scaled.py:66-72)
CORNER_ROWS = np.array([[nu, al, be, .3, eta, vs] for nu, al, be, eta, vs in product((-4, 0, 4), (.8, 1.4), (.3, .7), (0, 2), (.8, 1.4))],
                       np.float32)
CORNER_N = 20000
KS_BAR = 2.2 / np.sqrt(CORNER_N)                 # Kolmogorov tail: 96 row tests exceed it with probability ~0.01


def mixed_invalid_batch():
    """The invalid rows placed among good ones -> (params [B, 6], indices of the invalid rows, indices of the good ones)."""
    from prior_util import alpha_ns_prior
    good = alpha_ns_prior(2 * len(INVALID_ROWS) + 1, 31)
    p = np.empty((len(good) + len(INVALID_ROWS), 6), np.float32)
    bad = np.arange(len(INVALID_ROWS)) * 3 + 1
    ok = np.setdiff1d(np.arange(len(p)), bad)
    p[bad], p[ok] = INVALID_ROWS, good
    return p, bad, ok


def same_bits(a, b):
    """NaN masks equal, and the bits equal wherever there is a number (nan_to_num alone would let a NaN pass for a 0)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def assert_rule_1(res, rows, n_trials):
    """Rows `rows` of a result dict are invalid rows' output: no trial, the summary finalize_summary gives for n_trials missing ones."""
    t, s = np.asarray(res["trials"])[rows], np.asarray(res["summary"])[rows]
    assert np.all(np.isnan(t))
    assert np.all(s[:, 0] == 0) and np.all(s[:, 1] == 0) and np.all(s[:, 2] == n_trials)
    assert np.all(np.isnan(s[:, 3:7]))
    assert np.all(s[:, 7:9] == 0) and np.all(s[:, 9] == 0.5)          # no latent z in this model; (n_upper + n_missing / 2) / n


def assert_ext_formula(run, p, rows, ext_sigma=0.1):
    """ext = fma(ext_sigma, z(seed, set), Alpha or 1) on invalid rows as on valid ones.  run(params, ext_mode) -> ext [B].  Around 1
    (ext_mode 1) the invalid rows' values are the bits a batch of valid rows has at the same set indices; around Alpha (ext_mode 0) it
    is NaN where Alpha is and else that same normal: ext - Alpha = ext_1 - 1 to the rounding of the two fmas."""
    clean = p.copy()
    clean[rows] = GOOD_ROW
    e1 = np.asarray(run(p, 1))
    assert same_bits(e1, run(clean, 1)) and not np.any(np.isnan(e1))
    e0 = np.asarray(run(p, 0))
    assert np.array_equal(np.isnan(e0), np.isnan(p[:, 1]))
    ok = ~np.isnan(e0)
    assert np.abs((e0[ok].astype(np.float64) - p[ok, 1]) - (e1[ok].astype(np.float64) - 1.0)).max() < 1e-6
    assert np.std(e1 - 1.0) > 0.3 * ext_sigma


def assert_missing_is_nan_count(res):
    t, s = np.asarray(res["trials"]), np.asarray(res["summary"])
    nan_y = np.isnan(t[..., 0])
    assert np.array_equal(nan_y, np.isnan(t[..., 1]))
    assert np.array_equal(s[:, 2], nan_y.sum(axis=1).astype(np.float32))
    assert np.array_equal(s[:, 0], (t[..., 0] > 0).sum(axis=1).astype(np.float32))
    assert np.array_equal(s[:, 1], (t[..., 0] < 0).sum(axis=1).astype(np.float32))


def ks_rows(y, p, alpha_scale=1.0):
    """Kolmogorov-Smirnov distance of each row's signed RTs y [B, N] (no NaN) from the float64 law of its parameters p [B, 6], the
    boundary separation scaled by alpha_scale (the control: a law that is NOT the sampler's)."""
    out = np.empty(len(p))
    for b, (row, yb) in enumerate(zip(p.astype(np.float64), np.asarray(y, np.float64))):
        ys = np.sort(yb)
        n = len(ys)
        G = ref.signed_cdf(ys, alpha_scale * row[1], row[0], row[2], row[3], row[5], row[4])
        i = np.arange(n)
        out[b] = max(np.abs((i + 1) / n - G).max(), np.abs(i / n - G).max())
    return out


def assert_corner_law(y, p=CORNER_ROWS):
    """Every row below the bar against its own law; the control -- the law of 1.03 Alpha -- above it in the median."""
    ks = ks_rows(y, p)
    print("corner KS: worst %.4f (bar %.4f)" % (ks.max(), KS_BAR))
    assert ks.max() < KS_BAR, (int(ks.argmax()), ks.max())
    ctl = np.median(ks_rows(y, p, alpha_scale=1.03))
    print("control (1.03 Alpha): median KS %.4f" % ctl)
    assert ctl > KS_BAR, ctl
