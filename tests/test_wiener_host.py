"""CPU tests of the Wiener log-likelihood (nddm_wiener_log_likelihood): the float64 yardstick pins itself against the published
identities, the fixed-trip scheme the kernel evaluates is exact to 1e-9 against it, and the C ABI / Python adapter refuse bad input
before any device work."""
import ctypes
import os
import shutil
import sys

import numpy as np
import pytest
from scipy import integrate

import wiener_cdf_ref as C
import wiener_ref as W
from conftest import GOLDEN, ROOT

U_GRID = np.geomspace(1e-3, 50.0, 400)[:, None]
W_GRID = np.linspace(0.01, 0.99, 99)[None, :]


def test_small_and_large_time_series_agree():
    # in float64 each series can be summed where its terms do not cancel: both do on [0.1, 2]
    u = np.geomspace(0.1, 2.0, 200)[:, None]
    assert np.max(np.abs(np.expm1(W.log_g_small(u, W_GRID) - W.log_g_large(u, W_GRID)))) < 1e-11
    # the ends of [1e-3, 50], where float64 cannot sum the other series, at 400 digits (mpmath)
    for u0 in (1e-3, 1e-2, 10.0, 50.0):
        for w0 in (0.01, 0.3, 0.99):
            s, l = W.mp_g(u0, w0, True, dps=400), W.mp_g(u0, w0, False, dps=400)
            assert abs(float((s - l).real)) < 1e-12, (u0, w0)
            assert abs(float(W.log_g(u0, w0)) - float(s.real)) < 1e-12 * max(1.0, abs(float(s.real))), (u0, w0)


def test_fixed_trip_scheme_of_the_kernel_is_exact_to_1e9():
    """5 small-time terms below u* = 0.375, 3 large-time terms at and above: the design choice of csrc/nddm_wiener.h."""
    ref = W.log_g(U_GRID, W_GRID)
    ft = W.log_g_fixed_trip(U_GRID, W_GRID)
    assert np.max(np.abs(np.expm1(ft - ref))) <= 1e-9
    band = np.linspace(0.30, 0.50, 201)[:, None]                       # the crossover band, densely
    assert np.max(np.abs(np.expm1(W.log_g_fixed_trip(band, W_GRID) - W.log_g(band, W_GRID)))) <= 1e-9


@pytest.mark.parametrize("nu,eta,w,t", [(1.0, 0.5, 0.4, 0.3), (-2.0, 1.5, 0.7, 1.2), (0.5, 2.5, 0.2, 0.05), (3.0, 1.0, 0.5, 2.5)])
def test_eta_closed_form_equals_quadrature_over_the_drift(nu, eta, w, t):
    a = 1.3
    def integrand(v):
        return np.exp(float(W.log_f_lower(t, a, v, w)) - 0.5 * ((v - nu) / eta) ** 2) / (eta * np.sqrt(2 * np.pi))
    q, _ = integrate.quad(integrand, nu - 12 * eta, nu + 12 * eta, epsabs=0, epsrel=1e-12, limit=400)
    closed = np.exp(float(W.log_f_lower(t, a, nu, w, eta)))
    assert abs(q - closed) <= 1e-9 * closed


@pytest.mark.parametrize("a,v,beta,s", [(1.0, 1.0, 0.5, 1.0), (2.0, -1.5, 0.3, 1.2), (0.8, 3.0, 0.7, 0.6), (1.5, 0.0, 0.5, 1.0)])
def test_density_normalises_and_upper_mass_is_closed_form(a, v, beta, s):
    up = integrate.quad(lambda t: np.exp(float(W.log_f(t, True, a, v, beta, s))), 0, np.inf, epsrel=1e-12, limit=400)[0]
    lo = integrate.quad(lambda t: np.exp(float(W.log_f(t, False, a, v, beta, s))), 0, np.inf, epsrel=1e-12, limit=400)[0]
    assert abs(up + lo - 1.0) < 1e-9
    assert abs(up - W.p_upper(a, v, beta, s)) < 1e-9


@pytest.mark.parametrize("a,v,beta,s,t", [(1.0, 1.0, 0.5, 1.0, 0.4), (2.0, -1.5, 0.3, 1.2, 1.5), (0.8, 3.0, 0.7, 0.6, 0.2)])
def test_survival_is_one_minus_the_integrated_density(a, v, beta, s, t):
    f = lambda x: np.exp(float(W.log_f(x, True, a, v, beta, s))) + np.exp(float(W.log_f(x, False, a, v, beta, s)))
    F = integrate.quad(f, 0, t, epsrel=1e-12, limit=400)[0]
    assert abs(W.survival(t, a, v, beta, s) - (1.0 - F)) < 1e-9
    assert abs(W.log_survival(t, a, v, beta, s) - np.log(W.survival(t, a, v, beta, s))) < 1e-9


def test_survival_yardsticks_agree_where_both_apply():
    """log1p(-(F_lower + F_upper)) of the distribution function's yardstick against the survival series at the precision it needs, to
    1e-9 where S >= 1e-3: on the four rows of the censoring defect's report and on rows of every set of the censoring tests, small u
    and wide boundaries (a'|v'| up to 500) included -- where the float64 series of W.log_survival is off or not finite."""
    pytest.importorskip("mpmath")
    sets = C.censor_sets(n_prior=400, n_box=100, with_fixture=False)
    rng = np.random.default_rng(3)
    n_checked, widest, smallest_u, series_off = 0, 0.0, np.inf, 0
    cases = [(C.REPORTED_ROWS, C._times(C.REPORTED_ROWS, C.REPORTED_T[:, None])[1])] + [(p32, t) for p32, _, t in sets.values()]
    for k, (p32, t) in enumerate(cases):
        a, v, beta, _, s, _ = C.row_columns(p32, True)
        ref, ok = C.log_survival(t, a[:, None], v[:, None], beta[:, None], s[:, None])
        # the series' cost grows with the precision it needs, a'|v'| + v'^2 t / 2 + 1 / (2u) digits-times-ln-10: points within 1200 of it
        ap, vp = (a / s)[:, None], (v / s)[:, None]
        cand = np.argwhere(ok & (ap * np.abs(vp) + vp * vp * t / 2 + ap * ap / (2 * t) <= 1200.0))
        idx = cand
        if k > 0:                                                       # the widest of them and a random few
            order = np.argsort(-(ap * np.abs(vp))[cand[:, 0], 0], kind="stable")
            idx = np.concatenate([cand[order[:8]], cand[rng.choice(len(cand), 8, replace=False)]])
        for i, j in idx:
            mp = W.mp_log_survival(t[i, j], a[i], v[i], beta[i], s[i])
            assert abs(mp - ref[i, j]) <= 1e-9, (k, p32[i], t[i, j], mp, ref[i, j])
            with np.errstate(all="ignore"):
                old = W.log_survival(t[i, j], a[i], v[i], beta[i], s[i])
            series_off += not abs(old - ref[i, j]) <= 1e-9
            n_checked += 1
            widest, smallest_u = max(widest, a[i] * abs(v[i]) / s[i] ** 2), min(smallest_u, t[i, j] * s[i] ** 2 / a[i] ** 2)
    print(f"{n_checked} points, a'|v'| up to {widest:.0f}, u down to {smallest_u:.2g}; the float64 series alone is off on {series_off}")
    assert n_checked >= 50 and widest > 100 and smallest_u < 0.01 and series_off > 0
    assert np.max(np.abs(C.log_survival(C.REPORTED_T, *[x for x in C.row_columns(C.REPORTED_ROWS, True)[:3]], C.REPORTED_ROWS[:, 4].astype(np.float64))[0]
                         - C.REPORTED_LOG_S)) < 1e-5


def test_survival_fixture_is_the_yardsticks_output():
    """tests/golden/wiener_survival.npz (tests/golden/make_wiener_survival.py): where S >= 1e-3 its values are C.log_survival's to 1e-12;
    below, they lie under log 1e-3 and continue each row's non-increasing sequence; the report's four rows lead it."""
    g = np.load(os.path.join(GOLDEN, "wiener_survival.npz"))
    p32, rt, log_s, deep = g["params"], g["rt"], g["log_s"], g["mp"]
    assert p32.dtype == rt.dtype == np.float32 and log_s.dtype == np.float64 and rt.shape == log_s.shape == deep.shape == (p32.shape[0], C.CENSOR_TIMES)
    t = (rt - p32[:, 3:4]).astype(np.float32).astype(np.float64)
    a, v, beta, _, s, _ = C.row_columns(p32, True)
    ref, ok = C.log_survival(t, a[:, None], v[:, None], beta[:, None], s[:, None])
    assert np.array_equal(ok, ~deep) and deep.sum() > 1000 and ok.sum() > 1000
    assert np.max(np.abs(log_s - ref)[ok]) <= 1e-12
    assert np.all(log_s[deep] < np.log(C.S_FLOOR)) and np.all(np.diff(log_s, axis=1) <= 0) and np.all(log_s <= 0)
    assert np.array_equal(p32[:4], C.REPORTED_ROWS) and np.array_equal(rt[:4, -1], C.REPORTED_RT)
    assert np.max(np.abs(log_s[:4, -1] - C.REPORTED_LOG_S)) < 1e-5
    assert np.any((t / (a / s)[:, None] ** 2 < 0.06) & deep)              # deep tails in the small-time form's own range


def test_prior_rows_cover_what_the_models_draw():
    p32, rt32, up, t = C.prior_rows(20_000, basic=True)
    assert p32.shape == (20_000, 5) and p32[:, 4].min() >= 0.05 and np.all(t > 0) and 0.45 < up.mean() < 0.55
    assert (p32[:, 1] / p32[:, 4]).max() > 20 and (np.abs(p32[:, 0]) / p32[:, 4]).max() > 60             # (27.8 and 79.7)
    p32, rt32, up, t = C.prior_rows(20_000, basic=False)
    s, eta = p32[:, 5], p32[:, 4]
    assert p32.shape == (20_000, 6) and np.all(t > 0)
    assert s[:10_000].min() >= 0.8 and s[:10_000].max() <= 1.4 and eta[:10_000].max() <= 2.0           # the model's prior
    assert s[10_000:].min() < 0.52 and s[10_000:].max() > 1.98 and eta[10_000:].max() > 2.9            # the box, Varsigma in [0.5, 2]
    assert np.mean((s != 1.0) & (eta > 0)) > 0.8
    # the same draw of u as accuracy_rows: log-uniform in [1e-3, 50] with a quarter in [0.3, 0.5]
    u = t / (p32[:, 1].astype(np.float64) / s) ** 2
    assert 0.24 < np.mean((u > 0.29) & (u < 0.51)) < 0.32 and u.min() < 2e-3 and u.max() > 40


@pytest.mark.skipif(shutil.which("g++") is None and shutil.which("c++") is None and shutil.which("clang++") is None, reason="no host C++ compiler")
def test_per_trial_code_compiled_for_the_host_meets_the_device_tests_bars():
    """tools/wiener_host.py: wiener_row, wiener_trial (choice 0 included), wiener_cdf_side and wiener_cdf_trial of the headers as a
    stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer, over the rows of tests/test_gpu_wiener_priors.py and at its
    bars.  Density: |d log f| <= 1e-4 where |log f| <= 20, 1e-5 relative beyond; F and P(upper): 2e-5.  Censored: never NaN, never above
    0, non-increasing along each row's 16 times; 2e-5 + 1e-5 |ref| where S >= 1e-3, 1e-3 |ref| below (the fixture); 1 - S through the
    distribution function at 2e-5.  With the large-time series alone (before the small-time form) this test fails on the report's four
    rows: NaN, +9.3, +15.7 and -0.16 for log S = -0.000000, -2.507289, -0.009398 and -6.160853."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import wiener_host as H
    r = H.survey(sanitize=True)
    cases = r["cases"]
    for name, c in cases.items():
        print(name, c)
    for name in ("basic_prior", "alpha_ns_prior_and_box"):
        c = cases[name]
        assert c["rows"] == 20_000
        assert c["max_abs_dlogf_inner"] <= 1e-4 and c["max_rel_dlogf_beyond"] <= 1e-5, name
        assert c["max_abs_dF"] <= 2e-5 and c["max_abs_dp_upper"] <= 2e-5, name
    for name in ("prior_1s", "prior_4s", "box", "fixture"):
        c = cases["censored_" + name]
        assert c["nan"] == 0 and c["above_0"] == 0 and c["increasing_pairs"] == 0, name
        assert c["points_S_ge_1e-3"] > 1000 and c["max_err_over_bar"] <= 1.0 and c["max_abs_dcdf"] <= 2e-5, name
    fx = cases["censored_fixture"]
    assert fx["points_S_lt_1e-3"] > 1000 and fx["max_rel_err_S_lt_1e-3"] <= 1e-3 and fx["max_abs_dcdf_S_lt_1e-3"] <= 2e-5
    got = np.array(fx["reported_rows_log_S"])
    assert np.all(np.abs(got - C.REPORTED_LOG_S) <= 2e-5 + 1e-5 * np.abs(C.REPORTED_LOG_S) + 1e-5), got       # (+ the table's own rounding)


def test_c_abi_exports_the_entry_and_validates_before_any_hip_call():
    from bayesflow_nddms_amd import _lib
    L = _lib.lib()
    assert "nddm_wiener_log_likelihood" in _lib.EXPORTS and hasattr(L, "nddm_wiener_log_likelihood")
    assert L.nddm_abi_version() == _lib.ABI_VERSION == 4
    d = ctypes.c_void_p(16)
    f = L.nddm_wiener_log_likelihood                                    # (the argument checks: test_argument_contract_of_the_five_entry_points)
    import torch
    if not torch.cuda.is_available():
        assert f(0, d, 4, 2, d, 10, 0, d, None, None) in (_lib.NDDM_ERR_HIP, _lib.NDDM_ERR_NO_DEVICE)


d = "d"                                                                 # stands for a non-NULL pointer (never dereferenced: every case ends before a launch)
# (entry point, (model, params, R, draws_per_dataset, data, n, flags, *outputs), status, nddm_last_error() in full).  The texts are the
# library's before the five entry points shared one launch path.  Per entry point: the cases its own file used to hold, then the order
# of the checks -- model before flags, flags before shape, shape and R / 16 before the pointers (so 2^35 rows need no memory), the
# empty batch before the pointers, inputs before outputs.
ARGUMENT_CASES = [
    ("log_likelihood", (1, d, 4, 1, d, 10, 0, d, None), "PARAM", 'nddm_wiener_log_likelihood: model 1 has no closed-form likelihood here (NDDM_BASIC_DDM_DC and NDDM_ALPHA_NOT_SCALED only)'),
    ("log_likelihood", (7, d, 4, 1, d, 10, 0, d, None), "PARAM", 'nddm_wiener_log_likelihood: model 7 has no closed-form likelihood here (NDDM_BASIC_DDM_DC and NDDM_ALPHA_NOT_SCALED only)'),
    ("log_likelihood", (0, d, 4, 1, d, 10, 1, d, None), "PARAM", 'nddm_wiener_log_likelihood: flags must be 0 (reserved)'),
    ("log_likelihood", (0, None, 4, 1, d, 10, 0, d, None), "NULL", 'params or data is NULL'),
    ("log_likelihood", (3, d, 4, 1, None, 10, 0, d, None), "NULL", 'params or data is NULL'),
    ("log_likelihood", (0, d, 4, 1, d, 10, 0, None, None), "NULL", 'no output buffer given'),
    ("log_likelihood", (0, d, -1, 1, d, 10, 0, d, None), "SHAPE", 'R >= 0, n_trials > 0 and draws_per_dataset > 0 dividing R are required'),
    ("log_likelihood", (0, d, 4, 1, d, 0, 0, d, None), "SHAPE", 'R >= 0, n_trials > 0 and draws_per_dataset > 0 dividing R are required'),
    ("log_likelihood", (0, d, 4, 0, d, 10, 0, d, None), "SHAPE", 'R >= 0, n_trials > 0 and draws_per_dataset > 0 dividing R are required'),
    ("log_likelihood", (0, d, 4, 3, d, 10, 0, d, None), "SHAPE", 'R >= 0, n_trials > 0 and draws_per_dataset > 0 dividing R are required'),
    ("log_likelihood", (0, d, 0, 1, d, 10, 0, d, None), "OK", ''),
    ("log_likelihood", (1, None, -1, 0, None, 0, 1, None, None), "PARAM", 'nddm_wiener_log_likelihood: model 1 has no closed-form likelihood here (NDDM_BASIC_DDM_DC and NDDM_ALPHA_NOT_SCALED only)'),
    ("log_likelihood", (0, None, -1, 0, None, 0, 1, None, None), "PARAM", 'nddm_wiener_log_likelihood: flags must be 0 (reserved)'),
    ("log_likelihood", (0, d, 4, 3, d, 10, 1, d, None), "PARAM", 'nddm_wiener_log_likelihood: flags must be 0 (reserved)'),
    ("log_likelihood", (0, None, 4, 3, None, 10, 0, None, None), "SHAPE", 'R >= 0, n_trials > 0 and draws_per_dataset > 0 dividing R are required'),
    ("log_likelihood", (0, None, 1 << 35, 1, None, 10, 0, None, None), "SHAPE", 'R / 16 must be < 2^31 per launch'),
    ("log_likelihood", (0, None, 0, 1, None, 10, 0, None, None), "OK", ''),
    ("log_likelihood", (0, None, 4, 1, d, 10, 0, None, None), "NULL", 'params or data is NULL'),
    ("log_likelihood", (0, d, 4, 1, None, 10, 0, None, None), "NULL", 'params or data is NULL'),
    ("cdf", (1, d, 4, 1, d, 10, 0, d, None), "PARAM", 'nddm_wiener_cdf: model 1 has no closed-form distribution function here (NDDM_BASIC_DDM_DC and NDDM_ALPHA_NOT_SCALED only)'),
    ("cdf", (7, d, 4, 1, d, 10, 0, d, None), "PARAM", 'nddm_wiener_cdf: model 7 has no closed-form distribution function here (NDDM_BASIC_DDM_DC and NDDM_ALPHA_NOT_SCALED only)'),
    ("cdf", (0, d, 4, 1, d, 10, 1, d, None), "PARAM", 'nddm_wiener_cdf: flags must be 0 (reserved)'),
    ("cdf", (0, None, 4, 1, d, 10, 0, d, None), "NULL", 'params or data is NULL'),
    ("cdf", (3, d, 4, 1, None, 10, 0, d, None), "NULL", 'params or data is NULL'),
    ("cdf", (0, d, 4, 1, d, 10, 0, None, None), "NULL", 'no output buffer given'),
    ("cdf", (0, d, 4, 1, None, 10, 0, None, None), "NULL", 'no output buffer given'),
    ("cdf", (0, d, -1, 1, d, 10, 0, d, None), "SHAPE", 'R >= 0, n_trials > 0 and draws_per_dataset > 0 dividing R are required'),
    ("cdf", (0, d, 4, 1, d, 0, 0, d, None), "SHAPE", 'R >= 0, n_trials > 0 and draws_per_dataset > 0 dividing R are required'),
    ("cdf", (0, d, 4, 0, d, 10, 0, d, None), "SHAPE", 'R >= 0, n_trials > 0 and draws_per_dataset > 0 dividing R are required'),
    ("cdf", (0, d, 4, 3, d, 10, 0, d, None), "SHAPE", 'R >= 0, n_trials > 0 and draws_per_dataset > 0 dividing R are required'),
    ("cdf", (0, d, 0, 1, d, 10, 0, d, None), "OK", ''),
    ("cdf", (0, d, 0, 1, None, 10, 0, None, d), "OK", ''),
    ("cdf", (7, None, -1, 0, None, 0, 1, None, None), "PARAM", 'nddm_wiener_cdf: model 7 has no closed-form distribution function here (NDDM_BASIC_DDM_DC and NDDM_ALPHA_NOT_SCALED only)'),
    ("cdf", (0, None, -1, 0, None, 0, 0, None, None), "SHAPE", 'R >= 0, n_trials > 0 and draws_per_dataset > 0 dividing R are required'),
    ("cdf", (1, None, -1, 0, None, 0, 1, None, None), "PARAM", 'nddm_wiener_cdf: model 1 has no closed-form distribution function here (NDDM_BASIC_DDM_DC and NDDM_ALPHA_NOT_SCALED only)'),
    ("cdf", (0, None, -1, 0, None, 0, 1, None, None), "PARAM", 'nddm_wiener_cdf: flags must be 0 (reserved)'),
    ("cdf", (0, d, 4, 3, d, 10, 1, d, None), "PARAM", 'nddm_wiener_cdf: flags must be 0 (reserved)'),
    ("cdf", (0, None, 4, 3, None, 10, 0, None, None), "SHAPE", 'R >= 0, n_trials > 0 and draws_per_dataset > 0 dividing R are required'),
    ("cdf", (0, None, 1 << 35, 1, None, 10, 0, None, None), "SHAPE", 'R / 16 must be < 2^31 per launch'),
    ("cdf", (0, None, 0, 1, None, 10, 0, None, None), "OK", ''),
    ("cdf", (0, None, 4, 1, d, 10, 0, None, None), "NULL", 'params or data is NULL'),
    ("quantile", (1, d, 4, 1, d, 10, 0, d), "PARAM", 'nddm_wiener_quantile: model 1 has no closed-form distribution function here (NDDM_BASIC_DDM_DC and NDDM_ALPHA_NOT_SCALED only)'),
    ("quantile", (0, None, 4, 1, d, 10, 0, d), "NULL", 'params or probs is NULL'),
    ("quantile", (0, d, 4, 1, None, 10, 0, d), "NULL", 'params or probs is NULL'),
    ("quantile", (0, d, 4, 1, d, 10, 0, None), "NULL", 'no output buffer given'),
    ("quantile", (0, d, 4, 3, d, 10, 0, d), "SHAPE", 'R >= 0, n > 0 and draws_per_dataset > 0 dividing R are required'),
    ("quantile", (0, d, 0, 1, d, 10, 0, d), "OK", ''),
    ("quantile", (0, None, 0, 1, None, 10, 1, None), "OK", ''),
    ("quantile", (0, d, 4, 1, d, 10, 2, d), "PARAM", 'nddm_wiener_quantile: flags must be 0 or NDDM_QUANTILE_CONDITIONAL'),
    ("quantile", (0, d, 4, 1, d, 10, 3, d), "PARAM", 'nddm_wiener_quantile: flags must be 0 or NDDM_QUANTILE_CONDITIONAL'),
    ("quantile", (0, d, 4, 1, d, 10, 4, d), "PARAM", 'nddm_wiener_quantile: flags must be 0 or NDDM_QUANTILE_CONDITIONAL'),
    ("quantile", (0, d, 4, 1, d, 10, 2147483648, d), "PARAM", 'nddm_wiener_quantile: flags must be 0 or NDDM_QUANTILE_CONDITIONAL'),
    ("quantile", (0, d, 4, 1, d, 10, 4294967294, d), "PARAM", 'nddm_wiener_quantile: flags must be 0 or NDDM_QUANTILE_CONDITIONAL'),
    ("quantile", (0, d, 0, 1, d, 10, 1, d), "OK", ''),
    ("quantile", (7, None, -1, 0, None, 0, 2, None), "PARAM", 'nddm_wiener_quantile: model 7 has no closed-form distribution function here (NDDM_BASIC_DDM_DC and NDDM_ALPHA_NOT_SCALED only)'),
    ("quantile", (0, None, -1, 0, None, 0, 2, None), "PARAM", 'nddm_wiener_quantile: flags must be 0 or NDDM_QUANTILE_CONDITIONAL'),
    ("quantile", (0, None, -1, 0, None, 0, 1, None), "SHAPE", 'R >= 0, n > 0 and draws_per_dataset > 0 dividing R are required'),
    ("quantile", (0, None, 4, 1, None, 10, 1, None), "NULL", 'params or probs is NULL'),
    ("quantile", (1, None, -1, 0, None, 0, 2, None), "PARAM", 'nddm_wiener_quantile: model 1 has no closed-form distribution function here (NDDM_BASIC_DDM_DC and NDDM_ALPHA_NOT_SCALED only)'),
    ("quantile", (0, d, 4, 3, d, 10, 2, d), "PARAM", 'nddm_wiener_quantile: flags must be 0 or NDDM_QUANTILE_CONDITIONAL'),
    ("quantile", (0, None, 4, 3, None, 10, 0, None), "SHAPE", 'R >= 0, n > 0 and draws_per_dataset > 0 dividing R are required'),
    ("quantile", (0, None, 1 << 35, 1, None, 10, 0, None), "SHAPE", 'R / 16 must be < 2^31 per launch'),
    ("quantile", (0, None, 0, 1, None, 10, 0, None), "OK", ''),
    ("quantile", (0, None, 4, 1, d, 10, 0, None), "NULL", 'params or probs is NULL'),
    ("quantile", (0, d, 4, 1, None, 10, 0, None), "NULL", 'params or probs is NULL'),
    ("log_likelihood_grad", (1, None, -1, 1, None, 0, 1, None, None), "PARAM", 'nddm_wiener_log_likelihood_grad: model 1 has no closed-form likelihood here (NDDM_BASIC_DDM_DC and NDDM_ALPHA_NOT_SCALED only)'),
    ("log_likelihood_grad", (7, d, 4, 1, d, 10, 0, d, d), "PARAM", 'nddm_wiener_log_likelihood_grad: model 7 has no closed-form likelihood here (NDDM_BASIC_DDM_DC and NDDM_ALPHA_NOT_SCALED only)'),
    ("log_likelihood_grad", (0, None, -1, 1, None, 0, 1, None, None), "PARAM", 'nddm_wiener_log_likelihood_grad: flags must be 0 (reserved)'),
    ("log_likelihood_grad", (0, None, -1, 1, None, 10, 0, None, None), "SHAPE", 'R >= 0, n_trials > 0 and draws_per_dataset > 0 dividing R are required'),
    ("log_likelihood_grad", (0, d, 4, 1, d, 0, 0, d, d), "SHAPE", 'R >= 0, n_trials > 0 and draws_per_dataset > 0 dividing R are required'),
    ("log_likelihood_grad", (0, d, 4, 0, d, 10, 0, d, d), "SHAPE", 'R >= 0, n_trials > 0 and draws_per_dataset > 0 dividing R are required'),
    ("log_likelihood_grad", (3, d, 4, 3, d, 10, 0, d, d), "SHAPE", 'R >= 0, n_trials > 0 and draws_per_dataset > 0 dividing R are required'),
    ("log_likelihood_grad", (0, None, 0, 1, None, 10, 0, None, None), "OK", ''),
    ("log_likelihood_grad", (0, None, 4, 1, d, 10, 0, d, d), "NULL", 'params or data is NULL'),
    ("log_likelihood_grad", (3, d, 4, 1, None, 10, 0, d, d), "NULL", 'params or data is NULL'),
    ("log_likelihood_grad", (0, d, 4, 1, d, 10, 0, d, None), "NULL", 'out_grad is NULL'),
    ("log_likelihood_grad", (1, None, -1, 0, None, 0, 1, None, None), "PARAM", 'nddm_wiener_log_likelihood_grad: model 1 has no closed-form likelihood here (NDDM_BASIC_DDM_DC and NDDM_ALPHA_NOT_SCALED only)'),
    ("log_likelihood_grad", (0, None, -1, 0, None, 0, 1, None, None), "PARAM", 'nddm_wiener_log_likelihood_grad: flags must be 0 (reserved)'),
    ("log_likelihood_grad", (0, d, 4, 3, d, 10, 1, d, d), "PARAM", 'nddm_wiener_log_likelihood_grad: flags must be 0 (reserved)'),
    ("log_likelihood_grad", (0, None, 4, 3, None, 10, 0, None, None), "SHAPE", 'R >= 0, n_trials > 0 and draws_per_dataset > 0 dividing R are required'),
    ("log_likelihood_grad", (0, None, 1 << 35, 1, None, 10, 0, None, None), "SHAPE", 'R / 16 must be < 2^31 per launch'),
    ("log_likelihood_grad", (0, None, 4, 1, d, 10, 0, None, None), "NULL", 'params or data is NULL'),
    ("log_likelihood_grad", (0, d, 4, 1, None, 10, 0, None, None), "NULL", 'params or data is NULL'),
    ("marginal_log_likelihood", (0, d, 4, 1, d, 10, 0, d, d), "PARAM", 'nddm_wiener_marginal_log_likelihood: model 0 has no marginal likelihood here (NDDM_SINGLE_TRIAL only)'),
    ("marginal_log_likelihood", (2, d, 4, 1, d, 10, 0, d, d), "PARAM", 'nddm_wiener_marginal_log_likelihood: model 2 has no marginal likelihood here (NDDM_SINGLE_TRIAL only)'),
    ("marginal_log_likelihood", (3, d, 4, 1, d, 10, 0, d, d), "PARAM", 'nddm_wiener_marginal_log_likelihood: model 3 has no marginal likelihood here (NDDM_SINGLE_TRIAL only)'),
    ("marginal_log_likelihood", (4, d, 4, 1, d, 10, 0, d, d), "PARAM", 'nddm_wiener_marginal_log_likelihood: model 4 has no marginal likelihood here (NDDM_SINGLE_TRIAL only)'),
    ("marginal_log_likelihood", (7, d, 4, 1, d, 10, 0, d, d), "PARAM", 'nddm_wiener_marginal_log_likelihood: model 7 has no marginal likelihood here (NDDM_SINGLE_TRIAL only)'),
    ("marginal_log_likelihood", (1, None, -1, 1, None, 0, 1, None, None), "PARAM", 'nddm_wiener_marginal_log_likelihood: flags must be 0 (reserved)'),
    ("marginal_log_likelihood", (1, None, -1, 1, None, 10, 0, None, None), "SHAPE", 'R >= 0, n_trials > 0 and draws_per_dataset > 0 dividing R are required'),
    ("marginal_log_likelihood", (1, d, 4, 1, d, 0, 0, d, d), "SHAPE", 'R >= 0, n_trials > 0 and draws_per_dataset > 0 dividing R are required'),
    ("marginal_log_likelihood", (1, d, 4, 0, d, 10, 0, d, d), "SHAPE", 'R >= 0, n_trials > 0 and draws_per_dataset > 0 dividing R are required'),
    ("marginal_log_likelihood", (1, d, 4, 3, d, 10, 0, d, d), "SHAPE", 'R >= 0, n_trials > 0 and draws_per_dataset > 0 dividing R are required'),
    ("marginal_log_likelihood", (1, None, 0, 1, None, 10, 0, None, None), "OK", ''),
    ("marginal_log_likelihood", (1, None, 4, 1, d, 10, 0, d, d), "NULL", 'params or data is NULL'),
    ("marginal_log_likelihood", (1, d, 4, 1, None, 10, 0, d, d), "NULL", 'params or data is NULL'),
    ("marginal_log_likelihood", (1, d, 4, 1, d, 10, 0, None, None), "NULL", 'no output buffer given'),
    ("marginal_log_likelihood", (0, None, -1, 0, None, 0, 1, None, None), "PARAM", 'nddm_wiener_marginal_log_likelihood: model 0 has no marginal likelihood here (NDDM_SINGLE_TRIAL only)'),
    ("marginal_log_likelihood", (1, None, -1, 0, None, 0, 1, None, None), "PARAM", 'nddm_wiener_marginal_log_likelihood: flags must be 0 (reserved)'),
    ("marginal_log_likelihood", (1, d, 4, 3, d, 10, 1, d, d), "PARAM", 'nddm_wiener_marginal_log_likelihood: flags must be 0 (reserved)'),
    ("marginal_log_likelihood", (1, None, 4, 3, None, 10, 0, None, None), "SHAPE", 'R >= 0, n_trials > 0 and draws_per_dataset > 0 dividing R are required'),
    ("marginal_log_likelihood", (1, None, 1 << 35, 1, None, 10, 0, None, None), "SHAPE", 'R / 16 must be < 2^31 per launch'),
    ("marginal_log_likelihood", (1, None, 4, 1, d, 10, 0, None, None), "NULL", 'params or data is NULL'),
    ("marginal_log_likelihood", (1, d, 4, 1, None, 10, 0, None, None), "NULL", 'params or data is NULL'),
]


@pytest.mark.parametrize("entry", ["log_likelihood", "cdf", "quantile", "log_likelihood_grad", "marginal_log_likelihood"])
def test_argument_contract_of_the_five_entry_points(entry):
    """Every status code, which check wins when two are violated, and the text of nddm_last_error(), for the shared launch path of the
    Wiener family (csrc/nddm_kernels.hip: wiener_launch).  No case reaches a HIP call."""
    from bayesflow_nddms_amd import _lib
    L = _lib.lib()
    f = getattr(L, "nddm_wiener_" + entry)
    status = {"OK": _lib.NDDM_OK, "NULL": _lib.NDDM_ERR_NULL, "SHAPE": _lib.NDDM_ERR_SHAPE, "PARAM": _lib.NDDM_ERR_PARAM}
    mine = [c for c in ARGUMENT_CASES if c[0] == entry]
    assert mine
    for _, args, want, text in mine:
        model, params, R, S, data, n, flags, *outs = [ctypes.c_void_p(16) if a is d else a for a in args]
        t_censor = (4.0,) if entry == "marginal_log_likelihood" else ()
        assert f(model, params, R, S, data, n, *t_censor, flags, *outs, None) == status[want], args
        assert L.nddm_last_error().decode() == text, args


def test_python_adapter_checks_host_inputs():
    from bayesflow_nddms_amd import engine
    from bayesflow_nddms_amd.likelihood import diffusion_lpdf, dwiener_logpdf  # noqa: F401  (exported names)
    import bayesflow_nddms_amd as pkg
    assert {"wiener_log_likelihood", "dwiener_logpdf", "diffusion_lpdf"} <= set(pkg.__all__)
    good = np.array([[1.0, 1.0, 0.5, 0.3, 1.0]])
    data = np.array([[[0.6, 1.0], [0.7, -1.0]]])
    wl = engine.wiener_log_likelihood
    with pytest.raises(ValueError, match="closed-form"):
        wl(engine.SINGLE_TRIAL, np.zeros((1, 8)), data)
    with pytest.raises(ValueError, match=r"\[R, 5\]"):
        wl(engine.BASIC_DDM_DC, np.zeros((1, 6)), data)
    for col, val, msg in ((1, 0.0, "> 0"), (4, -1.0, "> 0"), (2, 1.0, r"\(0, 1\)"), (2, 0.0, r"\(0, 1\)"), (3, -0.1, ">= 0"), (0, np.nan, "finite")):
        p = good.copy()
        p[0, col] = val
        with pytest.raises(ValueError, match=msg):
            wl(engine.BASIC_DDM_DC, p, data)
    ans = np.array([[1.0, 1.0, 0.5, 0.3, -0.2, 1.0]])
    with pytest.raises(ValueError, match="Eta"):
        wl(engine.ALPHA_NOT_SCALED, ans, data)
    with pytest.raises(ValueError, match="choice"):
        wl(engine.BASIC_DDM_DC, good, np.array([[[0.6, 0.5]]]))
    with pytest.raises(ValueError, match=r"\[D, n_trials, 2\]"):
        wl(engine.BASIC_DDM_DC, good, np.zeros((1, 3, 3)))
    with pytest.raises(ValueError, match="data sets"):
        wl(engine.BASIC_DDM_DC, np.repeat(good, 3, 0), np.repeat(data, 2, 0))
    with pytest.raises(ValueError, match="draws_per_dataset"):
        wl(engine.BASIC_DDM_DC, good, data, draws_per_dataset=0)
    with pytest.raises(ValueError, match="per_trial"):
        wl(engine.BASIC_DDM_DC, good, data, per_trial=False, want_sum=False)
