"""CPU tests of the single-trial model's marginal log-likelihood (nddm_wiener_marginal_log_likelihood; csrc/nddm_wiener_marginal.h): the
float64 yardstick (tests/wiener_marginal_ref.py) pins itself against scipy.integrate.quad, its two closed-form limits and the total mass;
the shipped quadrature restated in float64 stays within 1e-6 of it on the prior's rows and finite on the box; the header's own per-trial
code compiled for the host meets the recorded float32 figures and gives the special values; the C ABI and the Python adapter refuse bad
input before any device work, and the four closed-form entry points still refuse this model."""
import ctypes
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import pytest
from scipy import integrate
from scipy.special import log_ndtr
from scipy.stats import norm

import wiener_marginal_ref as M
import wiener_ref as W
from conftest import ROOT

HAVE_CXX = not (shutil.which("g++") is None and shutil.which("c++") is None and shutil.which("clang++") is None)
N_HOST = 300              # rows of each set the host program is run on here (the survey behind the recorded figures: 1500)


def _one(p, y, z, tc):
    return float(M.log_lik(np.asarray(p, np.float64)[None], np.array([y], np.float64), np.array([z], np.float64), tc)[0])


def _quad_log_lik(p, y, z, tc):
    """log L of one trial by scipy.integrate.quad in a (not in log a), breakpoints at m and at h's own peak, the largest log integrand on a
    grid taken out."""
    p = np.asarray(p, np.float64)[None]
    t, code = M.trial_parts(p, np.array([y]), tc)
    m, tau, outside = M.gaussian_parts(p, np.array([z]))
    li = lambda a: (M.log_h(np.atleast_1d(a), np.broadcast_to(t, np.shape(np.atleast_1d(a))), np.broadcast_to(code, np.shape(np.atleast_1d(a))),
                            *(np.broadcast_to(p[:, j], np.shape(np.atleast_1d(a))) for j in (0, 2, 5)))
                    - (np.atleast_1d(a) - m) ** 2 / (2.0 * tau ** 2) - np.log(tau) - 0.5 * np.log(2.0 * np.pi))
    grid = np.geomspace(1e-4, 200.0, 6000)
    lg = li(grid)
    top = lg.max()
    lh = M.log_h(grid, np.broadcast_to(t, grid.shape), np.broadcast_to(code, grid.shape), *(np.broadcast_to(p[:, j], grid.shape) for j in (0, 2, 5)))
    band = grid[lg >= top - 50.0]
    lo, hi = band[0] * 0.9, band[-1] * 1.1
    pts = sorted({float(x) for x in (m[0], grid[np.argmax(lg)], grid[np.argmax(lh)]) if lo < x < hi})
    val, err = integrate.quad(lambda a: float(np.exp(li(a)[0] - top)), lo, hi, points=pts or None, limit=400, epsabs=0.0, epsrel=1e-11)
    return float(outside[0] + top + np.log(val))


def test_yardstick_agrees_with_scipy_quad():
    """30 rows: the first 12 of prior_rows, its first 3 censored ones, the first 12 of box and 3 censored ones of it.  quad integrates in a over
    the band where the integrand is within e^-50 of its largest value; the yardstick in log a.  To 1e-8."""
    worst = 0.0
    for name, rows in M.SETS.items():
        p32, y32, z32, tc = rows(M.POOL)
        cens = np.flatnonzero(y32 == 0)[:3]
        assert cens.size == 3, name
        for i in list(range(12)) + list(cens):
            p, y, z = M.as_f64(p32[i:i + 1], y32[i:i + 1], z32[i:i + 1])
            ref, q = _one(p[0], y[0], z[0], tc), _quad_log_lik(p[0], y[0], z[0], tc)
            worst = max(worst, abs(ref - q))
            assert abs(ref - q) <= 1e-8, (name, i, ref, q)
    print(f"30 rows: max |yardstick - quad| = {worst:.3g}")


LIMIT_ROWS = [([1.2, 1.4, 0.45, 0.25, 0.5, 0.9, None, 1.0], 0.85, 1.5), ([-0.8, 1.0, 0.6, 0.3, 0.4, 1.1, None, 2.0], -0.9, 2.3),
              ([0.5, 1.8, 0.3, 0.2, 0.7, 0.8, None, 0.5], 1.4, 0.8)]


def test_sigma1_to_zero_limit():
    """z pins the boundary at a = z / gamma: log L -> log TN(z / gamma; mu, sd) - log gamma + log f_W(y | a = z / gamma), the difference
    second order in sigma1 (the Gaussian N(a; m, tau^2) tightens symmetrically around z / gamma): halving sigma1 quarters it."""
    for row, y, z in LIMIT_ROWS:
        drift, mu, beta, ter, sd, dc, _, g = row
        a = z / g
        lim = norm.logpdf(a, mu, sd) - log_ndtr(mu / sd) - np.log(g) + float(W.log_f(abs(y) - ter, y > 0, a, drift, beta, dc))
        d = []
        for s1 in (0.04, 0.02, 0.01):
            p = list(row)
            p[6] = s1 * g                                               # (tau = sigma1 / gamma to first order: the same tightness for every gamma)
            d.append(_one(p, y, z, None) - lim)
        print(row, d)
        assert 3.8 <= d[0] / d[1] <= 4.2 and 3.8 <= d[1] / d[2] <= 4.2, d      # second order, so the limit is the limit


def test_std_alpha_to_zero_limit():
    """The boundary is mu_alpha: log L -> log N(z; gamma mu, sigma1^2) + log f_W(y | a = mu); second order in std_alpha as well."""
    for row, y, z in LIMIT_ROWS:
        drift, mu, beta, ter, _, dc, _, g = row
        s1 = 0.6
        lim = norm.logpdf(z, g * mu, s1) + float(W.log_f(abs(y) - ter, y > 0, mu, drift, beta, dc))
        d = []
        for sd in (0.04, 0.02, 0.01):
            p = list(row)
            p[4], p[6] = sd, s1
            d.append(_one(p, y, z, None) - lim)
        print(row, d)
        assert 3.8 <= d[0] / d[1] <= 4.2 and 3.8 <= d[1] / d[2] <= 4.2, d      # second order, so the limit is the limit


def test_mass_ties_the_censored_branch_to_the_response_branch():
    """With gamma = 0 the datum z ~ N(0, sigma1^2) says nothing about the boundary, so L / N(z; 0, sigma1^2) is the response-time law with
    the boundary integrated over its prior: its integral over both boundaries up to t_censor plus the censored term is 1."""
    tc = 1.5
    for row in ([1.0, 1.3, 0.4, 0.2, 0.5, 1.0, 0.7, 0.0], [-0.5, 1.6, 0.55, 0.3, 0.3, 0.7, 1.2, 0.0]):
        p, z = np.array(row), 0.3
        lz = norm.logpdf(z, 0.0, row[6])
        # a boundary near 0 ends its trial at once: the law's density grows as t^-1/2 toward t = 0, so the panels are geometric in t; the
        # mass below 1e-16 s is that of a boundary below about 1e-8, under 1e-8
        g, wt = np.polynomial.legendre.leggauss(16)
        edges = np.geomspace(1e-16, tc, 41)
        t = np.concatenate([0.5 * (b + a) + 0.5 * (b - a) * g for a, b in zip(edges[:-1], edges[1:])])
        w = np.concatenate([0.5 * (b - a) * wt for a, b in zip(edges[:-1], edges[1:])])
        y = np.concatenate([row[3] + t, -(row[3] + t)])
        dens = np.exp(M.log_lik(np.tile(p, (y.size, 1)), y, np.full(y.size, z), tc) - lz)
        mass = float(np.sum(np.concatenate([w, w]) * dens))
        cens = float(np.exp(_one(p, 0.0, z, tc) - lz))
        print(f"{row}: responses {mass:.10f} + censored {cens:.10f} = {mass + cens:.10f}")
        assert 0.01 < cens < 0.99 and abs(mass + cens - 1.0) <= 1e-7


def test_scheme_in_float64_within_1e6_on_the_prior_and_finite_on_the_box():
    """The shipped rule (hull window, two zooms, 32-node sum) restated in float64 on N_HOST rows of each set.  Measured on 1500 rows: 1.5e-7
    on prior_rows and 2.6e-7 on box (profiles/r13_wiener_marginal_host.json)."""
    for name, rows in M.SETS.items():
        p32, y32, z32, tc = rows(N_HOST)
        p, y, z = M.as_f64(p32, y32, z32)
        ref, sch = M.log_lik(p, y, z, tc), M.scheme_log_lik(p, y, z, tc)
        assert np.all(np.isfinite(ref)), name                           # no row left out: the yardstick scores every one
        err = np.abs(sch - ref)
        print(f"{name}: {N_HOST} rows, {int((y32 == 0).sum())} censored, max |scheme - yardstick| = {err.max():.3g}")
        assert np.all(np.isfinite(sch)), name
        if name == "prior_rows":
            assert err.max() <= 1e-6


@pytest.fixture(scope="module")
def host():
    """(module of tools/wiener_marginal_host.py, its program built without a sanitizer, a scratch directory)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import wiener_marginal_host as MH
    with tempfile.TemporaryDirectory() as td:
        yield MH, MH.build(td), td


@pytest.mark.skipif(not HAVE_CXX, reason="no host C++ compiler")
def test_header_compiled_for_the_host_meets_the_recorded_figures(host):
    """The header's float32 on the first N_HOST rows of each set stays within the largest error of the 1500-row survey
    (profiles/r13_wiener_marginal_host.json, the tool's own output), which the device bars are 4 x of."""
    MH, exe, td = host
    tracked = json.load(open(os.path.join(ROOT, "profiles", "r13_wiener_marginal_host.json")))
    assert tracked["sanitized"] and tracked["rows_per_set"] == M.POOL
    for name, rows in M.SETS.items():
        p32, y32, z32, tc = rows(N_HOST)
        got = MH.evaluate(exe, td, p32, np.stack([y32, z32], 1)[:, None, :], tc)[:, 0].astype(np.float64)
        ref = M.log_lik(*M.as_f64(p32, y32, z32), tc)
        err = np.abs(got - ref)
        c = tracked["cases"][name]
        print(f"{name}: max |float32 - yardstick| = {err.max():.3g} (recorded on {c['rows']} rows: {c['max_abs_err_float32']:.3g})")
        assert np.all(np.isfinite(got)) and c["finite"] == c["rows"] == M.POOL
        assert err.max() <= c["max_abs_err_float32"]
        assert M.DEVICE_BAR[name] == c["device_bar"] == MH.round_up_1sd(4.0 * c["max_abs_err_float32"])
        assert c["max_abs_err_scheme_float64"] <= 1e-6


@pytest.mark.skipif(not HAVE_CXX, reason="no host C++ compiler")
def test_special_values_on_the_host(host):
    MH, exe, td = host
    good = [0.8, 1.2, 0.45, 0.2, 0.5, 1.1, 0.7, 1.0]
    bad = [dict(col=4, val=0.0), dict(col=6, val=-1.0), dict(col=5, val=0.0), dict(col=2, val=1.0), dict(col=2, val=0.0), dict(col=3, val=-0.1),
           dict(col=0, val=np.nan), dict(col=7, val=np.inf)]
    P = [good]
    for b in bad:
        r = list(good)
        r[b["col"]] = b["val"]
        P += [r, good]
    tr = [[0.6, 1.0], [-0.9, 1.4], [0.0, 1.1], [0.15, 1.0], [0.7, np.nan], [0.7, np.inf], [0.2, 1.0]]
    out = MH.evaluate(exe, td, np.array(P), np.tile(np.array(tr), (len(P), 1, 1)), 2.0)
    assert np.all(np.isnan(out[1::2]))                                  # every invalid row, every trial
    assert np.array_equal(out[0::2], np.tile(out[0], (len(bad) + 1, 1)), equal_nan=True)      # neighbours unaffected
    v = out[0]
    assert np.all(np.isfinite(v[:3])) and v[2] < 0                      # two responses and a timeout with t_censor
    assert v[3] == -np.inf and v[6] == -np.inf                          # |y| < ter, |y| == ter
    assert np.isnan(v[4]) and np.isnan(v[5])                            # non-finite z1
    ref = M.pairs_log_lik(np.float32([good]), np.float32([[0.6, -0.9, 0.0]]), np.float32([[1.0, 1.4, 1.1]]), 2.0)[0]
    assert np.all(np.abs(v[:3] - ref) <= M.DEVICE_BAR["prior_rows"])
    for tc in (0.0, -1.0, float("nan")):                                # a timeout without a censoring time
        o = MH.evaluate(exe, td, np.array([good]), np.array([[tr[0], tr[2]]]), tc)[0]
        assert o[0] == v[0] and np.isnan(o[1])


def test_c_abi_exports_the_entry_and_validates_before_any_hip_call():
    from bayesflow_nddms_amd import _lib
    L = _lib.lib()
    assert "nddm_wiener_marginal_log_likelihood" in _lib.EXPORTS and hasattr(L, "nddm_wiener_marginal_log_likelihood")
    assert L.nddm_abi_version() == _lib.ABI_VERSION == 4
    f = L.nddm_wiener_marginal_log_likelihood
    assert f.argtypes[6] is ctypes.c_float and f.argtypes[7] is ctypes.c_uint32 and len(f.argtypes) == 11
    d = ctypes.c_void_p(16)
    # (the argument checks and their order: tests/test_wiener_host.py, test_argument_contract_of_the_five_entry_points)
    hdr = open(os.path.join(ROOT, "include", "nddm.h")).read()
    assert "int nddm_wiener_marginal_log_likelihood(" in hdr and "#define NDDM_ABI_VERSION 4" in hdr
    assert "NDDM_SINGLE_TRIAL_ALT (a latent diffusion coefficient) is OUT OF" in hdr
    for name in ("nddm_wiener_log_likelihood.  No existing entry point changes.", "nddm_wiener_cdf.  No existing entry point changes.",
                 "nddm_wiener_quantile.", "nddm_wiener_log_likelihood_grad.  No existing entry point changes.",
                 "nddm_wiener_marginal_log_likelihood.  No existing entry point changes."):
        assert f"/* 4 (additive): {name} */" in hdr, name
    from bayesflow_nddms_amd import build
    assert any(p.endswith("nddm_wiener_marginal.h") for p in build.HEADERS)              # part of the source hash
    import torch
    if not torch.cuda.is_available():
        assert f(1, d, 4, 2, d, 10, 4.0, 0, None, d, None) in (_lib.NDDM_ERR_HIP, _lib.NDDM_ERR_NO_DEVICE)      # (out_trial may be NULL)


def test_python_adapter_checks_host_inputs():
    from bayesflow_nddms_amd import engine, likelihood, single_trial_alpha_not_scaled as st
    import bayesflow_nddms_amd as pkg
    assert {"wiener_marginal_log_likelihood", "single_trial_logpdf"} <= set(pkg.__all__)
    good = np.array([[0.8, 1.2, 0.45, 0.2, 0.5, 1.1, 0.7, 1.0]])
    data = np.array([[[0.6, 1.0], [-0.7, 1.3]]])
    wl = engine.wiener_marginal_log_likelihood
    for model, P in ((engine.BASIC_DDM_DC, 5), (engine.ALPHA_NOT_SCALED, 6), (engine.SINGLE_TRIAL_ALT, 8), (engine.EXPLICIT_BOUNDARY, 4)):
        with pytest.raises(ValueError, match="SINGLE_TRIAL only"):
            wl(model, np.ones((1, P)), data)
    with pytest.raises(ValueError, match=r"\[R, 8\]"):
        wl(engine.SINGLE_TRIAL, np.ones((1, 7)), data)
    for col, val, msg in ((4, 0.0, "> 0"), (6, -1.0, "> 0"), (5, 0.0, "> 0"), (2, 1.0, r"\(0, 1\)"), (2, 0.0, r"\(0, 1\)"), (3, -0.1, ">= 0"),
                          (0, np.nan, "finite"), (7, np.inf, "finite")):
        p = good.copy()
        p[0, col] = val
        with pytest.raises(ValueError, match=msg):
            wl(engine.SINGLE_TRIAL, p, data)
    with pytest.raises(ValueError, match=r"\[D, n_trials, 2\]"):
        wl(engine.SINGLE_TRIAL, good, np.zeros((1, 3, 3)))
    with pytest.raises(ValueError, match="data sets"):
        wl(engine.SINGLE_TRIAL, np.repeat(good, 3, 0), np.repeat(data, 2, 0))
    with pytest.raises(ValueError, match="draws_per_dataset"):
        wl(engine.SINGLE_TRIAL, good, data, draws_per_dataset=0)
    with pytest.raises(ValueError, match="ask for"):
        wl(engine.SINGLE_TRIAL, good, data, per_trial=False, want_sum=False)
    for tc in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="t_censor"):
            wl(engine.SINGLE_TRIAL, good, data, t_censor=tc)
    with pytest.raises(ValueError, match="> 0"):
        st.log_likelihood(np.array([0.8, 1.2, 0.45, 0.2, 0.0, 1.1, 0.7]), data[0])
    assert "t_censor" in likelihood.single_trial_logpdf.__doc__ and "max_steps" in st.log_likelihood.__doc__


def test_closed_form_entry_points_still_refuse_the_single_trial_model():
    from bayesflow_nddms_amd import engine
    data = np.array([[[0.6, 1.0], [0.7, -1.0]]])
    for model in (engine.SINGLE_TRIAL, engine.SINGLE_TRIAL_ALT):
        for fn in (engine.wiener_log_likelihood, engine.wiener_cdf, engine.wiener_quantile, engine.wiener_log_likelihood_grad):
            with pytest.raises(ValueError, match="closed-form"):
                fn(model, np.ones((1, 8)), data)
