"""CPU tests of the Wiener log-likelihood (nddm_wiener_log_likelihood): the float64 yardstick pins itself against the published
identities, the fixed-trip scheme the kernel evaluates is exact to 1e-9 against it, and the C ABI / Python adapter refuse bad input
before any device work."""
import ctypes

import numpy as np
import pytest
from scipy import integrate

import wiener_ref as W

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


def test_c_abi_exports_the_entry_and_validates_before_any_hip_call():
    from bayesflow_nddms_amd import _lib
    L = _lib.lib()
    assert "nddm_wiener_log_likelihood" in _lib.EXPORTS and hasattr(L, "nddm_wiener_log_likelihood")
    assert L.nddm_abi_version() == _lib.ABI_VERSION == 4
    d = ctypes.c_void_p(16)
    f = L.nddm_wiener_log_likelihood
    # model: only the two with a closed form, named in the message
    assert f(1, d, 4, 1, d, 10, 0, d, None, None) == _lib.NDDM_ERR_PARAM and b"model 1" in L.nddm_last_error()
    assert f(7, d, 4, 1, d, 10, 0, d, None, None) == _lib.NDDM_ERR_PARAM and b"model 7" in L.nddm_last_error()
    assert f(0, d, 4, 1, d, 10, 1, d, None, None) == _lib.NDDM_ERR_PARAM                 # flags reserved
    assert f(0, None, 4, 1, d, 10, 0, d, None, None) == _lib.NDDM_ERR_NULL
    assert f(3, d, 4, 1, None, 10, 0, d, None, None) == _lib.NDDM_ERR_NULL
    assert f(0, d, 4, 1, d, 10, 0, None, None, None) == _lib.NDDM_ERR_NULL               # both outputs NULL
    assert f(0, d, -1, 1, d, 10, 0, d, None, None) == _lib.NDDM_ERR_SHAPE
    assert f(0, d, 4, 1, d, 0, 0, d, None, None) == _lib.NDDM_ERR_SHAPE
    assert f(0, d, 4, 0, d, 10, 0, d, None, None) == _lib.NDDM_ERR_SHAPE
    assert f(0, d, 4, 3, d, 10, 0, d, None, None) == _lib.NDDM_ERR_SHAPE                 # 3 does not divide 4
    assert f(0, d, 0, 1, d, 10, 0, d, None, None) == _lib.NDDM_OK                        # empty batch
    import torch
    if not torch.cuda.is_available():
        assert f(0, d, 4, 2, d, 10, 0, d, None, None) in (_lib.NDDM_ERR_HIP, _lib.NDDM_ERR_NO_DEVICE)


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
