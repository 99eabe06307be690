"""CPU tests of the Wiener distribution function (nddm_wiener_cdf): the float64 yardstick (tests/wiener_cdf_ref.py) equals the integral
of the density's yardstick, the fixed-trip scheme the kernel evaluates is within 1e-6 of it, it reproduces the reference sampler's
tables, and the C ABI / Python adapter refuse bad input before any device work."""
import ctypes
import os

import numpy as np
import pytest

import wiener_cdf_ref as C
import wiener_ref as W
from conftest import GOLDEN


def _simpson_log_grid(x0, x1, n):
    """Nodes and Simpson weights of int_x0^x1 f(x) dx on a grid uniform in log x (n odd): the grid of tests/test_gpu_wiener.py."""
    s = np.linspace(np.log(x0), np.log(x1), n)
    h = s[1] - s[0]
    w = np.ones(n)
    w[1:-1:2], w[2:-1:2] = 4.0, 2.0
    x = np.exp(s)
    return x, w * h / 3.0 * x


# (a', v', w, eta', u = t / a'^2): both sides of the yardstick's switch at u = 1 and of the kernel's at 0.375, eta = 0 and eta > 0,
# the last four with eta' a' = 7.5 (the corner where a quadrature over the prior of the drift fails)
ROWS = [(0.671, -2.632, 0.771, 0.0, 0.654), (0.688, -0.669, 0.481, 0.0, 0.052), (1.969, -3.863, 0.402, 0.0, 0.442),
        (1.361, 0.868, 0.714, 0.0, 6.156), (1.068, 1.485, 0.677, 0.949, 0.020), (2.447, -2.016, 0.333, 2.686, 0.666),
        (1.443, 2.733, 0.077, 2.150, 0.188), (0.682, 1.605, 0.888, 0.701, 0.872), (1.096, 2.418, 0.700, 0.734, 2.887),
        (1.815, 1.828, 0.788, 1.343, 1.885), (2.5, -1.003, 0.602, 3.0, 0.059), (2.5, 2.522, 0.560, 3.0, 1.4),
        (2.5, -3.310, 0.918, 3.0, 0.759), (2.5, 4.870, 0.261, 3.0, 12.0)]


@pytest.mark.parametrize("a,v,w,eta,u", ROWS)
def test_yardstick_is_the_integral_of_the_density(a, v, w, eta, u):
    T = u * a * a
    x, wts = _simpson_log_grid(1e-8 * a * a, T, 40001)
    mass = float(np.sum(np.exp(W.log_f_lower(x, a, v, w, eta)) * wts))
    assert abs(float(C.F_lower(T, a, v, w, eta)) - mass) <= 1e-9


def test_choice_probability_is_the_prior_mean_of_the_fixed_drift_one():
    """P_lo with eta > 0 against a 16 001-point trapezoid rule over the drift (exponentially convergent on a Gaussian weight)."""
    rng = np.random.default_rng(3)
    n = 400
    a, v, w, eta = rng.uniform(0.5, 2.5, n), rng.uniform(-5, 5, n), rng.uniform(0.02, 0.98, n), rng.uniform(0.05, 3, n)
    z = np.linspace(-10, 10, 16001)
    wz = np.exp(-z * z / 2) / np.sqrt(2 * np.pi) * (z[1] - z[0])
    truth = C.p_lower(a[:, None], v[:, None] + eta[:, None] * z, w[:, None]) @ wz
    assert np.max(np.abs(C.P_lower(a, v, w, eta) - truth)) <= 1e-11


@pytest.mark.parametrize("basic", [False, True])
def test_shipped_scheme_is_within_1e6_of_the_yardstick(basic):
    """j <= 3 below u* = 0.375, k <= 4 and 16 Gauss-Hermite nodes at and above (csrc/nddm_wiener_cdf.h), restated in float64, over the
    domain of the device's accuracy test: 20x inside the device bar of 2e-5."""
    p32, _, up, t = C.accuracy_rows(20_000, basic)
    a, v, beta, _, s, eta = C.row_columns(p32, basic)
    ref, got = C.cdf(t, up, a, v, beta, s, eta), C.cdf(t, up, a, v, beta, s, eta, **C.SHIPPED)
    pref, pgot = C.p_upper(a, v, beta, s, eta), C.p_upper(a, v, beta, s, eta, **C.SHIPPED)
    print(f"scheme: max |F - yardstick| {np.max(np.abs(got - ref)):.3g}, max |P_up - yardstick| {np.max(np.abs(pgot - pref)):.3g}")
    assert np.all(np.isfinite(ref)) and ref.min() >= 0.0 and ref.max() <= 1.0
    assert np.max(np.abs(got - ref)) <= 1e-6 and np.max(np.abs(pgot - pref)) <= 1e-6


def test_limit_is_the_choice_probability_and_the_two_add_to_one():
    rng = np.random.default_rng(6)
    n = 200
    a, v, w = rng.uniform(0.5, 2.5, n), rng.uniform(-5, 5, n), rng.uniform(0.02, 0.98, n)
    eta = np.where(np.arange(n) % 2 == 0, 0.0, rng.uniform(0.1, 3, n))
    assert np.max(np.abs(C.F_lower(1e4 * a * a, a, v, w, eta) - C.P_lower(a, v, w, eta))) <= 1e-12
    assert np.max(np.abs(C.P_lower(a, v, w, eta) + C.P_lower(a, -v, 1.0 - w, eta) - 1.0)) <= 1e-11
    e0 = eta == 0
    pu = np.array([W.p_upper(ai, vi, wi) for ai, vi, wi in zip(a[e0], v[e0], w[e0])])
    assert np.max(np.abs(C.p_upper(a[e0], v[e0], w[e0]) - pu)) <= 1e-12
    assert np.all(C.F_lower(0.0, a, v, w, eta) == 0.0) and np.all(C.F_lower(-1.0, a, v, w, eta) == 0.0)


def test_yardstick_reproduces_the_reference_samplers_tables():
    """tests/golden/ratcliff.npz: 4001-point quantile tables of the signed RT from 2e5 reference trials per set, and P(upper)."""
    g = np.load(os.path.join(GOLDEN, "ratcliff.npz"))
    q = np.arange(4001) / 4000.0
    for i, (nu, a, beta, tau, eta, s) in enumerate(g["sets"]):
        G = C.signed_cdf(g[f"yq_s{i}"], a, nu, beta, tau, s, eta)
        d = np.max(np.abs(G - q)[1:-1])
        dp = abs(float(C.p_upper(a, nu, beta, s, eta)) - g[f"pupper_s{i}"][0])
        print(f"set {i}: max |G(yq) - q| {d:.4f}, |P_up - pupper| {dp:.4f}")
        assert d <= 0.005 and dp <= 0.005, (i, d, dp)


def test_c_abi_exports_the_entry_and_validates_before_any_hip_call():
    from bayesflow_nddms_amd import _lib
    L = _lib.lib()
    assert "nddm_wiener_cdf" in _lib.EXPORTS and hasattr(L, "nddm_wiener_cdf")
    assert L.nddm_abi_version() == _lib.ABI_VERSION == 4
    d = ctypes.c_void_p(16)
    f = L.nddm_wiener_cdf
    # (the argument checks and their order: tests/test_wiener_host.py, test_argument_contract_of_the_five_entry_points)
    import torch
    if not torch.cuda.is_available():
        assert f(0, d, 4, 2, d, 10, 0, d, None, None) in (_lib.NDDM_ERR_HIP, _lib.NDDM_ERR_NO_DEVICE)
        assert f(0, d, 4, 2, None, 10, 0, None, d, None) in (_lib.NDDM_ERR_HIP, _lib.NDDM_ERR_NO_DEVICE)   # data may be NULL without out_cdf


def test_python_adapter_checks_host_inputs():
    from bayesflow_nddms_amd import alpha_not_scaled, basic_ddm_dc, diagnostics, engine
    from bayesflow_nddms_amd.likelihood import pwiener, wiener_choice_prob  # noqa: F401  (exported names)
    import bayesflow_nddms_amd as pkg
    assert {"wiener_cdf", "pwiener", "wiener_choice_prob"} <= set(pkg.__all__)
    assert callable(basic_ddm_dc.cdf) and callable(alpha_not_scaled.cdf)
    assert callable(diagnostics.signed_cdf_analytic) and callable(diagnostics.ks_analytic)
    good = np.array([[1.0, 1.0, 0.5, 0.3, 1.0]])
    data = np.array([[[0.6, 1.0], [0.7, -1.0]]])
    wc = engine.wiener_cdf
    with pytest.raises(ValueError, match="closed-form"):
        wc(engine.SINGLE_TRIAL, np.zeros((1, 8)), data)
    with pytest.raises(ValueError, match=r"\[R, 5\]"):
        wc(engine.BASIC_DDM_DC, np.zeros((1, 6)), data)
    for col, val, msg in ((1, 0.0, "> 0"), (4, -1.0, "> 0"), (2, 1.0, r"\(0, 1\)"), (2, 0.0, r"\(0, 1\)"), (3, -0.1, ">= 0"), (0, np.nan, "finite")):
        p = good.copy()
        p[0, col] = val
        with pytest.raises(ValueError, match=msg):
            wc(engine.BASIC_DDM_DC, p, data)
    with pytest.raises(ValueError, match="Eta"):
        wc(engine.ALPHA_NOT_SCALED, np.array([[1.0, 1.0, 0.5, 0.3, -0.2, 1.0]]), data)
    with pytest.raises(ValueError, match="choice"):
        wc(engine.BASIC_DDM_DC, good, np.array([[[0.6, 0.5]]]))
    with pytest.raises(ValueError, match=r"\[D, n_trials, 2\]"):
        wc(engine.BASIC_DDM_DC, good, np.zeros((1, 3, 3)))
    with pytest.raises(ValueError, match="data sets"):
        wc(engine.BASIC_DDM_DC, np.repeat(good, 3, 0), np.repeat(data, 2, 0))
    with pytest.raises(ValueError, match="draws_per_dataset"):
        wc(engine.BASIC_DDM_DC, good, data, draws_per_dataset=0)
    with pytest.raises(ValueError, match="want_cdf"):
        wc(engine.BASIC_DDM_DC, good, data, want_cdf=False, want_p_upper=False)
    with pytest.raises(ValueError, match="split"):
        basic_ddm_dc.cdf(np.repeat(good, 3, 0), np.repeat(data, 2, 0))
