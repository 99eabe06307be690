"""CPU tests of the Wiener log-likelihood's gradient (nddm_wiener_log_likelihood_grad; csrc/nddm_wiener_grad.h): the float64 yardstick
(tests/wiener_grad_ref.py) pins itself against finite differences of wiener_ref.log_f, the fixed-trip sums the header evaluates are exact to
3e-10 in the derivative ratios, the header's own per-trial code and chain rule compiled for the host meet the bar B on the priors' rows and
give the special values, and the C ABI / Python adapter refuse bad input before any device work."""
import ctypes
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import pytest

import wiener_grad_ref as G
import wiener_ref as W
from conftest import ROOT
from test_wiener_host import U_GRID, W_GRID

HAVE_CXX = not (shutil.which("g++") is None and shutil.which("c++") is None and shutil.which("clang++") is None)


def _richardson(f, x, j, h):
    """Central difference of f in column j at step h and h / 2, extrapolated: error O(h^4)."""
    def cd(step):
        hi, lo = x.copy(), x.copy()
        hi[:, j] += step
        lo[:, j] -= step
        return (f(hi) - f(lo)) / (2.0 * step)
    return (4.0 * cd(0.5 * h) - cd(h)) / 3.0


def _fd_grid(basic):
    rows = []
    for up in (False, True):
        for u in np.geomspace(1e-3, 50.0, 13):
            for w in (0.01, 0.2, 0.5, 0.8, 0.99):
                for eta in ((0.0,) if basic else (0.0, 0.5, 2.0)):
                    for s in (0.5, 1.0, 2.0):
                        for v in (0.8, -2.1):
                            a, tau = 1.3, 0.25
                            beta = 1.0 - w if up else w
                            rows.append(([v, a, beta, tau, s] if basic else [v, a, beta, tau, eta, s]) + [tau + u * (a / s) ** 2, float(up)])
    r = np.array(rows)
    return r[:, :-2].copy(), r[:, -2].copy(), r[:, -1] > 0


@pytest.mark.parametrize("basic", [True, False], ids=["basic_ddm_dc", "alpha_not_scaled"])
def test_yardstick_equals_finite_differences_of_log_f(basic):
    """Both boundaries, u in [1e-3, 50], w in [0.01, 0.99], eta in {0, 0.5, 2}, s in {0.5, 1, 2}: every parameter column of
    wiener_grad_ref.trial_grad against Richardson-extrapolated central differences (relative step 1e-5) of wiener_ref.log_f in float64,
    to 1e-6 of max(1, |value|)."""
    p, rt, up = _fd_grid(basic)
    got = G.trial_grad(basic, p, rt - p[:, 3], up)
    assert np.all(np.isfinite(got))
    worst = 0.0
    for j in range(p.shape[1]):
        h = 1e-5 * np.where(p[:, j] == 0.0, 1.0, np.abs(p[:, j]))      # (eta = 0: log f is even in eta, the difference straddles 0)
        fd = _richardson(lambda x: G.log_f_of_params(basic, x, rt, up), p, j, h)
        err = np.abs(got[:, j] - fd) / np.maximum(1.0, np.abs(got[:, j]))
        worst = max(worst, float(err.max()))
        assert err.max() <= 1e-6, (G.COLUMNS[basic][j], float(err.max()), p[np.argmax(err)])
    print(f"{p.shape[0]} points x {p.shape[1]} columns: max |analytic - finite difference| / max(1, |value|) = {worst:.3g}")
    assert np.any(np.abs(got[:, 0]) > 1.0) and np.any(np.abs(got[:, 3]) > 100.0)       # (not a grid of zeros)


def test_clipped_nu_has_the_clamps_derivative():
    p = np.array([[7.0, 1.2, 0.4, 0.2, 0.7, 1.1], [5.0, 1.2, 0.4, 0.2, 0.7, 1.1], [-6.0, 1.2, 0.4, 0.2, 0.7, 1.1], [-5.0, 1.2, 0.4, 0.2, 0.7, 1.1]])
    g = G.trial_grad(False, p, 0.5, np.array([True, True, False, False]))
    assert np.all(g[[0, 2], 0] == 0.0) and np.all(g[[1, 3], 0] != 0.0)
    assert np.array_equal(g[0, 1:], g[1, 1:]) and np.array_equal(g[2, 1:], g[3, 1:])


def test_fixed_trip_derivative_ratios_are_exact_to_3e10():
    """The header's scheme in float64 -- 5 small-time terms below u* = 0.375, 3 large-time terms at and above -- against the 60 / 200-term
    sums, both partials of log g, on the density test's grid and densely over the crossover band.  Measured: 1.7e-10 (d/du) and 3.2e-11
    (d/dw) of max(1, |value|) on the grid, 2.3e-10 and 4.5e-11 on the band; asserted: 3e-10."""
    for u in (U_GRID, np.linspace(0.30, 0.50, 201)[:, None]):
        ref, ft = G.dlog_g(u, W_GRID), G.dlog_g_fixed_trip(u, W_GRID)
        for r, f, name in zip(ref, ft, ("d/du", "d/dw")):
            err = np.max(np.abs(f - r) / np.maximum(1.0, np.abs(r)))
            print(f"{name} over {u.size} x {W_GRID.size}: {err:.3g}")
            assert err <= 3e-10, name
    # the two full series are one function where both can be summed
    u = np.geomspace(0.1, 2.0, 200)[:, None]
    for s, l in zip(G.dlog_g_small(u, W_GRID), G.dlog_g_large(u, W_GRID)):
        assert np.max(np.abs(s - l) / np.maximum(1.0, np.abs(s))) < 1e-10


@pytest.fixture(scope="module")
def host():
    """(module of tools/wiener_grad_host.py, its program built without a sanitizer, a scratch directory)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import wiener_grad_host as GH
    with tempfile.TemporaryDirectory() as td:
        yield GH, GH.build(td), td


@pytest.mark.skipif(not HAVE_CXX, reason="no host C++ compiler")
def test_header_compiled_for_the_host_meets_the_bar_on_the_priors(host):
    """tools/wiener_grad_host.py over wiener_cdf_ref.prior_rows, 20 000 rows of each model, one trial per row with u in [1e-3, 50]: per
    column |gradient - yardstick| <= B scale_j, every row used (the yardstick and the header are finite on all of them).  B = 0.07 is 4 x
    the largest error measured with this tool, 0.0152 (basic_ddm_dc's tau column, a trial where d/dt log g = 1.3055 and the drift's
    v'^2 / 2 = 1.3052 cancel to 4.0e-4: with ONE trial per row scale_j is the derivative itself, and a zero crossing of it is where
    float32 has no relative accuracy), rounded up to one significant digit; the 99th percentile over the rows is 5e-6 at the most.
    profiles/r12_wiener_grad_host.json is this survey's output."""
    GH = host[0]
    r = GH.survey(sanitize=False)
    for name, c in r["cases"].items():
        print(name, c)
        assert c["rows"] == c["yardstick_finite_rows"] == c["header_finite_rows"] == 20_000, name      # no row left out
        for col, e in c["max_err_over_scale"].items():
            assert e <= G.BAR_B, (name, col, e)
    tracked = json.load(open(os.path.join(ROOT, "profiles", "r12_wiener_grad_host.json")))
    assert tracked["bar_B"] == G.BAR_B and G.BAR_B == GH.round_up_1sd(4.0 * tracked["max_err_over_scale"])


def _rows_of_trials(GH, exe, td, basic, p, trials):
    return GH.evaluate(exe, td, 0 if basic else 3, np.asarray(p, np.float32), np.asarray(trials, np.float32))


@pytest.mark.skipif(not HAVE_CXX, reason="no host C++ compiler")
def test_special_values_on_the_host(host):
    GH, exe, td = host
    good = [0.8, 1.2, 0.45, 0.2, 1.1]
    tr = [[0.6, 1.0], [0.9, -1.0], [1.4, 1.0]]
    # rows: plain; one censored trial (choice 0); one trial at rt <= tau; invalid rows (a = 0, beta = 1, NaN drift) between valid ones
    P = np.array([good, good, good, [0.8, 0.0, 0.45, 0.2, 1.1], good, [0.8, 1.2, 1.0, 0.2, 1.1], [np.nan, 1.2, 0.45, 0.2, 1.1], good])
    D = np.array([tr, [tr[0], [1.1, 0.0], tr[2]], [tr[0], [0.2, -1.0], tr[2]], tr, tr, tr, tr, tr])
    ll, g = _rows_of_trials(GH, exe, td, True, P, D)
    plain = [0, 4, 7]
    assert np.all(np.isfinite(ll[plain])) and np.all(np.isfinite(g[plain]))
    assert np.array_equal(ll[plain], np.repeat(ll[0], 3)) and np.array_equal(g[plain], np.tile(g[0], (3, 1)))       # neighbours unaffected
    ref, scale = G.row_grad(True, np.float32(P[:1]).astype(np.float64), (np.float32(D[:1, :, 0]) - np.float32(0.2)).astype(np.float64), D[:1, :, 1] > 0)
    assert np.all(np.abs(g[0] - ref[0]) <= 1e-5 * scale[0])
    # censored: the value is the uncensored trials' plus log S of the censored one (tools/wiener_host.py: wiener_trial), the gradient NaN
    import wiener_host as H
    with tempfile.TemporaryDirectory() as td2:
        lf = H.evaluate(H.build(td2), td2, 0, np.tile(np.float32(good), (3, 1)), np.float32(D[1]))[0]
    assert np.isfinite(ll[1]) and lf[1] < 0 and abs(ll[1] - np.cumsum(lf)[-1]) <= 1e-12 * abs(ll[1])
    assert np.all(np.isnan(g[1]))
    assert ll[2] == -np.inf and np.all(np.isnan(g[2]))                   # rt <= tau
    for i in (3, 5, 6):
        assert np.isnan(ll[i]) and np.all(np.isnan(g[i])), i
    # alpha_not_scaled: |Nu| > 5 has d/dNu == 0 and the other columns of Nu = +-5; y == 0 is NaN in both
    A = np.array([[7.0, 1.0, 0.5, 0.2, 0.5, 1.3], [5.0, 1.0, 0.5, 0.2, 0.5, 1.3], [-9.0, 1.0, 0.5, 0.2, 0.0, 1.3], [-5.0, 1.0, 0.5, 0.2, 0.0, 1.3],
                  [1.0, 1.0, 0.5, 0.2, 0.5, 1.3], [7.0, 1.0, 0.5, 0.2, 0.5, 1.3]])
    y = np.array([0.5, -0.7, 1.1])
    Dy = np.tile(np.stack([y, (np.sign(y) + 1) / 2], -1), (6, 1, 1))
    Dy[4:, 1, 0] = 0.0
    ll, g = _rows_of_trials(GH, exe, td, False, A, Dy)
    assert g[0, 0] == 0.0 and g[2, 0] == 0.0 and g[1, 0] != 0.0 and g[3, 0] != 0.0
    assert np.array_equal(g[0, 1:], g[1, 1:]) and np.array_equal(g[2, 1:], g[3, 1:]) and ll[0] == ll[1] and ll[2] == ll[3]
    assert np.all(np.isfinite(g[:4])) and g[3, 4] == 0.0                # (eta = 0: log f is even in eta)
    assert np.all(np.isnan(ll[4:])) and np.all(np.isnan(g[4:]))         # (the clipped row's Nu column too)


def test_c_abi_exports_the_entry_and_validates_before_any_hip_call():
    from bayesflow_nddms_amd import _lib
    L = _lib.lib()
    assert "nddm_wiener_log_likelihood_grad" in _lib.EXPORTS and hasattr(L, "nddm_wiener_log_likelihood_grad")
    assert L.nddm_abi_version() == _lib.ABI_VERSION == 4
    d = ctypes.c_void_p(16)
    f = L.nddm_wiener_log_likelihood_grad
    # (the argument checks and their order: tests/test_wiener_host.py, test_argument_contract_of_the_five_entry_points)
    hdr = open(os.path.join(ROOT, "include", "nddm.h")).read()
    assert "int nddm_wiener_log_likelihood_grad(" in hdr and "NOT IMPLEMENTED: the gradient of basic_ddm_dc's censored timeouts" in hdr
    from bayesflow_nddms_amd import build
    assert any(p.endswith("nddm_wiener_grad.h") for p in build.HEADERS)                  # part of the source hash
    import torch
    if not torch.cuda.is_available():
        assert f(0, d, 4, 2, d, 10, 0, None, d, None) in (_lib.NDDM_ERR_HIP, _lib.NDDM_ERR_NO_DEVICE)      # (out_loglik may be NULL)


def test_python_adapter_checks_host_inputs():
    from bayesflow_nddms_amd import alpha_not_scaled, basic_ddm_dc, engine, likelihood
    import bayesflow_nddms_amd as pkg
    assert {"wiener_log_likelihood_grad", "wiener_loglik"} <= set(pkg.__all__)
    good = np.array([[1.0, 1.0, 0.5, 0.3, 1.0]])
    data = np.array([[[0.6, 1.0], [0.7, -1.0]]])
    for wl in (engine.wiener_log_likelihood_grad, likelihood.wiener_loglik):
        with pytest.raises(ValueError, match="closed-form"):
            wl(engine.SINGLE_TRIAL, np.zeros((1, 8)), data)
        with pytest.raises(ValueError, match=r"\[R, 5\]"):
            wl(engine.BASIC_DDM_DC, np.zeros((1, 6)), data)
        for col, val, msg in ((1, 0.0, "> 0"), (4, -1.0, "> 0"), (2, 1.0, r"\(0, 1\)"), (2, 0.0, r"\(0, 1\)"), (3, -0.1, ">= 0"), (0, np.nan, "finite")):
            p = good.copy()
            p[0, col] = val
            with pytest.raises(ValueError, match=msg):
                wl(engine.BASIC_DDM_DC, p, data)
        with pytest.raises(ValueError, match="Eta"):
            wl(engine.ALPHA_NOT_SCALED, np.array([[1.0, 1.0, 0.5, 0.3, -0.2, 1.0]]), data)
        with pytest.raises(ValueError, match="choice"):
            wl(engine.BASIC_DDM_DC, good, np.array([[[0.6, 0.5]]]))
        with pytest.raises(ValueError, match=r"\[D, n_trials, 2\]"):
            wl(engine.BASIC_DDM_DC, good, np.zeros((1, 3, 3)))
        with pytest.raises(ValueError, match="data sets"):
            wl(engine.BASIC_DDM_DC, np.repeat(good, 3, 0), np.repeat(data, 2, 0))
        with pytest.raises(ValueError, match="draws_per_dataset"):
            wl(engine.BASIC_DDM_DC, good, data, draws_per_dataset=0)
    with pytest.raises(ValueError, match="cannot be split"):
        basic_ddm_dc.log_likelihood_and_grad(np.repeat(good, 3, 0), np.repeat(data, 2, 0))
    with pytest.raises(ValueError, match="cannot be split"):
        alpha_not_scaled.log_likelihood_and_grad(np.ones((3, 6)), np.ones((2, 4)))
    for doc in (engine.wiener_log_likelihood_grad.__doc__, likelihood.wiener_loglik.__doc__, basic_ddm_dc.log_likelihood_and_grad.__doc__):
        assert "NOT IMPLEMENTED" in doc and "censored" in doc
