"""CPU tests of NDDM_WIENER_CENSORED in the Wiener log-likelihood's gradient (nddm_wiener_log_likelihood_grad; csrc/nddm_wiener_grad.h:
wiener_grad_censored): the float64 yardstick (tests/wiener_censored_ref.py) pins itself against central differences of log S across the
header's small / large crossover, the header's own code compiled for the host meets the bar on rows with 10 % timeouts and gives the
special values, the flag is neutral where nothing is censored, one run under AddressSanitizer and UndefinedBehaviorSanitizer, and the C
ABI / Python adapters accept the flag where it applies and refuse it where it does not."""
import ctypes
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import pytest

import wiener_cdf_ref as C
import wiener_censored_ref as R
import wiener_grad_ref as G
from conftest import ROOT

HAVE_CXX = not (shutil.which("g++") is None and shutil.which("c++") is None and shutil.which("clang++") is None)
SURV_U = 0.06             # WIENER_SURV_U: the header's images below, its series at and above


def _crossover_grid():
    rows = []
    for u in np.concatenate([np.geomspace(5e-3, 8.0, 12), [0.05, 0.059, 0.061, 0.07]]):
        for beta in (0.1, 0.5, 0.85):
            for s in (0.6, 1.0, 1.7):
                for v in (0.0, 0.9, -2.3):
                    a, tau = 1.4, 0.22
                    rows.append([v, a, beta, tau, s, tau + u * (a / s) ** 2])
    r = np.array(rows)
    return r[:, :5].copy(), r[:, 5].copy()


def test_yardstick_equals_central_differences_of_log_s():
    """u in [5e-3, 8] with points on either side of WIENER_SURV_U, beta in {.1, .5, .85}, s in {.6, 1, 1.7}, drift in {0, .9, -2.3}: every
    column of wiener_censored_ref.timeout_grad -- a's from the scaling identity, tau's from (f_lower + f_upper) / S -- against
    Richardson-extrapolated central differences (relative step 2e-3) of the float64 log S, to 1e-6 of max(1, |value|), where S >= 1e-3."""
    p, rt = _crossover_grid()
    _, ok = R.log_survival(p, rt - p[:, 3])
    p, rt = p[ok], rt[ok]
    u = (rt - p[:, 3]) / (p[:, 1] / p[:, 4]) ** 2
    assert np.any(u < SURV_U) and np.any(u >= SURV_U) and p.shape[0] > 300
    got = R.timeout_grad(p, rt - p[:, 3])
    fd = R.fd_timeout_grad(p, rt)
    assert np.all(np.isfinite(got))
    err = np.abs(got - fd) / np.maximum(1.0, np.abs(got))
    print(f"{p.shape[0]} points x 5 columns: max |yardstick - finite difference| / max(1, |value|) per column {np.array2string(err.max(0), precision=2)}")
    assert np.all(err <= 1e-6), err.max(0)
    assert np.all(got[:, 3] >= 0.0) and np.any(got[:, 3] > 1.0) and np.any(np.abs(got[:, 1]) > 1.0)      # (not a grid of zeros)
    # t <= 0: log 1 = 0 with a zero gradient
    assert np.all(R.timeout_grad(p[:3], np.array([0.0, -0.1, -3.0])) == 0.0)


@pytest.fixture(scope="module")
def host():
    """(module of tools/wiener_grad_host.py, its program built without a sanitizer, a scratch directory)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import wiener_grad_host as GH
    with tempfile.TemporaryDirectory() as td:
        yield GH, GH.build(td), td


@pytest.mark.skipif(not HAVE_CXX, reason="no host C++ compiler")
def test_header_compiled_for_the_host_meets_the_bar_with_timeouts(host):
    """tools/wiener_grad_host.py's censored survey on the first 300 / 300 / 150 rows of prior_1s, prior_4s and box, 160 trials per row, 16
    of them timeouts at the set's times: per column |gradient - yardstick| <= BAR scale_j.  The whole survey (5000 / 5000 / 2000 rows) is
    profiles/r22_wiener_censored_host.json: its largest error is within wiener_grad_ref.BAR_B, so by the rule the bar is BAR_B itself."""
    GH = host[0]
    r = GH.censored_survey(sanitize=False, n_prior=300, n_box=150)
    for name, c in r["cases"].items():
        print(name, c)
        assert c["rows"] == c["header_finite_rows"] and c["rows"] >= 0.8 * c["rows_of_the_set"], name
        for col, e in c["max_err_over_scale"].items():
            assert e <= R.BAR, (name, col, e)
    tracked = json.load(open(os.path.join(ROOT, "profiles", "r22_wiener_censored_host.json")))
    assert tracked["max_err_over_scale"] <= G.BAR_B and tracked["bar"] == R.BAR == G.BAR_B
    assert tracked["max_err_over_scale"] <= R.HOST_MAX_ERR < 1.01 * tracked["max_err_over_scale"]
    assert set(tracked["cases"]) == {"prior_1s", "prior_4s", "box"} and tracked["cases"]["prior_1s"]["rows_of_the_set"] == 5000


def _case():
    good = [0.8, 1.2, 0.45, 0.2, 1.1]
    tr = [[0.6, 1.0], [0.9, -1.0], [1.4, 1.0]]
    return good, tr


@pytest.mark.skipif(not HAVE_CXX, reason="no host C++ compiler")
def test_special_values_and_neutrality_on_the_host(host):
    GH, exe, td = host
    good, tr = _case()
    ev = lambda P, D, c: GH.evaluate(exe, td, 0, np.asarray(P, np.float32), np.asarray(D, np.float32), censored=c)
    # rows: plain; a timeout; a timeout with rt <= tau; a timeout with a NaN rt; a choice of 2; a NaN choice; an invalid row; plain
    P = np.array([good, good, good, good, good, good, [0.8, 0.0, 0.45, 0.2, 1.1], good])
    D = np.array([tr, [tr[0], [1.1, 0.0], tr[2]], [tr[0], [0.15, 0.0], tr[2]], [tr[0], [np.nan, 0.0], tr[2]], [tr[0], [0.9, 2.0], tr[2]],
                  [tr[0], [0.9, np.nan], tr[2]], tr, tr])
    ll, g = ev(P, D, True)
    ll0, g0 = ev(P, D, False)
    assert np.array_equal(ll, ll0, equal_nan=True)                      # the value is the unflagged build's, bit for bit
    for i in (0, 7):                                                    # no timeout in the row: no bit changes
        assert np.array_equal(g[i], g0[i]) and np.all(np.isfinite(g[i]))
    assert np.all(np.isnan(g0[1])) and np.all(np.isnan(g0[2]))         # (unflagged: a timeout poisons)
    # the timeout's row against the yardstick, and its difference from the two responses alone: the timeout's own partials
    p64 = np.float32(good).astype(np.float64)[None]
    t = (np.float32(D[1, :, 0]) - np.float32(0.2)).astype(np.float64)[None]
    ref, scale = R.row_grad(p64, t, D[1:2, :, 1])
    assert np.all(np.isfinite(g[1])) and np.all(np.abs(g[1] - ref[0]) <= 1e-5 * scale[0])
    two = ev([good], [[tr[0], tr[2]]], True)[1][0]
    own = R.timeout_grad(p64[0], t[0, 1])
    assert np.all(np.abs((g[1] - two) - own) <= 1e-5 * scale[0]) and own[3] > 0.1 and abs(own[1]) > 0.1
    # rt <= tau on a timeout: log 1 = 0, zero partials -- the row is the two responses' (the sums add +0.0)
    assert np.array_equal(g[2], two) and ll[2] == ev([good], [[tr[0], tr[2]]], True)[0][0]
    for i in (3, 4, 5, 6):
        assert np.all(np.isnan(g[i])), i
    assert np.isnan(ll[3]) and np.isfinite(ll[4]) and np.isnan(ll[5]) and np.isnan(ll[6])
    # a row made of one timeout
    ll1, g1 = ev([good], [[[1.1, 0.0]]], True)
    assert np.all(np.abs(g1[0] - own) <= 1e-5 * np.abs(own)) and np.isfinite(ll1[0]) and ll1[0] < 0


@pytest.mark.skipif(not HAVE_CXX, reason="no host C++ compiler")
def test_censored_path_under_the_sanitizers():
    """The censored instantiation as the stand-alone program, built with -fsanitize=address,undefined -fno-sanitize-recover=all: both of
    log S's forms, a timeout at rt <= tau, and the special values; the results are the unsanitized build's to 1e-9."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import wiener_grad_host as GH
    sets = C.censor_sets(n_prior=40, n_box=40, with_fixture=False)
    p32, rt32, _ = sets["box"]
    rows, data, t, code = R.censored_rows(p32, rt32)
    u = t / (p32[rows, 1:2].astype(np.float64) / p32[rows, 4:5]) ** 2
    assert np.any((code == 0) & (u < SURV_U)) and np.any((code == 0) & (u >= SURV_U))
    data[0, 5] = (0.0, 0.0)                                             # a timeout at rt <= tau
    data[1, 6] = (np.nan, 0.0)
    with tempfile.TemporaryDirectory() as td, tempfile.TemporaryDirectory() as td2:
        san = GH.evaluate(GH.build(td, sanitize=True), td, 0, p32[rows], data, censored=True)
        plain = GH.evaluate(GH.build(td2), td2, 0, p32[rows], data, censored=True)
    assert np.all(np.isnan(san[1][1])) and np.all(np.isfinite(san[1][0])) and np.all(np.isfinite(san[1][2:]))
    for a, b in zip(san, plain):
        assert np.allclose(a, b, rtol=1e-9, atol=0, equal_nan=True)


def test_c_abi_takes_the_flag_for_basic_ddm_dc_only():
    """flags = NDDM_WIENER_CENSORED passes the flags check for NDDM_BASIC_DDM_DC (the next check, the shape, answers) and is
    NDDM_ERR_PARAM with its own words for NDDM_ALPHA_NOT_SCALED; model before flags, flags before shape; every other value keeps the
    words it had.  No case reaches a HIP call."""
    from bayesflow_nddms_amd import _lib
    L = _lib.lib()
    f = L.nddm_wiener_log_likelihood_grad
    d = ctypes.c_void_p(16)
    hdr = open(os.path.join(ROOT, "include", "nddm.h")).read()
    assert "#define NDDM_WIENER_CENSORED 4u" in hdr and _lib.WIENER_CENSORED == 4 and "#define NDDM_ABI_VERSION 4\n" in hdr
    shape = "R >= 0, n_trials > 0 and draws_per_dataset > 0 dividing R are required"
    reserved = "nddm_wiener_log_likelihood_grad: flags must be 0 (reserved)"
    own = "nddm_wiener_log_likelihood_grad: NDDM_WIENER_CENSORED takes NDDM_BASIC_DDM_DC only (alpha_not_scaled's y == 0 carries no time)"
    cases = [((0, d, 4, 3, d, 10, 4, d, d), _lib.NDDM_ERR_SHAPE, shape),
             ((0, d, 0, 1, d, 10, 4, d, d), _lib.NDDM_OK, ""),
             ((0, None, 4, 1, d, 10, 4, d, d), _lib.NDDM_ERR_NULL, "params or data is NULL"),
             ((0, d, 4, 1, d, 10, 4, None, None), _lib.NDDM_ERR_NULL, "out_grad is NULL"),
             ((3, d, 4, 3, d, 10, 4, d, d), _lib.NDDM_ERR_PARAM, own),
             ((3, d, 0, 1, d, 10, 4, d, d), _lib.NDDM_ERR_PARAM, own),
             ((1, d, 4, 1, d, 10, 4, d, d), _lib.NDDM_ERR_PARAM, "nddm_wiener_log_likelihood_grad: model 1 has no closed-form likelihood here "
                                                                 "(NDDM_BASIC_DDM_DC and NDDM_ALPHA_NOT_SCALED only)")]
    cases += [((m, d, 4, 3, d, 10, fl, d, d), _lib.NDDM_ERR_PARAM, reserved) for m in (0, 3) for fl in (1, 2, 3, 5, 6, 8, 12, 1 << 31)]
    for args, want, text in cases:
        assert f(*args, None) == want, args
        assert L.nddm_last_error().decode() == text, args


def test_python_adapters_take_censored():
    from bayesflow_nddms_amd import basic_ddm_dc, engine, likelihood
    import inspect
    for fn in (engine.wiener_log_likelihood_grad, likelihood.wiener_loglik, basic_ddm_dc.log_likelihood_and_grad):
        assert inspect.signature(fn).parameters["censored"].default is False
    data = np.array([[[0.6, 1.0], [0.7, 0.0]]])
    for wl in (engine.wiener_log_likelihood_grad, likelihood.wiener_loglik):
        with pytest.raises(ValueError, match="BASIC_DDM_DC only"):
            wl(engine.ALPHA_NOT_SCALED, np.array([[1.0, 1.0, 0.5, 0.3, 0.2, 1.0]]), data, censored=True)
        with pytest.raises(ValueError, match=r"\(0, 1\)"):              # (the host checks are the unflagged call's)
            wl(engine.BASIC_DDM_DC, np.array([[1.0, 1.0, 1.0, 0.3, 1.0]]), data, censored=True)
        with pytest.raises(ValueError, match="choice"):
            wl(engine.BASIC_DDM_DC, np.array([[1.0, 1.0, 0.5, 0.3, 1.0]]), np.array([[[0.6, 2.0]]]), censored=True)
