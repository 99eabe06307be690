"""CPU tests of the gradient of the single-trial model's marginal log-likelihood (nddm_wiener_marginal_log_likelihood_grad;
csrc/nddm_wiener_marginal_grad.h): the float64 yardstick (tests/wiener_marginal_grad_ref.py) pins itself against Richardson-extrapolated
central differences of wiener_marginal_ref.log_lik; the header's own per-trial code and chain rule compiled for the host meet the recorded
float32 figures, give the forward header's value bit for bit and the special values -- a timeout gets a FINITE gradient; the partials of log S
alone hold against central differences of wiener_cdf_ref.log_survival across the crossover of its two forms; the C ABI and the Python adapters
refuse bad input before any device work."""
import ctypes
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import pytest

import wiener_cdf_ref as C
import wiener_marginal_grad_ref as MG
import wiener_marginal_ref as M
from conftest import ROOT

HAVE_CXX = not (shutil.which("g++") is None and shutil.which("c++") is None and shutil.which("clang++") is None)
N_HOST = 300              # rows of each set the host program is run on here (the survey behind the recorded figures: 1500)
RECORD = os.path.join(ROOT, "profiles", "r16_wiener_marginal_grad_host.json")


def test_yardstick_equals_finite_differences_of_log_lik():
    """The first 16 rows and the first 4 censored rows of each set, all 8 columns: wiener_marginal_grad_ref.grad_log_lik against
    Richardson-extrapolated central differences of wiener_marginal_ref.log_lik (relative steps 2e-3 and 1e-3; ter's scaled to the decision
    time), to 1e-6 of max(1, |d|), section 14's bar.  Measured: 2.1e-8 at the most (beta on prior_rows); largest |d| 147."""
    worst, largest = 0.0, 0.0
    for name, rows in M.SETS.items():
        p32, y32, z32, tc = rows(M.POOL)
        cens = np.flatnonzero(y32 == 0)[:4]
        assert cens.size == 4, name
        idx = np.array(list(range(16)) + list(cens))
        p, y, z = M.as_f64(p32[idx], y32[idx], z32[idx])
        got, fd = MG.grad_log_lik(p, y, z, tc), MG.fd_grad(p, y, z, tc)
        assert np.all(np.isfinite(got)) and np.all(np.isfinite(fd)), name
        err = np.abs(got - fd) / np.maximum(1.0, np.abs(fd))
        print(f"{name}: max |yardstick - finite difference| / max(1, |d|) per column = {np.array2string(err.max(0), precision=2)}")
        worst, largest = max(worst, float(err.max())), max(largest, float(np.abs(fd).max()))
        assert err.max() <= 1e-6, (name, MG.COLUMNS[int(np.argmax(err.max(0)))], float(err.max()))
        assert np.all(got[16:, 3] == 0.0)                               # a timeout does not depend on ter
    print(f"40 rows x 8 columns: {worst:.3g}; largest |d| {largest:.3g}")
    assert largest > 10.0                                               # (not a set of zeros)


@pytest.fixture(scope="module")
def host():
    """(module of tools/wiener_marginal_grad_host.py, its program built without a sanitizer, a scratch directory)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import wiener_marginal_grad_host as GH
    with tempfile.TemporaryDirectory() as td:
        yield GH, GH.build(td), td


@pytest.fixture(scope="module")
def surveyed(host):
    """name -> (rows of the set, the host program's (loglik, grad), the yardstick's gradient) on the first N_HOST rows: computed once."""
    GH, exe, td = host
    out = {}
    for name, rows in M.SETS.items():
        p32, y32, z32, tc = rows(N_HOST)
        got = GH.evaluate(exe, td, p32, np.stack([y32, z32], 1)[:, None, :], tc)
        out[name] = ((p32, y32, z32, tc), got, MG.grad_log_lik(*M.as_f64(p32, y32, z32), tc))
    return out


@pytest.mark.skipif(not HAVE_CXX, reason="no host C++ compiler")
def test_header_compiled_for_the_host_meets_the_recorded_figures(host, surveyed):
    """The header's float32 gradient on the first N_HOST rows of each set stays, per column, within the largest error over scale_j of the
    1500-row survey (profiles/r16_wiener_marginal_grad_host.json, the tool's own output), which the set's device bar is 4 x of.  No row is
    left out: the yardstick converges on every one and the header is finite on every one, censored rows included."""
    GH = host[0]
    tracked = json.load(open(RECORD))
    assert tracked["sanitized"] and tracked["rows_per_set"] == M.POOL and tracked["trials_per_row"] == 1
    for name, ((p32, y32, z32, tc), (ll, grad), ref) in surveyed.items():
        c = tracked["cases"][name]
        assert np.all(np.isfinite(ref)) and np.all(np.isfinite(grad)) and np.all(np.isfinite(ll)), name
        assert c["rows"] == c["yardstick_finite_rows"] == c["header_finite_rows"] == M.POOL and c["censored"] > 0
        rel = GH.errors_over_scale(grad, ref, np.abs(ref))
        for j, col in enumerate(MG.COLUMNS):
            print(f"{name} {col}: max |float32 - yardstick| / scale = {rel[:, j].max():.3g} (recorded on {c['rows']} rows: {c['max_err_over_scale'][col]:.3g})")
            assert rel[:, j].max() <= c["max_err_over_scale"][col], (name, col)
        worst = max(c["max_err_over_scale"].values())
        assert MG.DEVICE_BAR[name] == c["device_bar"] == GH.round_up_1sd(4.0 * worst), name


@pytest.mark.skipif(not HAVE_CXX, reason="no host C++ compiler")
def test_value_is_the_forward_headers_bit_for_bit(host, surveyed):
    GH, exe, td = host
    import wiener_marginal_host as MH
    with tempfile.TemporaryDirectory() as td2:
        fwd = MH.build(td2)
        for name, ((p32, y32, z32, tc), (ll, _), _) in surveyed.items():
            v = MH.evaluate(fwd, td2, p32, np.stack([y32, z32], 1)[:, None, :], tc)[:, 0]
            assert np.array_equal(ll, v.astype(np.float64)), name
        # several trials per row: the float64 sum of the forward header's float32 trials, in order
        p32, y32, z32, tc = M.box(8)
        ym, zm = M.more_trials("box", p32, 5)
        data = np.stack([np.concatenate([y32[:, None], ym], 1), np.concatenate([z32[:, None], zm], 1)], -1)
        ll, g = GH.evaluate(exe, td, p32, data, tc)
        tr = MH.evaluate(fwd, td2, p32, data, tc).astype(np.float64)
        s = np.zeros(8)
        for j in range(6):
            s = s + tr[:, j]
        assert np.array_equal(ll, s) and np.all(np.isfinite(g)) and np.any(data[..., 0] == 0)


@pytest.mark.skipif(not HAVE_CXX, reason="no host C++ compiler")
def test_special_values_on_the_host(host):
    GH, exe, td = host
    good = [0.8, 1.2, 0.45, 0.2, 0.5, 1.1, 0.7, 1.0]
    tr = [[0.6, 1.0], [-0.9, 1.4], [1.3, 0.9]]
    run = lambda P, D, tc=2.0: GH.evaluate(exe, td, np.array(P), np.array(D), tc)
    # a row whose only oddity is a timeout: a finite value and a FINITE gradient, the yardstick's
    odd = [tr[0], [0.0, 1.1], tr[2]]
    ll, g = run([good, good], [tr, odd])
    assert np.all(np.isfinite(ll)) and np.all(np.isfinite(g))
    p32 = np.float32([good])
    for k, d in enumerate((tr, odd)):
        d32 = np.float32([d])
        ref = MG.pairs_grad(p32, d32[..., 0], d32[..., 1], 2.0)[0]
        assert np.all(np.abs(g[k] - ref.sum(0)) <= MG.DEVICE_BAR["prior_rows"] * np.abs(ref).sum(0)), k
    assert np.any(np.abs(g[1] - g[0]) > 1e-3)                            # (the timeout moved it)
    # invalid rows between valid ones: NaN in the value and in every column, the neighbours unaffected
    bad = [dict(col=4, val=0.0), dict(col=6, val=-1.0), dict(col=5, val=0.0), dict(col=2, val=1.0), dict(col=2, val=0.0), dict(col=3, val=-0.1),
           dict(col=0, val=np.nan), dict(col=7, val=np.inf)]
    P = [good]
    for b in bad:
        r = list(good)
        r[b["col"]] = b["val"]
        P += [r, good]
    ll2, g2 = run(P, [odd] * len(P))
    assert np.all(np.isnan(ll2[1::2])) and np.all(np.isnan(g2[1::2]))
    assert np.array_equal(ll2[0::2], np.repeat(ll[1], len(bad) + 1)) and np.array_equal(g2[0::2], np.tile(g[1], (len(bad) + 1, 1)))
    # a response with |y| < ter and with |y| == ter: -inf and a NaN row gradient
    for y in (0.15, 0.2):
        l, gg = run([good], [[tr[0], [y, 1.0], tr[2]]])
        assert l[0] == -np.inf and np.all(np.isnan(gg))
    # a timeout without a censoring time, a non-finite z1, a NaN y: NaN in both
    for tc in (0.0, -1.0, float("nan")):
        l, gg = run([good], [odd], tc)
        assert np.isnan(l[0]) and np.all(np.isnan(gg))
    for d in ([0.7, np.nan], [0.7, np.inf], [np.nan, 1.0]):
        l, gg = run([good], [[tr[0], d, tr[2]]])
        assert np.isnan(l[0]) and np.all(np.isnan(gg))
    # every node at -inf (z1 so far out that the Gaussian factor underflows at every boundary): -inf and NaN
    l, gg = run([good], [[[0.6, 1e30]]])
    assert l[0] == -np.inf and np.all(np.isnan(gg))


@pytest.mark.skipif(not HAVE_CXX, reason="no host C++ compiler")
def test_log_survival_partials_against_central_differences(host):
    """wiener_log_survival_grad alone: u in [1e-3, 50] log-uniform plus a quarter in [0.04, 0.09] (the WIENER_SURV_U = 0.06 crossover of the
    images and the series), w in [0.01, 0.99], v' in [-5, 5], a' in [0.5, 2.5], against Richardson-extrapolated central differences of
    wiener_cdf_ref.log_survival where S >= 1e-3 (its domain).  Bar: 1e-4 of max(1, |d|) -- float32's 6e-8 over the cancellation the
    difference of images may have to hold, 1 / S <= 1e3, rounded up to a power of ten.  Measured: 6.3e-6 at the most."""
    GH, exe, td = host
    rng = np.random.default_rng(3)
    n = 4000
    u = np.exp(rng.uniform(np.log(1e-3), np.log(50.0), n))
    u[:n // 4] = rng.uniform(0.04, 0.09, n // 4)
    q = np.stack([rng.uniform(0.5, 2.5, n), rng.uniform(0.01, 0.99, n), rng.uniform(-5, 5, n), u], 1)
    q[:, 3] *= q[:, 0] ** 2
    a, w, v, t = q.astype(np.float32).astype(np.float64).T
    ls = lambda a_, w_, v_: C.log_survival(t, a_, v_, w_, 1.0)

    def rich(f, h):
        def cd(s):
            (hi, ok1), (lo, ok2) = f(s), f(-s)
            return (hi - lo) / (2.0 * s), ok1 & ok2
        (c1, o1), (c2, o2) = cd(h), cd(0.5 * h)
        return (4.0 * c2 - c1) / 3.0, o1 & o2
    refs = [rich(lambda s: ls(a + s, w, v), 1e-3 * a), rich(lambda s: ls(a, w + s, v), 1e-3 * np.minimum(w, 1.0 - w)),
            rich(lambda s: ls(a, w, v + s), 1e-3 * np.maximum(np.abs(v), 1.0))]
    val, ok = ls(a, w, v)
    for _, o in refs:
        ok = ok & o
    small = t / (a * a) < 0.06
    assert (ok & small).sum() > 500 and (ok & ~small).sum() > 500      # both forms
    got = GH.survival(exe, td, a, w, v, t).astype(np.float64)
    assert np.max(np.abs(got[ok, 0] - val[ok])) <= 1e-5                  # (the value: wiener_log_survival's)
    for j, (name, (ref, _)) in enumerate(zip(("d/da'", "d/dw", "d/dv'"), refs), 1):
        err = np.abs(got[ok, j] - ref[ok]) / np.maximum(1.0, np.abs(ref[ok]))
        print(f"{name}: {int(ok.sum())} points, max |header - central difference| / max(1, |d|) = {err.max():.3g}; largest |d| {np.abs(ref[ok]).max():.3g}")
        assert err.max() <= 1e-4, name
    # t <= 0: log 1 = 0 and no slope
    z = GH.survival(exe, td, [1.0, 1.0], [0.4, 0.4], [1.0, 1.0], [0.0, -1.0])
    assert np.all(z == 0.0)


def test_c_abi_exports_the_entry_and_validates_before_any_hip_call():
    from bayesflow_nddms_amd import _lib
    L = _lib.lib()
    assert "nddm_wiener_marginal_log_likelihood_grad" in _lib.EXPORTS and hasattr(L, "nddm_wiener_marginal_log_likelihood_grad")
    assert L.nddm_abi_version() == _lib.ABI_VERSION == 4
    f = L.nddm_wiener_marginal_log_likelihood_grad
    assert f.argtypes[6] is ctypes.c_float and f.argtypes[7] is ctypes.c_uint32 and len(f.argtypes) == 11
    d = ctypes.c_void_p(16)
    hdr = open(os.path.join(ROOT, "include", "nddm.h")).read()
    assert "int nddm_wiener_marginal_log_likelihood_grad(" in hdr and "#define NDDM_ABI_VERSION 4" in hdr
    assert "/* 4 (additive): nddm_wiener_marginal_log_likelihood_grad.  No existing entry point changes. */" in hdr
    assert "NOT IMPLEMENTED: the gradient of basic_ddm_dc's censored timeouts" in hdr                    # (section 14's entry: unchanged)
    assert "NDDM_SINGLE_TRIAL_ALT (a latent diffusion coefficient) is OUT OF" in hdr
    from bayesflow_nddms_amd import build
    assert any(p.endswith("nddm_wiener_marginal_grad.h") for p in build.HEADERS)         # part of the source hash
    import torch
    if not torch.cuda.is_available():
        assert f(1, d, 4, 2, d, 10, 4.0, 0, None, d, None) in (_lib.NDDM_ERR_HIP, _lib.NDDM_ERR_NO_DEVICE)      # (out_loglik may be NULL)


d = "d"                                                                 # stands for a non-NULL pointer (never dereferenced: every case ends before a launch)
NAME = "nddm_wiener_marginal_log_likelihood_grad"
MODEL_MSG = NAME + ": model %d has no marginal likelihood here (NDDM_SINGLE_TRIAL only)"
FLAGS_MSG = NAME + ": flags must be 0 (reserved)"
SHAPE_MSG = "R >= 0, n_trials > 0 and draws_per_dataset > 0 dividing R are required"
# ((model, params, R, draws_per_dataset, data, n, flags, out_loglik, out_grad), status, nddm_last_error() in full): nddm_wiener_marginal_
# log_likelihood's cases (tests/test_wiener_host.py) with this entry's name and its one mandatory output
ARGUMENT_CASES = [
    ((0, d, 4, 1, d, 10, 0, d, d), "PARAM", MODEL_MSG % 0),
    ((2, d, 4, 1, d, 10, 0, d, d), "PARAM", MODEL_MSG % 2),
    ((3, d, 4, 1, d, 10, 0, d, d), "PARAM", MODEL_MSG % 3),
    ((4, d, 4, 1, d, 10, 0, d, d), "PARAM", MODEL_MSG % 4),
    ((7, d, 4, 1, d, 10, 0, d, d), "PARAM", MODEL_MSG % 7),
    ((1, None, -1, 1, None, 0, 1, None, None), "PARAM", FLAGS_MSG),
    ((1, None, -1, 1, None, 10, 0, None, None), "SHAPE", SHAPE_MSG),
    ((1, d, 4, 1, d, 0, 0, d, d), "SHAPE", SHAPE_MSG),
    ((1, d, 4, 0, d, 10, 0, d, d), "SHAPE", SHAPE_MSG),
    ((1, d, 4, 3, d, 10, 0, d, d), "SHAPE", SHAPE_MSG),
    ((1, None, 0, 1, None, 10, 0, None, None), "OK", ""),
    ((1, None, 4, 1, d, 10, 0, d, d), "NULL", "params or data is NULL"),
    ((1, d, 4, 1, None, 10, 0, d, d), "NULL", "params or data is NULL"),
    ((1, d, 4, 1, d, 10, 0, d, None), "NULL", "out_grad is NULL"),
    ((1, d, 4, 1, d, 10, 0, None, None), "NULL", "out_grad is NULL"),
    # the order of the checks: model before flags, flags before shape, shape and R / 16 before the pointers, inputs before outputs
    ((0, None, -1, 0, None, 0, 1, None, None), "PARAM", MODEL_MSG % 0),
    ((1, None, -1, 0, None, 0, 1, None, None), "PARAM", FLAGS_MSG),
    ((1, d, 4, 3, d, 10, 1, d, d), "PARAM", FLAGS_MSG),
    ((1, None, 4, 3, None, 10, 0, None, None), "SHAPE", SHAPE_MSG),
    ((1, None, 1 << 35, 1, None, 10, 0, None, None), "SHAPE", "R / 16 must be < 2^31 per launch"),
    ((1, None, 4, 1, d, 10, 0, None, None), "NULL", "params or data is NULL"),
    ((1, d, 4, 1, None, 10, 0, None, None), "NULL", "params or data is NULL"),
]


def test_argument_contract_of_the_entry_point():
    """Every status code, which check wins when two are violated, and the text of nddm_last_error(): the shared launch path's
    (csrc/nddm_kernels.hip: wiener_launch), with this entry's name.  No case reaches a HIP call."""
    from bayesflow_nddms_amd import _lib
    L = _lib.lib()
    f = L.nddm_wiener_marginal_log_likelihood_grad
    status = {"OK": _lib.NDDM_OK, "NULL": _lib.NDDM_ERR_NULL, "SHAPE": _lib.NDDM_ERR_SHAPE, "PARAM": _lib.NDDM_ERR_PARAM}
    for args, want, text in ARGUMENT_CASES:
        model, params, R, S, data, n, flags, *outs = [ctypes.c_void_p(16) if a is d else a for a in args]
        assert f(model, params, R, S, data, n, 4.0, flags, *outs, None) == status[want], args
        assert L.nddm_last_error().decode() == text, args


def test_python_adapters_check_host_inputs():
    from bayesflow_nddms_amd import engine, likelihood, single_trial_alpha_not_scaled as st
    import bayesflow_nddms_amd as pkg
    assert {"wiener_marginal_log_likelihood_grad", "single_trial_loglik"} <= set(pkg.__all__)
    assert pkg.wiener_marginal_log_likelihood_grad is engine.wiener_marginal_log_likelihood_grad and pkg.single_trial_loglik is likelihood.single_trial_loglik
    good = np.array([[0.8, 1.2, 0.45, 0.2, 0.5, 1.1, 0.7, 1.0]])
    data = np.array([[[0.6, 1.0], [-0.7, 1.3]]])
    for wl in (engine.wiener_marginal_log_likelihood_grad, lambda model, *a, **k: likelihood.single_trial_loglik(*a, **k)):
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
        for tc in (-1.0, float("nan")):
            with pytest.raises(ValueError, match="t_censor"):
                wl(engine.SINGLE_TRIAL, good, data, t_censor=tc)
    for model, P in ((engine.BASIC_DDM_DC, 5), (engine.ALPHA_NOT_SCALED, 6), (engine.SINGLE_TRIAL_ALT, 8), (engine.EXPLICIT_BOUNDARY, 4)):
        with pytest.raises(ValueError, match="SINGLE_TRIAL only"):
            engine.wiener_marginal_log_likelihood_grad(model, np.ones((1, P)), data)
    with pytest.raises(ValueError, match="cannot be split"):
        st.log_likelihood_and_grad(np.repeat(good[:, :7], 3, 0), np.repeat(data, 2, 0))
    with pytest.raises(ValueError, match="> 0"):
        st.log_likelihood_and_grad(np.array([0.8, 1.2, 0.45, 0.2, 0.0, 1.1, 0.7]), data[0])
    for doc in (engine.wiener_marginal_log_likelihood_grad.__doc__, likelihood.single_trial_loglik.__doc__, st.log_likelihood_and_grad.__doc__):
        assert "t_censor" in doc or "max_steps" in doc
        assert "gradient" in doc
