"""GPU tests of the Wiener trio (nddm_wiener_log_likelihood, nddm_wiener_cdf, nddm_wiener_quantile) on the parameters the two models
actually draw, against the float64 yardsticks (tests/wiener_ref.py, tests/wiener_cdf_ref.py) and at the shipped tests' bars: the
density, the distribution function and P(upper), the quantile's three residuals, the right-censored timeouts (the survival's two forms
and its deep tails, tests/golden/wiener_survival.npz), and the density's launch shapes at the lane, tile and row-group edges with
distinct parameters per row.  tests/test_wiener_host.py runs the same rows through the headers' code compiled for the host."""
import os

import numpy as np
import pytest

import wiener_cdf_ref as C
import wiener_ref as W
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

N_ROWS = 20_000


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _model(basic):
    from bayesflow_nddms_amd import engine
    return engine.BASIC_DDM_DC if basic else engine.ALPHA_NOT_SCALED


def _trials(basic, rt32, up):
    """float32 [..., 2] trials of response time rt32 on the boundary `up` in the model's format."""
    if basic:
        return np.stack([rt32, np.where(up, 1.0, -1.0)], -1).astype(np.float32)
    y = np.where(up, rt32, -rt32).astype(np.float32)
    return np.stack([y, (np.sign(y) + 1) / 2], -1).astype(np.float32)


_ROWS = {}


def _prior_rows(basic):
    """C.prior_rows and its float64 references, worked out once per model: (p32, rt32, up, t, log f, F, P(upper))."""
    if basic not in _ROWS:
        p32, rt32, up, t = C.prior_rows(N_ROWS, basic)
        a, v, beta, _, s, eta = C.row_columns(p32, basic)
        ref = (W.log_f(t, up, a, v, beta, s, eta), C.cdf(t, up, a, v, beta, s, eta), C.p_upper(a, v, beta, s, eta))
        for x in (p32, rt32, up, t) + ref:
            x.setflags(write=False)
        _ROWS[basic] = (p32, rt32, up, t) + ref
    return _ROWS[basic]


def _name(basic):
    return "basic_ddm_dc" if basic else "alpha_not_scaled"


@pytest.mark.parametrize("basic", [True, False])
def test_density_on_the_priors(basic):
    """|d log f| <= 1e-4 where |log f| <= 20 and 1e-5 relative beyond: the shipped pointwise bars, on basic_ddm_dc's prior (dc >= 0.05:
    a / dc up to 39) and on alpha_not_scaled's prior and box with Varsigma != 1 and Eta > 0 (eta / s, a / s, v / s all in play)."""
    torch = _torch()
    from bayesflow_nddms_amd import engine
    p32, rt32, up, t, ref, _, _ = _prior_rows(basic)
    got = engine.wiener_log_likelihood(_model(basic), torch.as_tensor(p32).cuda(), torch.as_tensor(_trials(basic, rt32, up)[:, None, :]).cuda(),
                                       per_trial=True)["trial_logp"][:, 0].double().cpu().numpy()
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(ref))
    err, inner = np.abs(got - ref), np.abs(ref) <= 20
    print(f"density on the priors ({_name(basic)}, {N_ROWS} rows): max |d log f| {err[inner].max():.3g} where |log f| <= 20 "
          f"({inner.sum()} rows), max rel {np.max(err[~inner] / np.abs(ref[~inner])):.3g} beyond")
    if not basic:                                                       # Varsigma is not 1 and Eta is not 0 where it is tested
        assert np.mean((p32[:, 5] != 1.0) & (p32[:, 4] > 0)) > 0.8
    assert err[inner].max() <= 1e-4
    assert np.all(err[~inner] <= 1e-5 * np.abs(ref[~inner]))


@pytest.mark.parametrize("basic", [True, False])
def test_distribution_function_and_p_upper_on_the_priors(basic):
    """|F - yardstick| <= 2e-5 and |P(upper) - yardstick| <= 2e-5 on the rows of the density's test."""
    torch = _torch()
    from bayesflow_nddms_amd import engine
    p32, rt32, up, t, _, Fref, Pref = _prior_rows(basic)
    r = engine.wiener_cdf(_model(basic), torch.as_tensor(p32).cuda(), torch.as_tensor(_trials(basic, rt32, up)[:, None, :]).cuda())
    got, gp = r["cdf"][:, 0].double().cpu().numpy(), r["p_upper"].double().cpu().numpy()
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(gp)) and got.min() >= 0.0 and got.max() <= 1.0
    err, perr = np.abs(got - Fref), np.abs(gp - Pref)
    print(f"distribution function on the priors ({_name(basic)}): max |F - ref| {err.max():.3g}, max |p_upper - ref| {perr.max():.3g}")
    assert err.max() <= 2e-5 and perr.max() <= 2e-5


@pytest.mark.parametrize("rows", ["basic_prior", "alpha_ns_prior", "varsigma_box"])
def test_quantile_residuals_on_the_priors(rows):
    """Residuals (i), (ii), (iii) of tests/test_gpu_wiener_quantile.py and their bars 2e-5, 6e-5, 4e-5, on the priors' rows with tau = 0:
    conditional p ~ U(0.001, 0.999) on the drawn boundary, rows with float64 P(boundary) >= 0.01 kept (at least 80 % of them, a
    property of the inputs alone)."""
    torch = _torch()
    from bayesflow_nddms_amd import engine
    basic = rows == "basic_prior"
    p32, _, up, _, _, _, pu = _prior_rows(basic)
    half = slice(None) if basic else slice(0, N_ROWS // 2) if rows == "alpha_ns_prior" else slice(N_ROWS // 2, None)
    p32, up, pu = p32[half].copy(), up[half], pu[half]
    p32[:, 3] = 0.0
    n = p32.shape[0]
    a, v, beta, _, s, eta = C.row_columns(p32, basic)
    P64 = np.where(up, pu, 1.0 - pu)
    keep = P64 >= 0.01
    print(f"{rows}: {keep.mean():.3f} of {n} rows have P(boundary) >= 0.01")
    assert keep.mean() >= 0.80
    pc = np.random.default_rng(21).uniform(0.001, 0.999, n).astype(np.float32)
    code = np.where(up, 1.0, -1.0).astype(np.float32)
    model, pd = _model(basic), torch.as_tensor(p32).cuda()
    q = engine.wiener_quantile(model, pd, torch.as_tensor(np.stack([pc, code], 1)[:, None, :]).cuda(), conditional=True)["quantile"][:, 0].double().cpu().numpy()
    assert np.all(np.isfinite(q[keep])) and np.all(q[keep] > 0.0)
    rt = np.stack([np.where(np.isfinite(q), q, 1.0), np.full(n, np.inf)], 1)
    Fd = engine.wiener_cdf(model, pd, torch.as_tensor(_trials(basic, rt, np.stack([up, up], 1))).cuda(), want_p_upper=False)["cdf"].double().cpu().numpy()
    r1 = np.abs(Fd[:, 0] - pc.astype(np.float64) * Fd[:, 1])[keep]
    r2 = np.abs(C.cdf(q, up, a, v, beta, s, eta) - pc.astype(np.float64) * P64)[keep]
    tgt = (pc.astype(np.float64) * P64).astype(np.float32)
    qd = engine.wiener_quantile(model, pd, torch.as_tensor(np.stack([tgt, code], 1)[:, None, :]).cuda())["quantile"][:, 0].double().cpu().numpy()
    assert np.all(np.isfinite(qd[keep]))
    r3 = np.abs(C.cdf(qd, up, a, v, beta, s, eta) - tgt.astype(np.float64))[keep]
    print(f"  max (i) |wiener_cdf(q) - p P_device| {r1.max():.3g}, (ii) |yardstick(q) - p P_float64| {r2.max():.3g}, "
          f"(iii) defective |yardstick(q) - target| {r3.max():.3g}")
    assert r1.max() <= 2e-5
    assert r2.max() <= 6e-5
    assert r3.max() <= 4e-5


@pytest.mark.parametrize("rows", ["prior_1s", "prior_4s", "box", "fixture"])
def test_censored_timeouts_on_the_priors(rows):
    """basic_ddm_dc choice 0 at 16 increasing times per row: never NaN, never above 0, non-increasing; within 2e-5 + 1e-5 |ref| of
    log1p(-(F_lower + F_upper)) of the float64 yardstick where S >= 1e-3, and within 1e-3 |ref| below it (the fixture's high-precision
    values: such a point is at least 6.9 nats down, and a relative 1e-3 there cannot reorder posterior draws); the same trials through
    wiener_cdf give 1 - S at 2e-5.  The fixture's first four rows are the report's: the large-time series alone gave NaN, +9.3, +15.7
    and -0.16 there for -0.000000, -2.507289, -0.009398 and -6.160853."""
    torch = _torch()
    from bayesflow_nddms_amd import engine
    p32, rt32, t = C.censor_sets()[rows]
    a, v, beta, _, s, _ = C.row_columns(p32, True)
    ref, ok = C.log_survival(t, a[:, None], v[:, None], beta[:, None], s[:, None])
    pd = torch.as_tensor(p32).cuda()
    d = torch.as_tensor(np.stack([rt32, np.zeros_like(rt32)], -1)).cuda()
    r = engine.wiener_log_likelihood(engine.BASIC_DDM_DC, pd, d, per_trial=True)
    lp = r["trial_logp"].double().cpu().numpy()
    F = engine.wiener_cdf(engine.BASIC_DDM_DC, pd, d, want_p_upper=False)["cdf"].double().cpu().numpy()
    u = t / (a / s)[:, None] ** 2
    ratio = (np.abs(lp - ref) / (2e-5 + 1e-5 * np.abs(ref)))[ok]
    dF = np.abs(F - (-np.expm1(ref)))[ok]
    print(f"censored ({rows}): {p32.shape[0]} rows x {t.shape[1]} times, u {u.min():.2g} .. {u.max():.3g}, {int((u < 0.06).sum())} below the forms' "
          f"switch; {ok.sum()} points with S >= 1e-3: max |err| / (2e-5 + 1e-5 |ref|) {np.nanmax(ratio):.3g}, max |cdf - (1 - S)| {np.nanmax(dF):.3g}; "
          f"NaN {int(np.isnan(lp).sum())}, above 0 {int((lp > 0).sum())}, increasing pairs {int((np.diff(lp, axis=1) > 0).sum())}")
    assert not np.isnan(lp).any() and np.all(lp <= 0.0)
    assert np.all(np.diff(lp, axis=1) <= 0.0)
    assert ok.sum() > 1000 and (u[ok] < 0.06).sum() > 100 and (u[ok] >= 0.06).sum() > 100
    assert np.all(ratio <= 1.0)
    assert np.all(np.isfinite(F)) and F.min() >= 0.0 and F.max() <= 1.0 and np.all(dF <= 2e-5)
    assert np.all(np.isfinite(r["loglik"].cpu().numpy()))
    if rows == "fixture":
        g = np.load(os.path.join(GOLDEN, "wiener_survival.npz"))
        deep, want = g["mp"], g["log_s"]
        assert np.array_equal(deep, ~ok) and deep.sum() > 1000
        rel = (np.abs(lp - want) / np.abs(want))[deep]
        dFd = np.abs(F - (-np.expm1(want)))[deep]
        print(f"  {deep.sum()} points with S < 1e-3 (log S down to {want.min():.0f}): max |err| / |ref| {rel.max():.3g}, max |cdf - (1 - S)| {dFd.max():.3g}; "
              f"the report's rows: {lp[:4, -1]}")
        assert np.all(rel <= 1e-3) and np.all(dFd <= 2e-5)
        assert np.array_equal(p32[:4], C.REPORTED_ROWS) and np.array_equal(rt32[:4, -1], C.REPORTED_RT)


def _shape_rows(n, rng, basic):
    """Distinct moderate rows, Varsigma in [0.8, 1.2]; alpha_not_scaled with Eta in [0, 1.5]."""
    cols = [rng.uniform(-2, 2, n), rng.uniform(0.6, 1.8, n), rng.uniform(0.2, 0.8, n), rng.uniform(0.1, 0.3, n)]
    cols += [rng.uniform(0.8, 1.2, n)] if basic else [rng.uniform(0, 1.5, n), rng.uniform(0.8, 1.2, n)]
    return np.stack(cols, 1).astype(np.float32)


@pytest.mark.parametrize("basic", [True, False])
@pytest.mark.parametrize("D,S,N", [(1, 1, 1), (15, 1, 65), (17, 1, 1025), (33, 1, 63), (2, 16, 1), (3, 17, 1025), (2, 31, 2049), (3, 40, 1023)])
def test_density_shapes_against_float64(basic, D, S, N):
    """Paired (S = 1: R = D rows, each with its own data) and LDS-staged (S >= 16 rows share a data set) launches at the 64-lane, the
    1024-trial tile and the 16-row group edges, with distinct parameters per row and distinct data per data set; basic_ddm_dc carries
    a censored trial at every fifth position.  Every per-trial value is held to the pointwise bars against float64; loglik is the
    float64 sum of the device's own trial_logp to 1e-12; the sum-only call gives the same bits."""
    torch = _torch()
    from bayesflow_nddms_amd import engine
    rng = np.random.default_rng(1000 * D + 10 * S + N + (7 if basic else 0))
    R = D * S
    p32 = _shape_rows(R, rng, basic)
    rt32 = rng.uniform(0.35, 3.0, (D, N)).astype(np.float32)                  # above every row's tau
    up = rng.random((D, N)) < 0.5
    data = _trials(basic, rt32, up)
    cens = np.zeros((D, N), bool)
    if basic:
        cens[:, ::5] = True
        data[cens, 1] = 0.0
    model, pd, dd = _model(basic), torch.as_tensor(p32).cuda(), torch.as_tensor(data).cuda()
    r = engine.wiener_log_likelihood(model, pd, dd, draws_per_dataset=S, per_trial=True)
    lp, ll = r["trial_logp"], r["loglik"]
    assert tuple(lp.shape) == (R, N) and tuple(ll.shape) == (R,) and ll.dtype == torch.float64
    # float64 reference per (row, trial) at the kernel's float32 t = rt - tau
    ds = np.repeat(np.arange(D), S)
    t = (rt32[ds] - p32[:, 3:4]).astype(np.float32).astype(np.float64)
    a, v, beta, _, s, eta = (x[:, None] for x in C.row_columns(p32, basic))
    ref = W.log_f(t, up[ds], a, v, beta, s, eta)
    got = lp.double().cpu().numpy()
    assert np.all(np.isfinite(got))
    unc = ~cens[ds]
    err, inner = np.abs(got - ref), np.abs(ref) <= 20
    assert np.all(err[unc & inner] <= 1e-4) and np.all(err[unc & ~inner] <= 1e-5 * np.abs(ref[unc & ~inner]))
    worst_c = 0.0
    if basic:
        sref, ok = C.log_survival(t, a, v, beta, s)
        ok &= cens[ds]
        assert ok.sum() >= cens[ds].sum() // 3 and np.all(got[cens[ds]] <= 0.0)       # (S >= 1e-3 on 52-64 % of them, by the inputs alone)
        ratio = (np.abs(got - sref) / (2e-5 + 1e-5 * np.abs(sref)))[ok]
        worst_c = ratio.max(initial=0.0)
        assert np.all(ratio <= 1.0)
    print(f"shape D {D} S {S} N {N} ({_name(basic)}): max |d log f| {err[unc & inner].max(initial=0.0):.3g}; censored max |err| / bar {worst_c:.3g}")
    # the row sum is the float64 sum of the device's own per-trial values, and the sum-only launch gives the same bits
    assert torch.allclose(ll, lp.double().sum(1), rtol=1e-12, atol=0)
    only = engine.wiener_log_likelihood(model, pd, dd, draws_per_dataset=S, per_trial=False)["loglik"]
    assert torch.equal(only.view(torch.int64), ll.view(torch.int64))


MAPPING_S, MAPPING_D, MAPPING_N = (1, 5, 16, 17, 35), (1, 3), (1, 65, 1030)
_MAPPING = {}


def _mapping_inputs(model_name):
    """Prior rows (distinct per row) and data sets (distinct per set) for the largest shape, drawn once per model; a shape takes the
    leading rows, sets and trials.  -> (params [105, P], {kernel: data [3, 1030, 2]})."""
    if model_name not in _MAPPING:
        import prior_util
        R, D, N = max(MAPPING_S) * max(MAPPING_D), max(MAPPING_D), max(MAPPING_N)
        rng = np.random.default_rng(41)
        rt32, up = rng.uniform(0.35, 3.0, (D, N)).astype(np.float32), rng.random((D, N)) < 0.5
        req = np.stack([rng.uniform(0.001, 0.999, (D, N)), rng.integers(-1, 2, (D, N))], -1).astype(np.float32)      # (p, code) requests
        if model_name == "single_trial":
            p32 = prior_util.single_prior(R, 43)
            d = np.stack([np.where(up, rt32, -rt32), np.abs(rng.normal(1.0, 0.5, (D, N)))], -1).astype(np.float32)   # (choicert, z1)
            d[:, 4::5, 0] = 0.0                                          # timeouts, censored at t_censor
            data = {"marginal": d}
        else:
            basic = model_name == "basic_ddm_dc"
            p32 = (prior_util.basic_prior if basic else prior_util.alpha_ns_prior)(R, 42)
            plain = _trials(basic, rt32, up)
            cens = plain.copy()
            if basic:
                cens[:, 4::5, 1] = 0.0                                   # censored timeouts (their gradient is not implemented: NaN)
            data = {"log_likelihood": cens, "cdf": cens, "grad": plain, "quantile": req}
        for x in (p32,) + tuple(data.values()):
            x.setflags(write=False)
        _MAPPING[model_name] = (p32, data)
    return _MAPPING[model_name]


@pytest.mark.parametrize("kernel,model_name", [(k, m) for k in ("log_likelihood", "cdf", "quantile", "grad") for m in ("basic_ddm_dc", "alpha_not_scaled")]
                         + [("marginal", "single_trial")])
def test_row_mapping_is_one_for_every_kernel_and_layout(kernel, model_name):
    """The kernels share one mapping of workgroups to rows (csrc/nddm_wiener.h: wiener_block_rows) and one tile staging.  At
    draws_per_dataset 1, 5 (paired layout), 16 (the staging threshold), 17 and 35 (ragged last chunks of 16 and of 4 rows), 1 and 3 data
    sets, and 1, 65 and 1030 trials (one lane, a second pass of the lane loop, a second LDS tile): every output of the [D * S]-row
    launch has the bits of the same rows launched with draws_per_dataset = 1 against repeated data sets, and rows 0, S - 1, S and R - 1
    have the values of a launch of that row alone (NaN where it has NaN)."""
    torch = _torch()
    from bayesflow_nddms_amd import engine
    p_all, data = _mapping_inputs(model_name)
    model = {"basic_ddm_dc": engine.BASIC_DDM_DC, "alpha_not_scaled": engine.ALPHA_NOT_SCALED, "single_trial": engine.SINGLE_TRIAL}[model_name]
    call = {"log_likelihood": lambda p, d, s: engine.wiener_log_likelihood(model, p, d, draws_per_dataset=s, per_trial=True),
            "cdf": lambda p, d, s: engine.wiener_cdf(model, p, d, draws_per_dataset=s),
            "quantile": lambda p, d, s: engine.wiener_quantile(model, p, d, draws_per_dataset=s),
            "grad": lambda p, d, s: engine.wiener_log_likelihood_grad(model, p, d, draws_per_dataset=s),
            "marginal": lambda p, d, s: engine.wiener_marginal_log_likelihood(model, p, d, draws_per_dataset=s, t_censor=4.0, per_trial=True)}[kernel]
    bits = lambda x: x.contiguous().view(torch.int64 if x.dtype == torch.float64 else torch.int32)
    p_dev, d_dev = torch.as_tensor(p_all.copy()).cuda(), torch.as_tensor(data[kernel].copy()).cuda()
    finite = 0
    for D in MAPPING_D:
        for S in MAPPING_S:
            for N in MAPPING_N:
                R = D * S
                p, d = p_dev[:R], d_dev[:D, :N].contiguous()
                full = call(p, d, S)
                paired = call(p, d.repeat_interleave(S, 0), 1)
                assert list(full) == list(paired)
                for key, x in full.items():
                    assert x.shape[0] == R and torch.equal(bits(x), bits(paired[key])), (D, S, N, key)
                    finite += int(torch.isfinite(x).sum())
                for r in sorted({0, S - 1, S if D > 1 else 0, R - 1}):
                    one = call(p[r:r + 1], d[r // S:r // S + 1], 1)
                    for key, x in full.items():
                        a, b = x[r:r + 1], one[key]
                        nan = torch.isnan(a)
                        assert torch.equal(nan, torch.isnan(b)) and torch.equal(bits(a)[~nan], bits(b)[~nan]), (D, S, N, r, key)
    assert finite > 0                                                   # (the comparisons are not of NaN alone)
