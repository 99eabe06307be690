"""CPU tests of the batched HMC sampler (nddm_wiener_hmc; csrc/nddm_wiener_hmc.h): the header's own chain compiled for the host
(tools/wiener_hmc_host.py) samples the posteriors the float64 yardsticks of tests/wiener_hmc_ref.py describe, conserves the energy its
gradient implies, and gives the same bits however a run is cut, whichever chains share a call and whatever data set lies next to it; the C
ABI and the Python adapters refuse bad input before any device work; theta <-> q round-trips; diagnostics.rhat_neff gives what the
reference's `diagnostic` gave on the recorded fixture (tests/golden/rhat_neff.npz, made by tests/golden/make_rhat_neff.py)."""
import ctypes
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import pytest

import wiener_hmc_ref as R
import wiener_ref as W
from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

HAVE_CXX = not (shutil.which("g++") is None and shutil.which("c++") is None and shutil.which("clang++") is None)
needs_cxx = pytest.mark.skipif(not HAVE_CXX, reason="no host C++ compiler")


@pytest.fixture(scope="module")
def host():
    import wiener_hmc_host as H
    with tempfile.TemporaryDirectory() as td:
        yield H, td, H.build(td), H.build(td, f64=True)


def _profile():
    import wiener_hmc_host as H
    with open(H.PROFILE) as f:
        return json.load(f)


# ---- the adapters -----------------------------------------------------------------------------------------------------------------------
def test_c_abi_exports_the_entry_and_validates_before_any_hip_call():
    from bayesflow_nddms_amd import _lib
    L = _lib.lib()
    assert "nddm_wiener_hmc" in _lib.EXPORTS and hasattr(L, "nddm_wiener_hmc")
    assert L.nddm_abi_version() == _lib.ABI_VERSION == 4
    with open(os.path.join(ROOT, "include", "nddm.h")) as f:
        assert "/* 4 (additive): nddm_wiener_hmc.  No existing entry point changes. */" in f.read()
    d = ctypes.c_void_p(16)                                             # a non-NULL pointer, never dereferenced: every case ends before a launch
    f = L.nddm_wiener_hmc

    def call(model=0, data=d, D=2, N=10, C=6, S=3, state=d, inv_mass=None, n_iter=5, n_adapt=0, L_=4, thin=1, mask=31, seed=1, coff=0, ioff=0,
             flags=0, outs=(d, None, None, None, None)):
        rc = f(model, data, D, N, C, S, state, inv_mass, n_iter, n_adapt, L_, thin, mask, seed, coff, ioff, flags, *outs, None)
        return rc, L.nddm_last_error().decode()
    E = _lib
    # the family's one order: model, flags, shape, the empty batch before any pointer, NULL inputs, NULL outputs, the stream
    for model in (1, 2, 3, 4, 7):
        rc, msg = call(model=model, flags=1, N=0, data=None)
        assert rc == E.NDDM_ERR_PARAM and msg == f"nddm_wiener_hmc: model {model} has no sampler here (NDDM_BASIC_DDM_DC only)"
    for kw in (dict(flags=1), dict(mask=32)):
        rc, msg = call(N=0, data=None, **kw)
        assert rc == E.NDDM_ERR_PARAM and msg == "nddm_wiener_hmc: flags must be 0 (reserved) and free_mask < 32"
    for kw in (dict(N=0), dict(N=2049), dict(C=5), dict(S=0), dict(C=-3, D=-1), dict(n_iter=0), dict(L_=0), dict(thin=0), dict(n_adapt=-1),
               dict(n_iter=1 << 16, L_=16), dict(N=130, n_iter=1 << 15, L_=6), dict(coff=(1 << 32) - 5), dict(ioff=(1 << 32) - 4),
               dict(D=3)):
        rc, msg = call(data=None, state=None, outs=(None,) * 5, **kw)
        assert rc == E.NDDM_ERR_SHAPE and msg.startswith("C >= 0 chains = D x chains_per_dataset > 0, 0 < n_trials <= 2048"), (kw, rc, msg)
    assert call(D=0, C=0, data=None, state=None, outs=(None,) * 5) == (E.NDDM_OK, "")       # the empty batch, before any pointer
    assert call(n_iter=1 << 15, L_=16)[0] != E.NDDM_ERR_SHAPE                               # exactly 2^19 rounds is allowed
    for kw in (dict(data=None), dict(state=None)):
        rc, msg = call(outs=(None,) * 5, **kw)
        assert rc == E.NDDM_ERR_NULL and msg == "data or state is NULL"
    rc, msg = call(outs=(None,) * 5)
    assert rc == E.NDDM_ERR_NULL and msg == "no output buffer given"
    import torch
    if not torch.cuda.is_available():                                   # everything in order: the stream check is the first HIP call
        for outs in ((d, None, None, None, None), (None, None, None, None, d)):
            assert call(outs=outs)[0] in (E.NDDM_ERR_HIP, E.NDDM_ERR_NO_DEVICE)


def test_python_adapter_refuses_bad_input_before_any_device_work():
    from bayesflow_nddms_amd import engine, mcmc
    data = np.stack([R.as_data(R.Y10)] * 2)
    st = mcmc.make_state(mcmc.hmc_init(data, 3, 0).reshape(-1, 5), np.repeat(data, 3, 0))
    ok = dict(chains_per_dataset=3, n_iter=4)
    for model in (engine.SINGLE_TRIAL, engine.SINGLE_TRIAL_ALT, engine.ALPHA_NOT_SCALED, engine.EXPLICIT_BOUNDARY):
        with pytest.raises(ValueError, match="has no sampler here"):
            engine.wiener_hmc(model, data, st, **ok)
    bad = [(dict(chains_per_dataset=0), "chains_per_dataset"), (dict(n_iter=0), "n_iter"), (dict(n_leapfrog=0), "n_iter"), (dict(thin=0), "n_iter"),
           (dict(n_adapt=-1), "n_iter"), (dict(free_mask=32), "five bits"), (dict(iter_offset=-1), "iter_offset"),
           (dict(n_iter=(1 << 15) + 1), "one launch runs at most 32768"), (dict(chain_offset=(1 << 32) - 2), "chain index")]
    for kw, words in bad:
        with pytest.raises(ValueError, match=words):
            engine.wiener_hmc(engine.BASIC_DDM_DC, data, st, **{**ok, **kw})
    for mutate, words in ((lambda x: x.__setitem__((0, 0, 1), 0.0), "timeout"), (lambda x: x.__setitem__((1, 2, 0), np.nan), "finite"),
                          (lambda x: x.__setitem__((1, 2, 0), -0.1), "> 0")):
        x = data.copy()
        mutate(x)
        with pytest.raises(ValueError, match=words):
            engine.wiener_hmc(engine.BASIC_DDM_DC, x, st, **ok)
    with pytest.raises(ValueError, match=r"data must have shape \[D, n_trials, 2\]"):
        engine.wiener_hmc(engine.BASIC_DDM_DC, data[..., :1], st, **ok)
    with pytest.raises(ValueError, match=r"n_trials must be <= 2048"):
        engine.wiener_hmc(engine.BASIC_DDM_DC, np.tile(data, (1, 300, 1)), st, **ok)
    with pytest.raises(ValueError, match=r"state must have shape \[6, 12\]"):
        engine.wiener_hmc(engine.BASIC_DDM_DC, data, st[:5], **ok)
    s2 = st.copy()
    s2[3, 2] = np.inf
    with pytest.raises(ValueError, match="state must be finite"):
        engine.wiener_hmc(engine.BASIC_DDM_DC, data, s2, **ok)
    with pytest.raises(ValueError, match=r"inv_mass must have shape \[6, 5\]"):
        engine.wiener_hmc(engine.BASIC_DDM_DC, data, st, inv_mass=np.ones((6, 4)), **ok)
    with pytest.raises(ValueError, match="inv_mass must be finite and > 0"):
        engine.wiener_hmc(engine.BASIC_DDM_DC, data, st, inv_mass=np.zeros((6, 5)), **ok)
    assert engine.wiener_hmc_max_iter(100, 16) == 16384 and engine.wiener_hmc_max_iter(64, 16) == 32768
    for kw, words in ((dict(chains=0), "chains >= 1"), (dict(samples=15, thin=10), "thin dividing samples"), (dict(free=("drift", "speed")), "unknown columns"),
                      (dict(fixed={"eta": 1.0}), "unknown fixed column")):
        with pytest.raises(ValueError, match=words):
            mcmc.hmc_fit(data, **kw)
    import bayesflow_nddms_amd as pkg
    from bayesflow_nddms_amd import basic_ddm_dc
    for name in ("wiener_hmc", "hmc_fit", "hmc_init", "theta_to_q", "q_to_theta", "rhat_neff"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    assert callable(basic_ddm_dc.fit_hmc)


def test_theta_q_round_trip_and_initial_values():
    from bayesflow_nddms_amd import mcmc
    data = np.stack([R.as_data(R.Y10), R.as_data(R.Y20)[:10], R.as_data(np.array(R.Y10) * 4.0)])      # T = .385, .359 and 1.5 (min rt 1.54)
    th = mcmc.hmc_init(data, 50, 4)
    assert th.shape == (3, 50, 5)
    mn = np.minimum(data[..., 0].min(1), 1.5)
    for j, (lo, hi) in ((0, (-4, 4)), (1, (.5, 2)), (2, (.2, .8)), (4, (.5, 2))):
        assert np.all((th[..., j] > lo) & (th[..., j] < hi)) and th[..., j].max() - th[..., j].min() > 0.8 * (hi - lo)
    assert np.all((th[..., 3] > 0) & (th[..., 3] < mn[:, None] / 2)) and np.all(th[..., 3].max(1) > 0.4 * mn)
    flat, per = th.reshape(-1, 5), np.repeat(data, 50, 0)
    q = mcmc.theta_to_q(flat, per)
    assert q.dtype == np.float64 and np.array_equal(q[:, 0], flat[:, 0])
    assert np.max(np.abs(mcmc.q_to_theta(q, per) - flat)) < 1e-14
    # the transform itself: tau = T sigmoid(q3) with T from the data, dc = .05 + 9.95 sigmoid(q4)
    assert np.allclose(flat[:, 3], mn.repeat(50) / (1 + np.exp(-q[:, 3])), rtol=0, atol=1e-15)
    assert np.allclose(flat[:, 4], 0.05 + 9.95 / (1 + np.exp(-q[:, 4])), rtol=0, atol=1e-14)
    # a fixed column keeps theta
    q3 = mcmc.theta_to_q(flat, per, free=("drift", "boundary"))
    assert np.array_equal(q3[:, 2:], flat[:, 2:]) and np.array_equal(q3[:, :2], q[:, :2])
    assert np.array_equal(mcmc.q_to_theta(q3, per, free=3)[:, 2:], flat[:, 2:])
    far = mcmc.q_to_theta(np.array([[0.0, 800.0, -800.0, 40.0, -40.0]]), data[:1])
    assert np.all(np.isfinite(far)) and far[0, 1] == 10.0 and far[0, 2] == 0.0
    bad = flat[:1].copy()
    bad[0, 3] = 0.39                                                    # beyond the smallest rt
    with pytest.raises(ValueError, match="outside the sampler's support"):
        mcmc.theta_to_q(bad, per[:1])
    st = mcmc.make_state(flat, per, eps0=0.1)
    assert st.shape == (150, 12) and np.array_equal(st[:, :5], q) and np.allclose(st[:, 5], np.log(0.1)) and np.allclose(st[:, 8], 0.0)
    assert not st[:, [6, 7, 9, 10, 11]].any()


def test_rhat_neff_gives_what_the_reference_reported_on_the_fixture():
    from bayesflow_nddms_amd import diagnostics as Dg
    g = np.load(os.path.join(GOLDEN, "rhat_neff.npz"))
    res = Dg.rhat_neff({"theta": g["in_theta"], "vector": g["in_vector"], "_hidden": g["in_vector"]})
    assert sorted(res) == ["theta", "vector"]
    for k in res:
        assert res[k]["rhat"].shape == g[f"in_{k}"].shape[:-2]
        assert np.allclose(res[k]["rhat"], g[f"rhat_{k}"], rtol=1e-12, atol=0)
        assert np.array_equal(res[k]["neff"], g[f"neff_{k}"])
        assert np.allclose(res[k]["mean"], g[f"mean_{k}"], rtol=0, atol=1e-12) and np.allclose(res[k]["std"], g[f"std_{k}"], rtol=1e-12, atol=0)
    assert g["rhat_theta"].max() > 1.3 and g["rhat_theta"].min() < 1.001 and g["neff_theta"].min() < 10 and g["neff_theta"].max() > 800
    one = Dg.rhat_neff(g["in_theta"][0, 0])                             # a bare [iterations, chains] array
    assert one["rhat"].shape == () and one["neff"] == g["neff_theta"][0, 0]
    with pytest.raises(ValueError, match="iterations >= 4, chains >= 2"):
        Dg.rhat_neff(np.zeros((100, 1)))


def test_the_yardsticks_cut_series_is_wiener_refs():
    u = np.geomspace(1e-3, 60.0, 400)[:, None]
    w = np.linspace(0.01, 0.99, 50)[None, :]
    assert np.max(np.abs(R.log_g(u, w) - W.log_g(u, w))) < 1e-12


# ---- the chain, on the host ---------------------------------------------------------------------------------------------------------------
def _fit(host, y, mask, fixed, n_sample=7500, C=64, seed=3):
    """C chains on one data set from the reference's initial values: 300 adapting iterations, then n_sample at thin 5, unit mass."""
    from bayesflow_nddms_amd import mcmc
    H, td, e32, _ = host
    data = R.as_data(y)[None]
    th = mcmc.hmc_init(data, C, seed).reshape(-1, 5)
    for k, v in fixed.items():
        th[:, mcmc.PARAM_NAMES.index(k)] = v
    st = mcmc.make_state(th, np.repeat(data, C, 0), free=mask)
    kw = dict(n_adapt=300, n_leapfrog=16, thin=5, free_mask=mask, seed=seed)
    r = H.run(e32, td, data, st, C, n_iter=300, **kw)
    return H.run(e32, td, data, r["state"], C, n_iter=n_sample, iter_offset=300, **kw), th


def check_statistics(draws, cols, mean, sd):
    """draws [C, K, 5]: Rhat < 1.02 and n_eff >= 4000 first (so that the bars below are 3 - 6 standard errors), then the pooled mean within
    0.05 sd and the pooled sd within 7 % of the yardstick's."""
    from bayesflow_nddms_amd import diagnostics as Dg
    x = draws.astype(np.float64)[:, :, cols]
    dg = Dg.rhat_neff(x.transpose(2, 1, 0))
    print("rhat", dg["rhat"], "neff", dg["neff"])
    assert np.all(dg["rhat"] < 1.02) and np.all(dg["neff"] >= 4000)
    pooled = x.reshape(-1, len(cols))
    dm, ds = (pooled.mean(0) - mean) / sd, pooled.std(0) / sd - 1.0
    print("mean error / sd", dm, "sd ratio - 1", ds)
    assert np.all(np.abs(dm) < 0.05) and np.all(np.abs(ds) < 0.07)


@needs_cxx
def test_two_free_columns_match_the_grid_quadrature(host):
    """drift and boundary free, beta, tau, dc fixed, N = 20: measured on the host build mean errors (-.004, -.002) sd, sd ratios within .001,
    n_eff 6e4 .. 9e4 of 96 000 draws.  The yardstick's last grid refinement (81 -> 161 points a side) moved its moments by 4e-14 sd."""
    m, sd, n, move = R.yardstick_2d()
    assert move < 1e-4
    assert np.allclose(m, R.recorded()["two"][0], rtol=0, atol=1e-9) and np.allclose(sd, R.recorded()["two"][1], rtol=0, atol=1e-9)
    r, th0 = _fit(host, R.Y20, 3, R.FIXED_2D)
    assert r["draws"].shape == (64, 1500, 5) and not r["flagged"].any()
    assert np.array_equal(r["draws"][:, :, 2:], np.broadcast_to(th0[:, None, 2:].astype(np.float32), (64, 1500, 3)))      # a fixed column never moves
    assert np.array_equal(r["state"][:, 2:5], th0[:, 2:])
    check_statistics(r["draws"], [0, 1], m, sd)


@needs_cxx
def test_five_free_columns_match_importance_sampling_from_the_prior(host):
    """N = 10, where the priors and the Jacobians carry weight.  The yardstick: 1 200 000 prior draws, effective size 25 174 (>= 20 000 is
    asserted).  Measured on the host build: mean errors within .006 sd, sd ratios within .008, n_eff 8.5e4 .. 1.06e5 of 96 000 draws."""
    m, sd, ess, n = R.yardstick_5d()
    print("importance sampling: draws", n, "effective size", ess)
    assert ess >= 20_000
    assert np.allclose(m, R.recorded()["five"][0], rtol=0, atol=1e-9) and np.allclose(sd, R.recorded()["five"][1], rtol=0, atol=1e-9)
    assert R.recorded()["five_ess"] >= 20_000
    r, _ = _fit(host, R.Y10, 31, {})
    assert not r["flagged"].any()
    check_statistics(r["draws"], [0, 1, 2, 3, 4], m, sd)


@needs_cxx
@pytest.mark.parametrize("N", [1, 20, 64, 65, 130])
def test_energy_error_of_short_trajectories_stays_under_the_recorded_bar(host, N):
    """eps = 1e-3, 8 leapfrog steps, no adaptation, 256 chains, 4 iterations: |H1 - H0| under the bar recorded by tools/wiener_hmc_host.py
    (4 x the host build's largest, per shape).  A gradient that is not the potential's -- a missing Jacobian or prior term -- shows here."""
    H, td, e32, _ = host
    data, theta = H.case(N)
    r = H.run(e32, td, data, H.init_state(theta, data, 64, eps0=1e-3), 64, **H.ENERGY)
    worst = float(np.max(r["state"][:, 11]))
    print("N", N, "largest |H1 - H0|", worst)
    assert not r["flagged"].any() and not r["divergent"].any() and np.all(np.isfinite(r["state"][:, 10:]))
    assert worst <= _profile()["energy_bar"][str(N)]


@needs_cxx
@pytest.mark.parametrize("N", [1, 20, 130])
def test_energy_error_falls_with_the_square_of_the_step(host, N):
    """The leapfrog integrator is second order ONLY when the gradient is the potential's: over a fixed trajectory length the energy error
    quarters when eps halves; with any term of the gradient missing or mis-scaled the error has a first-order part and merely halves.  In
    the float64 build of the likelihood's arithmetic the median ratio is 4 to three digits (measured 4.000 - 4.009); asserted 3.9 .. 4.1."""
    H, td, _, e64 = host
    data, theta = H.case(N)
    err = []
    for eps in (4e-3, 2e-3, 1e-3):
        r = H.run(e64, td, data, H.init_state(theta, data, 64, eps0=eps), 64, n_iter=1, n_leapfrog=int(round(8e-3 / eps)), seed=11)
        err.append(np.abs(r["state"][:, 10]))
    ratios = [float(np.median(err[i] / err[i + 1])) for i in range(2)]
    print("N", N, "median ratios", ratios)
    assert all(3.9 < x < 4.1 for x in ratios)


def _bits_case(H, C=32, N=65):
    return H.case(N, C=C, D=4, seed=17)


SAME = ("draws", "log_post", "divergent", "flagged", "state")


@needs_cxx
def test_cut_runs_give_the_bits_of_the_uncut_run(host):
    """40 iterations, 25 of them adapting, thin 3: one call, two calls (cut inside the adaptation) and five (one cut on the border)."""
    H, td, e32, _ = host
    data, theta = _bits_case(H)
    st = H.init_state(theta, data, 8)
    kw = dict(n_adapt=25, n_leapfrog=5, thin=3, seed=21)
    whole = H.run(e32, td, data, st, 8, n_iter=40, **kw)
    assert whole["draws"].shape == (32, 13, 5) and np.all(whole["state"][:, 9] == 25)
    for cuts in ((17, 23), (7, 8, 10, 4, 11)):
        parts, s, off = [], st, 0
        for n in cuts:
            r = H.run(e32, td, data, s, 8, n_iter=n, iter_offset=off, **kw)
            parts.append(r)
            s, off = r["state"], off + n
        assert np.array_equal(np.concatenate([p["draws"] for p in parts], 1), whole["draws"])
        assert np.array_equal(np.concatenate([p["log_post"] for p in parts], 1), whole["log_post"])
        assert np.array_equal(s, whole["state"]) and np.array_equal(sum(p["divergent"] for p in parts), whole["divergent"])
    # the acceptance mean is of the call's own non-adapting iterations: NaN where there are none
    assert np.all(np.isnan(H.run(e32, td, data, st, 8, n_iter=10, **kw)["accept"])) and np.all(np.isfinite(whole["accept"]))


@needs_cxx
def test_chains_do_not_depend_on_their_neighbours(host):
    """32 chains in one call equal 2 x 16 with chain_offset; a data set that cannot be sampled changes no bit of the two beside it."""
    H, td, e32, _ = host
    data, theta = _bits_case(H)
    st = H.init_state(theta, data, 8)
    kw = dict(n_iter=12, n_adapt=6, n_leapfrog=5, thin=2, seed=22)
    whole = H.run(e32, td, data, st, 8, chain_offset=100, **kw)
    halves = [H.run(e32, td, data[2 * h:2 * h + 2], st[16 * h:16 * h + 16], 8, chain_offset=100 + 16 * h, **kw) for h in range(2)]
    for k in SAME + ("accept",):
        assert np.array_equal(np.concatenate([h[k] for h in halves]), whole[k], equal_nan=True), k
    assert not np.array_equal(whole["draws"], H.run(e32, td, data, st, 8, chain_offset=101, **kw)["draws"])       # (the stream is the chain's)
    for mutate in (lambda x: x.__setitem__((1, 3, 1), 0.0), lambda x: x.__setitem__((1, 64, 0), np.nan), lambda x: x.__setitem__((1, 0, 0), 0.0)):
        x = data.copy()
        mutate(x)
        r = H.run(e32, td, x, st, 8, chain_offset=100, **kw)
        bad = np.arange(32) // 8 == 1
        assert np.array_equal(r["flagged"], bad.astype(np.int32))
        assert np.all(np.isnan(r["draws"][bad])) and np.all(np.isnan(r["log_post"][bad])) and np.array_equal(r["state"][bad], st[bad])
        for k in SAME:
            assert np.array_equal(r[k][~bad], whole[k][~bad]), k
    s2 = st.copy()
    s2[5, 1] = np.nan
    r = H.run(e32, td, data, s2, 8, chain_offset=100, **kw)
    assert r["flagged"].sum() == 1 and r["flagged"][5] == 1 and np.all(np.isnan(r["draws"][5]))
    assert np.array_equal(r["state"][5], s2[5], equal_nan=True) and np.array_equal(np.delete(r["draws"], 5, 0), np.delete(whole["draws"], 5, 0))


@needs_cxx
def test_free_mask_fixes_columns_and_inverse_mass_scales_the_momentum(host):
    H, td, e32, _ = host
    data, theta = _bits_case(H)
    st = H.init_state(theta, data, 8, free=0b01101)
    st[:, [1, 4]] = theta[:, [1, 4]]
    r = H.run(e32, td, data, st, 8, n_iter=20, n_leapfrog=4, free_mask=0b01101, seed=5)
    assert np.array_equal(r["state"][:, [1, 4]], theta[:, [1, 4]])
    assert np.array_equal(r["draws"][:, :, [1, 4]], np.broadcast_to(theta[:, None, [1, 4]].astype(np.float32), (32, 20, 2)))
    assert np.all(np.ptp(r["draws"][:, :, [0, 2, 3]], axis=1).max(0) > 0)
    # unit inverse mass given explicitly is the NULL default; another one changes the trajectories
    ones = H.run(e32, td, data, st, 8, inv_mass=np.ones((32, 5)), n_iter=20, n_leapfrog=4, free_mask=0b01101, seed=5)
    assert np.array_equal(ones["draws"], r["draws"])
    other = H.run(e32, td, data, st, 8, inv_mass=np.full((32, 5), 0.25), n_iter=20, n_leapfrog=4, free_mask=0b01101, seed=5)
    assert not np.array_equal(other["draws"], r["draws"])


@needs_cxx
def test_float32_and_float64_builds_agree_within_the_recorded_tolerance(host):
    """The device test's tolerance is 4 x what this comparison shows (tools/wiener_hmc_host.py records it); here: the float32 build stays
    inside it against the float64 build of the same arithmetic, and the chains left out because an accept decision flipped are under 2 %."""
    H, td, e32, e64 = host
    P = _profile()
    for N in H.ENERGY_SHAPES:
        data, theta = H.case(N)
        st = H.init_state(theta, data, 64, eps0=0.02)
        same, dl, dd = H.compare(H.run(e32, td, data, st, 64, **H.COMPARE), H.run(e64, td, data, st, 64, **H.COMPARE), theta)
        print("N", N, "left out", int((~same).sum()), "log_post", dl, "draws", dd)
        assert (~same).mean() <= 0.02 and dl <= P["device_tolerance_log_post_rel"] and dd <= P["device_tolerance_draw_abs"]


@needs_cxx
def test_hmc_fit_on_the_host_build_returns_the_jags_layout(host):
    """mcmc.hmc_fit with the host chain in the device call's place (2 participants x 40 trials, 4 chains, 300 + 500 iterations): the
    reference's layout, Rhat < 1.05 on every variable, and the acceptance rate in the [0.6, 0.95] band the device test asserts."""
    from bayesflow_nddms_amd import diagnostics as Dg, mcmc
    H, td, e32, _ = host
    data = H.example_data(2, 40, 31)

    def call(model, d, state, want_draws=True, want_log_post=True, **kw):
        return H.run(e32, td, d, state, **kw)
    fit = mcmc.hmc_fit(data, chains=4, warmup=300, samples=500, thin=5, seed=8, _call=call)
    fixed = mcmc.hmc_fit(data[:1], chains=2, warmup=40, samples=20, thin=5, seed=8, fixed={"dc": 1.0}, _call=call)
    assert np.all(fixed["varsigma"] == 1.0) and np.ptp(fixed["alpha"]) > 0
    for k in ("alpha", "ndt", "beta", "delta", "varsigma", "log_post"):
        assert fit[k].shape == (2, 100, 4) and fit[k].dtype == np.float64 and np.all(np.isfinite(fit[k]))
    assert fit["accept_rate"].shape == fit["n_divergent"].shape == fit["flagged"].shape == (2, 4) and not fit["flagged"].any()
    dg = Dg.rhat_neff({k: fit[k] for k in ("alpha", "ndt", "beta", "delta", "varsigma")})
    print({k: v["rhat"] for k, v in dg.items()}, fit["accept_rate"])
    assert all(np.all(v["rhat"] < 1.05) for v in dg.values())
    assert np.all((fit["accept_rate"] >= 0.6) & (fit["accept_rate"] <= 0.95))
