"""CPU tests of the joint sampler (nddm_wiener_hmc_joint; csrc/nddm_wiener_hmc_joint.h): the header's own participant and sigma steps
compiled for the host (tools/wiener_hmc_joint_host.py) sample the posteriors the float64 yardsticks of tests/wiener_hmc_joint_ref.py
describe, equal the independent sampler bit for bit when the ext term vanishes, conserve the energy the gradient with the ext term
implies, and give the same bits however a run is cut and whatever the other joint chains hold; the C ABI and the Python adapters refuse bad
input before any device work."""
import ctypes
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import pytest

import wiener_hmc_joint_ref as JR
import wiener_hmc_ref as R
from conftest import ROOT
from test_wiener_hmc_host import check_statistics

sys.path.insert(0, os.path.join(ROOT, "tools"))

HAVE_CXX = not (shutil.which("g++") is None and shutil.which("c++") is None and shutil.which("clang++") is None)
needs_cxx = pytest.mark.skipif(not HAVE_CXX, reason="no host C++ compiler")


@pytest.fixture(scope="module")
def host():
    import wiener_hmc_host as H
    import wiener_hmc_joint_host as J
    with tempfile.TemporaryDirectory() as td:
        yield J, td, J.build(td), J.build(td, f64=True), H, H.build(td)


def _profile():
    import wiener_hmc_joint_host as J
    with open(J.PROFILE) as f:
        return json.load(f)


# ---- the adapters -----------------------------------------------------------------------------------------------------------------------
def test_c_abi_exports_the_entry_and_validates_before_any_hip_call():
    from bayesflow_nddms_amd import _lib
    L = _lib.lib()
    assert "nddm_wiener_hmc_joint" in _lib.EXPORTS and hasattr(L, "nddm_wiener_hmc_joint")
    assert L.nddm_abi_version() == _lib.ABI_VERSION == 4
    with open(os.path.join(ROOT, "include", "nddm.h")) as f:
        assert "/* 4 (additive): nddm_wiener_hmc_joint.  No existing entry point changes. */" in f.read()
    d = ctypes.c_void_p(16)                                             # a non-NULL pointer, never dereferenced: every case ends before a launch
    f = L.nddm_wiener_hmc_joint

    def call(model=0, data=d, P=2, N=10, C=6, S=3, ext=d, state=d, inv_mass=None, sigma=d, ws=d, n_iter=5, n_adapt=0, L_=4, thin=1, mask=31, seed=1,
             coff=0, ioff=0, flags=0, outs=(d,) + (None,) * 6):
        rc = f(model, data, P, N, C, S, ext, state, inv_mass, sigma, ws, n_iter, n_adapt, L_, thin, mask, seed, coff, ioff, flags, *outs, None)
        return rc, L.nddm_last_error().decode()
    E = _lib
    none = (None,) * 7
    # nddm_wiener_hmc's order: model, flags, shape, the empty batch before any pointer, NULL inputs, NULL outputs, the stream
    for model in (1, 2, 3, 4, 7):
        rc, msg = call(model=model, flags=2, N=0, data=None)
        assert rc == E.NDDM_ERR_PARAM and msg == f"nddm_wiener_hmc_joint: model {model} has no sampler here (NDDM_BASIC_DDM_DC only)"
    for kw in (dict(flags=2), dict(flags=3), dict(mask=32)):
        rc, msg = call(N=0, data=None, **kw)
        assert rc == E.NDDM_ERR_PARAM and msg == "nddm_wiener_hmc_joint: flags must be 0 or NDDM_HMC_SIGMA_FIXED and free_mask < 32"
    for kw in (dict(N=0), dict(N=2049), dict(C=5), dict(S=0), dict(C=-3, P=-1), dict(n_iter=0), dict(L_=0), dict(thin=0), dict(n_adapt=-1),
               dict(n_iter=4097, L_=1), dict(N=130, n_iter=4096, L_=64), dict(coff=(1 << 32) - 5), dict(ioff=(1 << 32) - 4), dict(P=3),
               dict(P=1, C=3), dict(P=1, C=3, flags=1, n_iter=4097)):
        rc, msg = call(data=None, state=None, outs=none, **kw)
        assert rc == E.NDDM_ERR_SHAPE and msg.startswith("C >= 0 chains = P x chains > 0 (P >= 2 when sigma is sampled)"), (kw, rc, msg)
    assert call(P=0, C=0, data=None, state=None, outs=none) == (E.NDDM_OK, "")              # the empty batch, before any pointer
    assert call(P=1, C=3, flags=1, outs=none)[0] == E.NDDM_ERR_NULL                         # one participant is enough when sigma is held
    assert call(n_iter=4096, L_=1, outs=none)[0] == E.NDDM_ERR_NULL                         # exactly 4096 iterations is allowed
    for kw in (dict(data=None), dict(state=None), dict(ext=None), dict(sigma=None), dict(ws=None)):
        rc, msg = call(outs=none, **kw)
        assert rc == E.NDDM_ERR_NULL and msg == "data, extdata, state, sigma or workspace is NULL"
    rc, msg = call(outs=none)
    assert rc == E.NDDM_ERR_NULL and msg == "no output buffer given"
    import torch
    if not torch.cuda.is_available():                                   # everything in order: the stream check is the first HIP call
        for outs in ((d,) + (None,) * 6, (None,) * 5 + (d, None), (None,) * 6 + (d,)):
            assert call(outs=outs)[0] in (E.NDDM_ERR_HIP, E.NDDM_ERR_NO_DEVICE)


def test_python_adapters_refuse_bad_input_before_any_device_work():
    from bayesflow_nddms_amd import alpha_not_scaled, engine, mcmc
    data = np.stack([R.as_data(R.Y10), R.as_data(JR.Y10[1])])
    ext = np.array([1.2, 0.7])
    theta, sigma = mcmc.hmc_init_joint(data, 3, 0)
    assert theta.shape == (2, 3, 5) and sigma.shape == (3,) and np.all((sigma > 0.01) & (sigma < 5.0))
    assert np.array_equal(theta, mcmc.hmc_init(data, 3, 0))
    big = mcmc.hmc_init_joint(data, 400, 1)[1]
    assert big.min() < 0.3 and big.max() > 4.7 and np.all((big > 0.01) & (big < 5.0))
    st = mcmc.make_state(theta.reshape(-1, 5), np.repeat(data, 3, 0))
    M = engine.BASIC_DDM_DC
    ok = dict(n_iter=4)
    for model in (engine.SINGLE_TRIAL, engine.SINGLE_TRIAL_ALT, engine.ALPHA_NOT_SCALED, engine.EXPLICIT_BOUNDARY):
        with pytest.raises(ValueError, match="has no sampler here"):
            engine.wiener_hmc_joint(model, data, ext, st, sigma, **ok)
    bad = [(dict(n_iter=0), "n_iter"), (dict(n_leapfrog=0), "n_iter"), (dict(thin=0), "n_iter"), (dict(n_adapt=-1), "n_iter"),
           (dict(free_mask=32), "five bits"), (dict(iter_offset=-1), "iter_offset"), (dict(n_iter=4097), "one call runs at most 4096"),
           (dict(chain_offset=(1 << 32) - 2), "chain index")]
    for kw, words in bad:
        with pytest.raises(ValueError, match=words):
            engine.wiener_hmc_joint(M, data, ext, st, sigma, **{**ok, **kw})
    assert engine.wiener_hmc_joint_max_iter(100, 16) == 4096 and engine.wiener_hmc_joint_max_iter(2048, 16) == 1024
    for mutate, words in ((lambda x: x.__setitem__((0, 0, 1), 0.0), "timeout"), (lambda x: x.__setitem__((1, 2, 0), np.nan), "finite"),
                          (lambda x: x.__setitem__((1, 2, 0), -0.1), "> 0")):
        x = data.copy()
        mutate(x)
        with pytest.raises(ValueError, match=words):
            engine.wiener_hmc_joint(M, x, ext, st, sigma, **ok)
    with pytest.raises(ValueError, match=r"data must have shape \[P, n_trials, 2\]"):
        engine.wiener_hmc_joint(M, data[..., :1], ext, st, sigma, **ok)
    with pytest.raises(ValueError, match="at least 2 participants"):
        engine.wiener_hmc_joint(M, data[:1], ext[:1], st[:3], sigma, **ok)
    with pytest.raises(ValueError, match=r"state must have shape \[6, 12\]"):
        engine.wiener_hmc_joint(M, data, ext, st[:5], sigma, **ok)
    with pytest.raises(ValueError, match=r"extdata must have shape \[2\]"):
        engine.wiener_hmc_joint(M, data, np.ones(3), st, sigma, **ok)
    with pytest.raises(ValueError, match="extdata must be finite"):
        engine.wiener_hmc_joint(M, data, np.array([1.0, np.inf]), st, sigma, **ok)
    with pytest.raises(ValueError, match=r"sigma must have shape \[S\]"):
        engine.wiener_hmc_joint(M, data, ext, st, 1.0, **ok)
    for s_bad, kw in ((np.array([1.0, -1.0, 2.0]), {}), (np.array([1.0, np.nan, 2.0]), {}), (np.array([1.0, 10.0, 2.0]), {}),
                      (np.array([1.0, 0.0, 2.0]), dict(sigma_fixed=True))):
        with pytest.raises(ValueError, match="sigma must be finite and > 0"):
            engine.wiener_hmc_joint(M, data, ext, st, s_bad, **ok, **kw)
    s2 = st.copy()
    s2[3, 2] = np.inf
    with pytest.raises(ValueError, match="state must be finite"):
        engine.wiener_hmc_joint(M, data, ext, s2, sigma, **ok)
    with pytest.raises(ValueError, match=r"inv_mass must have shape \[6, 5\]"):
        engine.wiener_hmc_joint(M, data, ext, st, sigma, inv_mass=np.ones((6, 4)), **ok)
    with pytest.raises(ValueError, match="inv_mass must be finite and > 0"):
        engine.wiener_hmc_joint(M, data, ext, st, sigma, inv_mass=np.zeros((6, 5)), **ok)
    for kw, words in ((dict(chains=0), "chains >= 1"), (dict(samples=15, thin=10), "thin dividing samples"), (dict(free=("drift", "speed")), "unknown columns"),
                      (dict(fixed={"eta": 1.0}), "unknown fixed column"), (dict(fixed={"sigma": 0.0}), "fixed sigma")):
        with pytest.raises(ValueError, match=words):
            mcmc.hmc_fit_joint(data, ext, **kw)
    with pytest.raises(ValueError, match="one finite value per participant"):
        mcmc.hmc_fit_joint(data, ext[:1])
    with pytest.raises(ValueError, match="at least 2 participants"):
        mcmc.hmc_fit_joint(data[:1], ext[:1])
    with pytest.raises(ValueError, match="extdata"):
        alpha_not_scaled.fit_hmc(np.ones((2, 5)))
    import bayesflow_nddms_amd as pkg
    for name in ("wiener_hmc_joint", "hmc_fit_joint", "hmc_init_joint"):
        assert name in pkg.__all__ and hasattr(pkg, name)


# ---- the yardsticks ---------------------------------------------------------------------------------------------------------------------
def test_yardstick_a_is_converged_recorded_and_far_from_the_prior():
    """The last refinement (81 -> 161 points a side, 500 -> 1000 of sigma) moves no moment by 1e-4 sd (measured 1e-10); sigma's posterior mean lies more than
    0.3 from its prior's 3.0, so a sampler that ignored the coupling fails the statistics test."""
    m, sd, n, ns, move = JR.yardstick_a()
    print("grid", n, "sigma grid", ns, "last move", move, "sigma", m[-1], sd[-1])
    assert move < 1e-4
    assert abs(m[-1] - 3.0) >= 0.3
    rec = JR.recorded()
    assert np.allclose(m, rec["a"][0], rtol=0, atol=1e-9) and np.allclose(sd, rec["a"][1], rtol=0, atol=1e-9)


def test_yardstick_b_has_the_projects_effective_size_and_is_recorded():
    m, sd, ess, n = JR.yardstick_b()
    print("importance sampling: draws", n, "effective size", ess)
    assert min(ess) >= 20_000
    rec = JR.recorded()
    assert np.allclose(m, rec["b"][0], rtol=0, atol=1e-9) and np.allclose(sd, rec["b"][1], rtol=0, atol=1e-9) and min(rec["b_ess"]) >= 20_000


# ---- the sampler, on the host -----------------------------------------------------------------------------------------------------------
def run_cut(run, data, ext, state, sigma, n_iter, iter_offset=0, step=4096, **kw):
    """n_iter iterations as calls of at most `step` -> the last call's dict with 'draws', 'log_post' and 'sigma_draws' concatenated."""
    parts, done = [], 0
    while done < n_iter:
        n = min(step, n_iter - done)
        r = run(data, ext, state, sigma, n_iter=n, iter_offset=iter_offset + done, **kw)
        parts.append(r)
        state, sigma, done = r["state"], r["sigma"], done + n
    out = dict(parts[-1])
    for k in ("draws", "log_post", "sigma_draws"):
        if k in out:
            out[k] = np.concatenate([p[k] for p in parts], 1)
    out["divergent"] = sum(p["divergent"] for p in parts)
    return out


def fit_joint(run, ys, ext, mask, fixed, sigma=None, S=64, n_sample=7500, seed=3):
    """S joint chains from the reference's initial values: 300 adapting iterations, then n_sample at thin 5, unit mass.  sigma: held there."""
    from bayesflow_nddms_amd import mcmc
    data = np.stack([R.as_data(y) for y in ys])
    th, sg = mcmc.hmc_init_joint(data, S, seed)
    for k, v in fixed.items():
        th[..., mcmc.PARAM_NAMES.index(k)] = v
    st = mcmc.make_state(th.reshape(-1, 5), np.repeat(data, S, 0), free=mask)
    kw = dict(n_adapt=300, n_leapfrog=16, thin=5, free_mask=mask, seed=seed, sigma_fixed=sigma is not None)
    if sigma is not None:
        sg = np.full(S, sigma)
    r = run(data, ext, st, sg, n_iter=300, **kw)
    return run_cut(run, data, np.asarray(ext), r["state"], r["sigma"], n_sample, iter_offset=300, **kw)


def check_a(r, S=64):
    m, sd = JR.recorded()["a"]
    assert not r["flagged"].any() and np.all(np.isfinite(r["draws"])) and np.all(np.isfinite(r["sigma_draws"]))
    for p in range(4):
        check_statistics(r["draws"][p * S:(p + 1) * S], [0, 1], m[2 * p:2 * p + 2], sd[2 * p:2 * p + 2])
    check_statistics(r["sigma_draws"][:, :, None], [0], m[8:], sd[8:])
    print("sigma accept", r["sigma_accept"].mean())


def check_b(r, S=64):
    m, sd = JR.recorded()["b"]
    assert not r["flagged"].any() and np.all(r["sigma_draws"] == np.float32(JR.SIGMA_B)) and np.all(r["sigma"] == JR.SIGMA_B)
    assert np.all(np.isnan(r["sigma_accept"]))
    for p in range(2):
        check_statistics(r["draws"][p * S:(p + 1) * S], [0, 1, 2, 3, 4], m[p], sd[p])


def _host_run(host):
    J, td, e32 = host[:3]
    return lambda data, ext, state, sigma, **kw: J.run(e32, td, data, ext, state, sigma, **kw)


@needs_cxx
def test_free_drift_boundary_and_sigma_match_the_nested_quadrature(host):
    """(a): 4 participants x 20 trials, 64 joint chains, 300 + 7500 iterations at thin 5: check_statistics' bars, unchanged, on every v_p,
    alpha_p and on sigma.  Measured on the host build: DESIGN.md section 18."""
    check_a(fit_joint(_host_run(host), JR.Y20, JR.EXT_A, 3, JR.FIXED_2D))


@needs_cxx
def test_five_free_columns_with_sigma_fixed_match_importance_sampling(host):
    """(b): 2 participants x 10 trials, sigma held at 0.3, all five columns free."""
    check_b(fit_joint(_host_run(host), JR.Y10, JR.EXT_B, 31, {}, sigma=JR.SIGMA_B))


TIE = dict(n_adapt=6, n_leapfrog=5, thin=2, seed=22)


@needs_cxx
@pytest.mark.parametrize("N", [1, 20, 65, 130])
@pytest.mark.parametrize("S", [1, 3])
def test_a_vanishing_ext_term_gives_the_independent_samplers_bits(host, N, S):
    """NDDM_HMC_SIGMA_FIXED and sigma = 1e150: the ext term is below half an ulp of every sum it joins, so draws, log_post, states, divergent
    counts and accept equal nddm_wiener_hmc's for the same data, states, seed and offsets -- 12 launches of one iteration against one of 12."""
    J, td, e32, _, H, h32 = host
    data, ext, theta = J.case(N, 3, S)
    st = H.init_state(theta, data, S)
    a = J.run(e32, td, data, ext, st, np.full(S, 1e150), n_iter=12, chain_offset=100, iter_offset=4, sigma_fixed=True, **TIE)
    b = H.run(h32, td, data, st, S, n_iter=12, chain_offset=100, iter_offset=4, **TIE)
    for k in ("draws", "log_post", "state", "divergent", "flagged", "accept"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert a["draws"].shape == (3 * S, 6, 5) and np.ptp(a["draws"][:, :, 0], axis=1).min() > 0


CUT = dict(n_adapt=25, n_leapfrog=5, thin=3, seed=21)
BITS = ("draws", "log_post", "sigma_draws")


def bits_case(J, H, N=65, P=5, S=4):
    data, ext, theta = J.case(N, P, S, seed=17)
    return data, ext, H.init_state(theta, data, S), np.linspace(0.5, 2.0, S)


def check_cut(run, J, H):
    data, ext, st, sg = bits_case(J, H)
    whole = run(data, ext, st, sg, n_iter=40, **CUT)
    assert whole["draws"].shape == (20, 13, 5) and whole["sigma_draws"].shape == (4, 13) and np.all(whole["state"][:, 9] == 25)
    assert np.any(np.ptp(whole["sigma_draws"], axis=1) > 0) and np.all(np.isfinite(whole["draws"]))       # (sigma is being sampled)
    for cuts in ((17, 23), (7, 8, 10, 4, 11)):
        parts, s, g, off = [], st, sg, 0
        for n in cuts:
            r = run(data, ext, s, g, n_iter=n, iter_offset=off, **CUT)
            parts.append(r)
            s, g, off = r["state"], r["sigma"], off + n
        for k in BITS:
            assert np.array_equal(np.concatenate([p[k] for p in parts], 1), whole[k]), k
        assert np.array_equal(s, whole["state"]) and np.array_equal(g, whole["sigma"])
        assert np.array_equal(sum(p["divergent"] for p in parts), whole["divergent"])


def check_neighbours(run, J, H, device_inputs=lambda st, sg: (st, sg)):
    """Joint chain k's bits do not depend on joint chain k': alone in a call (with its chain_offset), beside a NaN state, beside sigma = -1;
    a bad data set flags every chain."""
    data, ext, st, sg = bits_case(J, H)
    P, S = 5, 4
    kw = dict(n_iter=12, n_adapt=6, n_leapfrog=5, thin=2, seed=22)
    whole = run(data, ext, st, sg, **kw)
    rows = lambda k: np.arange(P) * S + k
    # purity: joint chain k is a function of (chain_offset + c) for its participants and (chain_offset + k) for sigma -- so of S as well;
    # a neighbour with other values changes nothing
    s2, g2 = st.copy(), sg.copy()
    s2[rows(1), 0] += 0.3
    g2[3] = 4.0
    r = run(data, ext, s2, g2, **kw)
    for k in (0, 2):
        assert all(np.array_equal(r[x][rows(k)], whole[x][rows(k)]) for x in ("draws", "log_post", "state")), k
        assert np.array_equal(r["sigma_draws"][k], whole["sigma_draws"][k]) and r["sigma"][k] == whole["sigma"][k]
    assert not np.array_equal(r["draws"][rows(1)], whole["draws"][rows(1)]) and not np.array_equal(r["sigma_draws"][3], whole["sigma_draws"][3])
    for which in ("state", "sigma"):
        s2, g2 = st.copy(), sg.copy()
        if which == "state":
            s2[2 * S + 1, 1] = np.nan
        else:
            g2[1] = -1.0
        r = run(data, ext, *device_inputs(s2, g2), **kw)
        bad = np.arange(P * S) % S == 1
        assert np.array_equal(r["flagged"], bad.astype(np.int32))
        assert np.all(np.isnan(r["draws"][bad])) and np.all(np.isnan(r["log_post"][bad])) and np.all(np.isnan(r["sigma_draws"][1]))
        assert np.array_equal(r["state"][bad], s2[bad], equal_nan=True) and r["sigma"][1] == g2[1]
        assert np.all(np.isnan(r["accept"][bad])) and np.isnan(r["sigma_accept"][1])
        for x in ("draws", "log_post", "state", "divergent", "accept"):
            assert np.array_equal(r[x][~bad], whole[x][~bad]), x
        assert np.array_equal(np.delete(r["sigma_draws"], 1, 0), np.delete(whole["sigma_draws"], 1, 0))
        assert np.array_equal(np.delete(r["sigma_accept"], 1), np.delete(whole["sigma_accept"], 1))
    return data, ext, st, sg, kw


def check_bad_data(run, J, H):
    data, ext, st, sg = bits_case(J, H)
    for mutate in (lambda x: x.__setitem__((1, 3, 1), 0.0), lambda x: x.__setitem__((4, 64, 0), np.nan), lambda x: x.__setitem__((0, 0, 0), 0.0)):
        x = data.copy()
        mutate(x)
        r = run(x, ext, st, sg, n_iter=4, n_leapfrog=3, thin=2, seed=1)
        assert r["flagged"].all() and np.all(np.isnan(r["draws"])) and np.all(np.isnan(r["sigma_draws"]))
        assert np.array_equal(r["state"], st) and np.array_equal(r["sigma"], sg)


@needs_cxx
def test_cut_runs_give_the_bits_of_the_uncut_run(host):
    """40 iterations, 25 of them adapting, thin 3, sigma sampled: one call, two (cut inside the adaptation) and five (one cut on the border)."""
    check_cut(_host_run(host), host[0], host[4])


@needs_cxx
def test_joint_chains_do_not_depend_on_their_neighbours(host):
    check_neighbours(_host_run(host), host[0], host[4])


@needs_cxx
def test_a_bad_data_set_flags_every_chain(host):
    check_bad_data(_host_run(host), host[0], host[4])


@needs_cxx
@pytest.mark.parametrize("N", [1, 20, 64, 65, 130])
def test_energy_error_with_the_ext_term_stays_under_the_recorded_bar(host, N):
    """sigma = 0.2 (the ext term's curvature 25 against the prior's 4), eps = 1e-3, 8 leapfrog steps, 4 iterations, 256 chains: |H1 - H0| under
    the bar tools/wiener_hmc_joint_host.py recorded (4 x the host build's largest, per shape)."""
    J, td, e32, _, H, _ = host
    data, ext, theta = J.energy_case(N)
    r = J.run(e32, td, data, ext, H.init_state(theta, data, 64, eps0=1e-3), np.full(64, J.ENERGY_SIGMA), **J.ENERGY)
    worst = float(np.max(r["state"][:, 11]))
    print("N", N, "largest |H1 - H0|", worst)
    assert not r["flagged"].any() and not r["divergent"].any() and np.all(np.isfinite(r["state"][:, 10:]))
    assert worst <= _profile()["energy_bar"][str(N)]


@needs_cxx
@pytest.mark.parametrize("N", [1, 20, 130])
def test_energy_error_with_the_ext_term_falls_with_the_square_of_the_step(host, N):
    """With the ext term in the potential but not in the gradient (or mis-scaled) the error has a first-order part; in the float64 build the
    median ratio of the errors at eps and eps / 2 over a fixed trajectory length is asserted in 3.9 .. 4.1."""
    J, td, _, e64, H, _ = host
    data, ext, theta = J.energy_case(N)
    err = []
    for eps in (4e-3, 2e-3, 1e-3):
        r = J.run(e64, td, data, ext, H.init_state(theta, data, 64, eps0=eps), np.full(64, J.ENERGY_SIGMA), n_iter=1,
                  n_leapfrog=int(round(8e-3 / eps)), seed=11, sigma_fixed=True)
        err.append(np.abs(r["state"][:, 10]))
    ratios = [float(np.median(err[i] / err[i + 1])) for i in range(2)]
    print("N", N, "median ratios", ratios)
    assert all(3.9 < x < 4.1 for x in ratios)


@needs_cxx
def test_float32_and_float64_builds_agree_within_the_recorded_tolerances(host):
    """The device test's tolerance is, case by case, 4 x what this comparison shows (tools/wiener_hmc_joint_host.py records it); the chains
    left out because an accept decision flipped are under 2 % over the cases."""
    J, td, e32, e64, H, _ = host
    P_ = _profile()
    left, total = 0, 0
    for N, P, S in J.COMPARE_CASES:
        data, ext, theta = J.case(N, P, S)
        st = H.init_state(theta, data, S, eps0=0.02)
        sg = np.full(S, J.COMPARE_SIGMA)
        same, dl, dq, same_k, ds = J.compare(J.run(e32, td, data, ext, st, sg, **J.COMPARE), J.run(e64, td, data, ext, st, sg, **J.COMPARE), theta)
        tol = P_["device_tolerance"][f"N{N}_P{P}_S{S}"]
        print(N, P, S, "left out", int((~same).sum()), dl, dq, ds)
        assert dl <= tol["log_post_rel"] and dq <= tol["q_abs"] and ds <= tol["sigma_abs"]
        left, total = left + int((~same).sum()), total + P * S
    assert left <= 0.02 * total and P_["left_out_share"] <= 0.02


def check_fit(fit, P):
    from bayesflow_nddms_amd import diagnostics as Dg
    names = ("alpha", "ndt", "beta", "delta", "varsigma")
    for k in names + ("log_post",):
        assert fit[k].shape == (P, 100, 4) and fit[k].dtype == np.float64 and np.all(np.isfinite(fit[k]))
    assert fit["sigma"].shape == (1, 100, 4) and fit["sigma"].dtype == np.float64 and np.all(np.isfinite(fit["sigma"]))
    assert np.all((fit["sigma"] > 0) & (fit["sigma"] < 10)) and fit["sigma_accept"].shape == (4,)
    assert fit["accept_rate"].shape == fit["n_divergent"].shape == fit["flagged"].shape == (P, 4) and not fit["flagged"].any()
    dg = Dg.rhat_neff({k: fit[k] for k in names + ("sigma",)})          # (sigma as it stands: a [1, K, chains] node, pyjags' scalar shape)
    assert dg["sigma"]["rhat"].shape == (1,) and dg["alpha"]["rhat"].shape == (P,)
    print({k: np.max(dg[k]["rhat"]) for k in names + ("sigma",)}, fit["accept_rate"].min(), fit["accept_rate"].max(), fit["sigma_accept"])
    assert all(np.all(dg[k]["rhat"] < 1.05) for k in names + ("sigma",))
    assert np.all((fit["accept_rate"] >= 0.6) & (fit["accept_rate"] <= 0.95))


def fit_data():
    import wiener_hmc_host as H
    return H.example_data(3, 40, 31), np.array([1.3, 0.9, 1.6])


@needs_cxx
def test_hmc_fit_joint_on_the_host_build_returns_the_jags_layout(host):
    """mcmc.hmc_fit_joint with the host build in the device call's place: 3 participants x 40 trials, 4 chains, 300 + 500 iterations."""
    from bayesflow_nddms_amd import alpha_not_scaled, mcmc
    run = _host_run(host)

    def call(model, d, ext, state, sigma, want_draws=True, want_log_post=True, **kw):
        return run(d, ext, state, sigma, **kw)
    data, ext = fit_data()
    fit = mcmc.hmc_fit_joint(data, ext, chains=4, warmup=300, samples=500, thin=5, seed=8, _call=call)
    check_fit(fit, 3)
    y = data[..., 0] * data[..., 1]
    held = alpha_not_scaled.fit_hmc(y, ext, chains=2, warmup=40, samples=20, thin=5, seed=8, fixed={"sigma": 0.5, "dc": 1.0}, _call=call)
    assert np.all(held["sigma"] == 0.5) and np.all(held["varsigma"] == 1.0) and np.ptp(held["alpha"]) > 0 and np.all(np.isnan(held["sigma_accept"]))
    gen = dict(y=y.reshape(-1), extdata=ext, nparts=3, ntrials=40)
    again = alpha_not_scaled.fit_hmc(gen, chains=2, warmup=40, samples=20, thin=5, seed=8, fixed={"sigma": 0.5, "dc": 1.0}, _call=call)
    assert all(np.array_equal(again[k], held[k], equal_nan=True) for k in held)
