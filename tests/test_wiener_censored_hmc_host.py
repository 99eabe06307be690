"""CPU tests of NDDM_WIENER_CENSORED in the two HMC samplers (csrc/nddm_wiener_hmc.h, nddm_wiener_hmc_joint.h), on their host builds
(tools/wiener_hmc_host.py, tools/wiener_hmc_joint_host.py with censored=True): with timeouts in the data the gradient is the potential's
(the energy error quarters when the step halves, all five columns free), cut runs equal the uncut run, the flag changes no bit where no
trial is a timeout, a data set of timeouts alone samples with T = 1.5, bad data are still flagged; the same for the joint sampler; the
host side (mcmc) takes its support and initial values from the responses and hands `censored` to every engine call and to none by
default; and the recorded statistics yardsticks are the float64 grid's."""
import os
import shutil
import sys
import tempfile

import numpy as np
import pytest

import wiener_censored_ref as R
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

HAVE_CXX = not (shutil.which("g++") is None and shutil.which("c++") is None and shutil.which("clang++") is None)
needs_cxx = pytest.mark.skipif(not HAVE_CXX, reason="no host C++ compiler")
SAME = ("draws", "log_post", "divergent", "flagged", "state", "accept")


@pytest.fixture(scope="module")
def host():
    """(tools/wiener_hmc_host.py, a scratch directory, build(name): the programs, each compiled on first use)"""
    import wiener_hmc_host as H
    with tempfile.TemporaryDirectory() as td:
        made = {}

        def build(name):
            if name not in made:
                made[name] = H.build(td, f64="64" in name, censored="c" in name)
            return made[name]
        yield H, td, build


@pytest.fixture(scope="module")
def joint():
    import wiener_hmc_joint_host as J
    with tempfile.TemporaryDirectory() as td:
        made = {}

        def build(name):
            if name not in made:
                made[name] = J.build(td, f64="64" in name, censored="c" in name)
            return made[name]
        yield J, td, build


def _equal(a, b, keys=SAME):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


@needs_cxx
@pytest.mark.parametrize("N", [20, 130])
def test_energy_error_falls_with_the_square_of_the_step_with_timeouts(host, N):
    """All five columns free, about 10 % of each data set's trials timeouts, the float64 build of the likelihood's arithmetic, a fixed
    trajectory length: the median ratio of the energy errors at eps, eps / 2 lies in 3.9 .. 4.1.  tau moves, so t = rt - tau of every
    timeout moves: a wrong d/dtau of log S, or a support that still counted the timeouts' rt, leaves a first-order part."""
    H, td, build = host
    data, theta = H.case(N)
    dc = H.censor(data)
    assert np.all((dc[..., 1] == 0).sum(1) == max(1, round(0.1 * N)))
    err = []
    for eps in (4e-3, 2e-3, 1e-3):
        r = H.run(build("64c"), td, dc, H.init_state(theta, dc, 64, eps0=eps, censored=True), 64, n_iter=1, n_leapfrog=int(round(8e-3 / eps)), seed=11)
        assert not r["flagged"].any()
        err.append(np.abs(r["state"][:, 10]))
    ratios = [float(np.median(err[i] / err[i + 1])) for i in range(2)]
    print("N", N, "median ratios", ratios)
    assert all(3.9 < x < 4.1 for x in ratios)


@needs_cxx
def test_cut_runs_give_the_bits_of_the_uncut_run_with_timeouts(host):
    """40 iterations, 25 of them adapting, thin 3: one call, two calls (cut inside the adaptation) and five (one cut on the border)."""
    H, td, build = host
    data, theta = H.case(65, C=32, D=4, seed=17)
    dc = H.censor(data)
    st = H.init_state(theta, dc, 8, censored=True)
    kw = dict(n_adapt=25, n_leapfrog=5, thin=3, seed=21)
    whole = H.run(build("32c"), td, dc, st, 8, n_iter=40, **kw)
    assert not whole["flagged"].any() and np.all(np.isfinite(whole["draws"])) and np.all(whole["state"][:, 9] == 25)
    for cuts in ((17, 23), (7, 8, 10, 4, 11)):
        parts, s, off = [], st, 0
        for n in cuts:
            r = H.run(build("32c"), td, dc, s, 8, n_iter=n, iter_offset=off, **kw)
            parts.append(r)
            s, off = r["state"], off + n
        assert np.array_equal(np.concatenate([p["draws"] for p in parts], 1), whole["draws"])
        assert np.array_equal(np.concatenate([p["log_post"] for p in parts], 1), whole["log_post"])
        assert np.array_equal(s, whole["state"]) and np.array_equal(sum(p["divergent"] for p in parts), whole["divergent"])


@needs_cxx
@pytest.mark.parametrize("N", [1, 20, 65, 130])
def test_the_flag_changes_no_bit_where_no_trial_is_a_timeout(host, N):
    H, td, build = host
    data, theta = H.case(N, C=16, D=4)
    st = H.init_state(theta, data, 4)
    assert np.array_equal(st, H.init_state(theta, data, 4, censored=True))
    kw = dict(n_iter=12, n_adapt=6, n_leapfrog=5, thin=2, seed=22)
    assert _equal(H.run(build("32"), td, data, st, 4, **kw), H.run(build("32c"), td, data, st, 4, **kw))


@needs_cxx
def test_timeouts_alone_sample_with_the_full_tau_range_and_bad_data_are_flagged(host):
    H, td, build = host
    from bayesflow_nddms_amd import mcmc
    data, theta = H.case(20, C=12, D=3, seed=17)
    dc = H.censor(data)
    dc[1, :, 0], dc[1, :, 1] = 1.3, 0.0                                  # a data set of timeouts alone
    theta[4:8, 3] = np.linspace(0.1, 1.45, 4)                            # tau up to 1.45 < T = 1.5, beyond every rt of the set
    lo, wd = mcmc._support(dc, censored=True)
    assert wd[1, 3] == 1.5 and np.all(wd[[0, 2], 3] == np.where(dc[[0, 2], :, 1] == 0, np.inf, dc[[0, 2], :, 0]).min(1).astype(np.float64))
    st = H.init_state(theta, dc, 4, censored=True)
    kw = dict(n_iter=12, n_adapt=6, n_leapfrog=5, thin=2, seed=22)
    whole = H.run(build("32c"), td, dc, st, 4, **kw)
    assert not whole["flagged"].any() and np.all(np.isfinite(whole["draws"])) and np.all(np.isfinite(whole["log_post"]))
    assert np.any(whole["draws"][4:8, :, 3] > 1.3) and np.all(whole["draws"][4:8, :, 3] < 1.5)
    # the unflagged chain refuses the same data; the flagged one still refuses what no chain can sample
    assert H.run(build("32"), td, dc, st, 4, **kw)["flagged"].all()
    for mutate in (lambda x: x.__setitem__((1, 3, 0), np.nan), lambda x: x.__setitem__((1, 5, 0), 0.0), lambda x: x.__setitem__((1, 0, 1), 2.0),
                   lambda x: x.__setitem__((1, 7, 1), np.nan), lambda x: x.__setitem__((1, 2, 0), np.inf)):
        x = dc.copy()
        mutate(x)
        r = H.run(build("32c"), td, x, st, 4, **kw)
        bad = np.arange(12) // 4 == 1
        assert np.array_equal(r["flagged"], bad.astype(np.int32))
        assert np.all(np.isnan(r["draws"][bad])) and np.all(np.isnan(r["log_post"][bad])) and np.array_equal(r["state"][bad], st[bad])
        for k in SAME:
            assert np.array_equal(r[k][~bad], whole[k][~bad], equal_nan=True), k


@needs_cxx
@pytest.mark.parametrize("S", [1, 3])
def test_the_joint_sampler_passes_the_flag_to_its_chains(joint, S):
    """P = 3 participants: no bit changes without timeouts; with them the chains run (the unflagged build flags every chain), the energy
    error quarters when the step halves (sigma held), and a data set no chain can sample still flags every chain."""
    J, td, build = joint
    import wiener_hmc_host as H
    P = 3
    data, ext, theta = J.case(20, P, S)
    sg = np.full(S, J.COMPARE_SIGMA)
    st = H.init_state(theta, data, S, eps0=0.02)
    kw = dict(n_iter=6, n_adapt=3, n_leapfrog=4, seed=13)
    keys = SAME + ("sigma_draws", "sigma_accept", "sigma")
    assert _equal(J.run(build("32"), td, data, ext, st, sg, **kw), J.run(build("32c"), td, data, ext, st, sg, **kw), keys)
    fx = J.run(build("32"), td, data, ext, st, sg, sigma_fixed=True, **kw)
    assert _equal(fx, J.run(build("32c"), td, data, ext, st, sg, sigma_fixed=True, **kw), keys)
    dc = H.censor(data)
    stc = H.init_state(theta, dc, S, eps0=0.02, censored=True)
    r = J.run(build("32c"), td, dc, ext, stc, sg, **kw)
    assert not r["flagged"].any() and np.all(np.isfinite(r["draws"])) and np.all(np.isfinite(r["sigma_draws"]))
    assert J.run(build("32"), td, dc, ext, stc, sg, **kw)["flagged"].all()
    err = []
    for eps in (4e-3, 2e-3, 1e-3):
        e = J.run(build("64c"), td, dc, ext, H.init_state(theta, dc, S, eps0=eps, censored=True), np.full(S, J.ENERGY_SIGMA), n_iter=1,
                  n_leapfrog=int(round(8e-3 / eps)), seed=11, sigma_fixed=True)
        err.append(np.abs(e["state"][:, 10]))
    ratios = [float(np.median(err[i] / err[i + 1])) for i in range(2)]
    print("S", S, "median ratios", ratios)
    assert all(3.9 < x < 4.1 for x in ratios)
    x = dc.copy()
    x[2, 4, 1] = 2.0
    bad = J.run(build("32c"), td, x, ext, stc, sg, **kw)
    assert bad["flagged"].all() and np.all(np.isnan(bad["draws"])) and np.array_equal(bad["state"], stc)


def test_the_host_side_takes_its_support_and_initial_values_from_the_responses():
    from bayesflow_nddms_amd import mcmc
    d = np.array([[[0.6, 1.0], [0.3, 0.0], [0.9, -1.0]], [[2.0, 0.0], [1.8, 0.0], [1.9, 0.0]]], np.float32)
    lo, wd = mcmc._support(d, censored=True)
    assert wd[0, 3] == np.float64(np.float32(0.6)) and wd[1, 3] == 1.5
    assert mcmc._support(d)[1][0, 3] == np.float64(np.float32(0.3))      # (the default counts every rt: what it did)
    th = np.array([[0.5, 1.2, 0.5, 0.45, 1.0], [0.5, 1.2, 0.5, 1.2, 1.0]])
    q = mcmc.theta_to_q(th, d, censored=True)
    assert np.allclose(mcmc.q_to_theta(q, d, censored=True), th, rtol=0, atol=1e-14)
    assert np.array_equal(mcmc.make_state(th, d, censored=True)[:, :5], q)
    with pytest.raises(ValueError, match="support"):
        mcmc.theta_to_q(th, d)                                           # tau .45 is beyond the timeout's rt .3
    a, b = mcmc.hmc_init(d, 50, 3, censored=True), mcmc.hmc_init(d, 50, 3)
    assert np.array_equal(a[..., [0, 1, 2, 4]], b[..., [0, 1, 2, 4]])
    assert a[0, :, 3].max() > 0.15 and a[0, :, 3].max() < 0.3 and b[0, :, 3].max() < 0.15 and 0.6 < a[1, :, 3].max() < 0.75
    assert np.array_equal(mcmc.hmc_init_joint(d, 4, 3, censored=True)[0], mcmc.hmc_init(d, 4, 3, censored=True))
    with pytest.raises(ValueError, match="> 0"):
        mcmc._support(np.array([[[0.6, 1.0], [-0.3, 0.0]]], np.float32), censored=True)


@pytest.mark.parametrize("is_joint", [False, True], ids=["hmc_fit", "hmc_fit_joint"])
def test_censored_adds_that_one_keyword_to_every_engine_call_and_nothing_else(is_joint):
    """tests/test_hmc_fit_schedule.py's recording fake in the engine call's place: the same launches in the same order with the same
    keywords, plus censored=True in every one of them; by default no call holds the keyword."""
    import test_hmc_fit_schedule as T
    from bayesflow_nddms_amd import mcmc
    d = T._data()

    def fit(**more):
        fake = T.Fake(is_joint)
        kw = dict(chains=T.CHAINS, warmup=T.WARMUP, samples=T.SAMPLES, thin=T.THIN, n_leapfrog=T.LEAPFROG, seed=T.SEED, _call=fake, **more)
        out = mcmc.hmc_fit_joint(d, np.array([1.0, 1.5]), **kw) if is_joint else mcmc.hmc_fit(d, **kw)
        return fake, out
    plain, out0 = fit()
    flagged, out1 = fit(censored=True)
    assert len(plain.calls) == len(flagged.calls) and [c["key"] for c in plain.calls] == [c["key"] for c in flagged.calls]
    for a, b in zip(plain.calls, flagged.calls):
        assert "censored" not in a["kw"] and b["kw"]["censored"] is True
        assert {k: v for k, v in b["kw"].items() if k != "censored"} == a["kw"]
        assert np.array_equal(a["state"], b["state"])                    # (no timeout in these data: the same support, the same start)
        assert (a["inv_mass"] is None) == (b["inv_mass"] is None) and (a["inv_mass"] is None or np.array_equal(a["inv_mass"], b["inv_mass"]))
    assert all(np.array_equal(out0[k], out1[k]) for k in out0)
    # with timeouts the first state is hmc_init's from the responses, in the responses' support
    dt = d.copy()
    dt[:, ::7, 1] = 0.0
    dt[:, ::7, 0] = 0.05
    fake = T.Fake(is_joint)
    kw = dict(chains=T.CHAINS, warmup=T.WARMUP, samples=T.SAMPLES, thin=T.THIN, n_leapfrog=T.LEAPFROG, seed=T.SEED, _call=fake, censored=True)
    mcmc.hmc_fit_joint(dt, np.array([1.0, 1.5]), **kw) if is_joint else mcmc.hmc_fit(dt, **kw)
    theta = mcmc.hmc_init(dt, T.CHAINS, T.SEED, censored=True).reshape(-1, 5)
    assert np.array_equal(fake.calls[0]["state"][:, :5], mcmc.theta_to_q(theta, np.repeat(dt, T.CHAINS, 0), censored=True))
    assert theta[:, 3].max() > 0.05


def test_engine_adapters_take_censored_and_check_host_data():
    import inspect
    from bayesflow_nddms_amd import basic_ddm_dc, engine, mcmc
    for fn in (engine.wiener_hmc, engine.wiener_hmc_joint, mcmc.hmc_fit, mcmc.hmc_fit_joint, mcmc.hmc_init, mcmc.hmc_init_joint, mcmc.make_state,
               mcmc.theta_to_q, mcmc.q_to_theta, mcmc._support):
        assert inspect.signature(fn).parameters["censored"].default is False, fn.__name__
    d = np.array([[[0.6, 1.0], [1.3, 0.0]]])
    st = np.zeros((1, 12))
    with pytest.raises(ValueError, match="no gradient here"):
        engine.wiener_hmc(engine.BASIC_DDM_DC, d, st)
    with pytest.raises(ValueError, match=r"\{1, -1, 0\}"):
        engine.wiener_hmc(engine.BASIC_DDM_DC, np.array([[[0.6, 2.0]]]), st, censored=True)
    with pytest.raises(ValueError, match="> 0"):
        engine.wiener_hmc(engine.BASIC_DDM_DC, np.array([[[0.6, 1.0], [0.0, 0.0]]]), st, censored=True)
    assert "censored" in basic_ddm_dc.fit_hmc.__doc__


def test_c_abi_takes_the_flag_in_both_samplers():
    """flags = 4 passes nddm_wiener_hmc's flags check and 4, 5 nddm_wiener_hmc_joint's (the next check, the shape, answers); 1 and 2, 3 keep
    their refusals and their words.  No case reaches a HIP call."""
    import ctypes
    from bayesflow_nddms_amd import _lib
    L = _lib.lib()
    d = ctypes.c_void_p(16)
    hmc = lambda flags, n_iter=0: L.nddm_wiener_hmc(0, d, 1, 10, 1, 1, d, None, n_iter, 0, 4, 1, 31, 0, 0, 0, flags, d, d, d, d, d, None)
    for fl in (1, 2, 3, 5, 8):
        assert hmc(fl) == _lib.NDDM_ERR_PARAM and L.nddm_last_error().decode() == "nddm_wiener_hmc: flags must be 0 (reserved) and free_mask < 32"
    for fl in (0, 4):
        assert hmc(fl) == _lib.NDDM_ERR_SHAPE and L.nddm_last_error().decode().startswith("C >= 0 chains")
    jnt = lambda flags: L.nddm_wiener_hmc_joint(0, d, 2, 10, 2, 1, d, d, None, d, d, 0, 0, 4, 1, 31, 0, 0, 0, flags, d, d, d, d, d, d, d, None)
    for fl in (2, 3, 6, 7, 8):
        assert jnt(fl) == _lib.NDDM_ERR_PARAM
        assert L.nddm_last_error().decode() == "nddm_wiener_hmc_joint: flags must be 0 or NDDM_HMC_SIGMA_FIXED and free_mask < 32"
    for fl in (0, 1, 4, 5):
        assert jnt(fl) == _lib.NDDM_ERR_SHAPE and L.nddm_last_error().decode().startswith("C >= 0 chains")


def test_recorded_statistics_yardsticks_are_the_float64_grids():
    """Y20 + four timeouts at rt = 1.5 (drift, boundary free): the grid quadrature recomputed equals the recorded moments; the last
    refinement moved them by less than 1e-4 sd; and the posterior WITHOUT the timeouts lies more than 0.5 sd away in both columns, so a
    sampler that ignored them cannot pass.  (The five-column importance sampler takes over a minute: `python tests/wiener_censored_ref.py`
    recomputes and records it, and asserts its effective size >= 20 000.)"""
    rec = R.recorded()
    m, sd, n, move = R.yardstick_2d()
    assert move < 1e-4 and n == rec["two_grid"]
    assert np.allclose(m, rec["two"][0], rtol=0, atol=1e-9) and np.allclose(sd, rec["two"][1], rtol=0, atol=1e-9)
    assert np.allclose(m, [0.6464, 1.6108], atol=5e-5) and np.allclose(sd, [0.288, 0.127], atol=5e-4)
    m0, sd0 = rec["two_without"]
    import wiener_hmc_ref as HR
    assert np.allclose(m0, HR.recorded()["two"][0], rtol=0, atol=1e-9)
    assert np.all(np.abs(m - m0) / sd > 0.5)
    assert rec["five_ess"] >= 20_000 and R.TIMEOUTS_5D == (1.2, 1.2) and R.TIMEOUTS_2D == (1.5,) * 4
