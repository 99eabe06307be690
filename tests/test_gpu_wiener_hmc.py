"""GPU tests of the batched HMC sampler (engine.wiener_hmc -> nddm_wiener_hmc -> wiener_hmc_kernel; csrc/nddm_wiener_hmc.h): the device
against the host build of the same header, the bits tests (cut = uncut, chain independence, the flagged neighbour), the energy bars and
both statistics tests of tests/test_wiener_hmc_host.py with 256 chains, the flags, and mcmc.hmc_fit end to end."""
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import pytest

import wiener_hmc_ref as R
from conftest import ROOT
from test_wiener_hmc_host import SAME, check_statistics

sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu
HAVE_CXX = not (shutil.which("g++") is None and shutil.which("c++") is None and shutil.which("clang++") is None)


@pytest.fixture(scope="module")
def host():
    import wiener_hmc_host as H
    with tempfile.TemporaryDirectory() as td:
        yield H, td, H.build(td) if HAVE_CXX else None


def _profile():
    import wiener_hmc_host as H
    with open(H.PROFILE) as f:
        return json.load(f)


def dev_run(data, state, chains_per_dataset=1, **kw):
    """engine.wiener_hmc with numpy in and out (the host tool's run())."""
    from bayesflow_nddms_amd import engine
    import torch
    d = torch.as_tensor(np.asarray(data, np.float32)).cuda()              # (device data: the kernel, not the adapter, meets a bad data set)
    r = engine.wiener_hmc(engine.BASIC_DDM_DC, d, np.asarray(state, np.float64), chains_per_dataset=chains_per_dataset, **kw)
    return {k: v.cpu().numpy() for k, v in r.items()}


@pytest.mark.parametrize("N,S,C", [(1, 64, 256), (20, 64, 256), (64, 64, 256), (65, 64, 256), (130, 64, 256), (65, 1, 4), (20, 3, 12), (65, 3, 9)],
                         ids=lambda v: str(v))
def test_device_equals_the_host_build_within_the_recorded_tolerance(host, N, S, C):
    """3 iterations of 4 leapfrog steps from the same state.  N: one lane, a partial first round, a full round, a second round of one lane,
    a third round; chains_per_dataset 1, 3, 64; C = 9 is no multiple of the workgroup's 4 chains.  Tolerance: 4 x what the host's float32
    build shows against the float64 build of the same arithmetic (profiles/r17_wiener_hmc_host.json); a chain whose accept decision
    flipped is left out, at most 2 % of them (at C < 50: none)."""
    H, td, exe = host
    if exe is None:
        pytest.skip("no host C++ compiler")
    P = _profile()
    data, theta = H.case(N, C=C, D=C // S)
    st = H.init_state(theta, data, S, eps0=0.02)
    a, b = dev_run(data, st, S, **H.COMPARE), H.run(exe, td, data, st, S, **H.COMPARE)
    same, dl, dd = H.compare(a, b, theta)
    print("N", N, "S", S, "C", C, "left out", int((~same).sum()), "log_post", dl, "draws", dd)
    assert not a["flagged"].any() and np.all(np.isfinite(a["draws"]))
    assert (~same).mean() <= 0.02 and dl <= P["device_tolerance_log_post_rel"] and dd <= P["device_tolerance_draw_abs"]
    assert np.array_equal(a["divergent"][same], b["divergent"][same])


def _bits_case():
    import wiener_hmc_host as H
    data, theta = H.case(65, C=32, D=4, seed=17)
    return data, theta, H.init_state(theta, data, 8)


def test_cut_runs_give_the_bits_of_the_uncut_run():
    """40 iterations, 25 of them adapting, thin 3: one launch, two (cut inside the adaptation) and five (one cut on the border)."""
    data, theta, st = _bits_case()
    kw = dict(n_adapt=25, n_leapfrog=5, thin=3, seed=21)
    whole = dev_run(data, st, 8, n_iter=40, **kw)
    assert whole["draws"].shape == (32, 13, 5) and np.all(whole["state"][:, 9] == 25) and np.all(np.isfinite(whole["draws"]))
    for cuts in ((17, 23), (7, 8, 10, 4, 11)):
        parts, s, off = [], st, 0
        for n in cuts:
            r = dev_run(data, s, 8, n_iter=n, iter_offset=off, **kw)
            parts.append(r)
            s, off = r["state"], off + n
        assert np.array_equal(np.concatenate([p["draws"] for p in parts], 1), whole["draws"])
        assert np.array_equal(np.concatenate([p["log_post"] for p in parts], 1), whole["log_post"])
        assert np.array_equal(s, whole["state"]) and np.array_equal(sum(p["divergent"] for p in parts), whole["divergent"])


def test_chains_do_not_depend_on_their_neighbours_and_bad_input_is_flagged():
    """32 chains in one launch equal 2 x 16 with chain_offset.  A timeout, a NaN, an rt <= 0 in one data set and a non-finite state each give
    flagged = 1, NaN draws and an unchanged state -- found by reading the values -- and change no bit of the other chains."""
    data, theta, st = _bits_case()
    kw = dict(n_iter=12, n_adapt=6, n_leapfrog=5, thin=2, seed=22)
    whole = dev_run(data, st, 8, chain_offset=100, **kw)
    halves = [dev_run(data[2 * h:2 * h + 2], st[16 * h:16 * h + 16], 8, chain_offset=100 + 16 * h, **kw) for h in range(2)]
    for k in SAME + ("accept",):
        assert np.array_equal(np.concatenate([h[k] for h in halves]), whole[k], equal_nan=True), k
    bad = np.arange(32) // 8 == 1
    for mutate in (lambda x: x.__setitem__((1, 3, 1), 0.0), lambda x: x.__setitem__((1, 64, 0), np.nan), lambda x: x.__setitem__((1, 0, 0), 0.0),
                   lambda x: x.__setitem__((1, 7, 0), np.inf)):
        x = data.copy()
        mutate(x)
        r = dev_run(x, st, 8, chain_offset=100, **kw)
        assert np.array_equal(r["flagged"], bad.astype(np.int32))
        assert np.all(np.isnan(r["draws"][bad])) and np.all(np.isnan(r["log_post"][bad])) and np.array_equal(r["state"][bad], st[bad])
        for k in SAME:
            assert np.array_equal(r[k][~bad], whole[k][~bad]), k
    # a non-finite state reaches the kernel only in a device tensor (the adapter refuses a host one)
    import torch
    from bayesflow_nddms_amd import engine
    s2 = st.copy()
    s2[5, 1] = np.nan
    sd = torch.as_tensor(s2).cuda()
    r = engine.wiener_hmc(engine.BASIC_DDM_DC, torch.as_tensor(data).cuda(), sd, chains_per_dataset=8, chain_offset=100, **kw)
    assert r["state"] is sd                                             # a device state is updated in place
    r = {k: v.cpu().numpy() for k, v in r.items()}
    assert r["flagged"].sum() == 1 and r["flagged"][5] == 1 and np.all(np.isnan(r["draws"][5]))
    assert np.array_equal(r["state"][5], s2[5], equal_nan=True) and np.array_equal(np.delete(r["draws"], 5, 0), np.delete(whole["draws"], 5, 0))


@pytest.mark.parametrize("N", [1, 20, 64, 65, 130])
def test_energy_error_of_short_trajectories_stays_under_the_recorded_bar(N):
    """eps = 1e-3, 8 leapfrog steps, no adaptation, 256 chains, 4 iterations: the host test's bar (4 x the host build's largest)."""
    import wiener_hmc_host as H
    data, theta = H.case(N)
    r = dev_run(data, H.init_state(theta, data, 64, eps0=1e-3), 64, **H.ENERGY)
    worst = float(np.max(r["state"][:, 11]))
    print("N", N, "largest |H1 - H0|", worst)
    assert not r["flagged"].any() and not r["divergent"].any() and np.all(np.isfinite(r["state"][:, 10:]))
    assert worst <= _profile()["energy_bar"][str(N)]


def _fit(y, mask, fixed, C=256, n_sample=1875, seed=3):
    """C chains on one data set from the reference's initial values: 300 adapting iterations, then n_sample at thin 5, unit mass."""
    from bayesflow_nddms_amd import mcmc
    data = R.as_data(y)[None]
    th = mcmc.hmc_init(data, C, seed).reshape(-1, 5)
    for k, v in fixed.items():
        th[:, mcmc.PARAM_NAMES.index(k)] = v
    st = mcmc.make_state(th, np.repeat(data, C, 0), free=mask)
    kw = dict(n_adapt=300, n_leapfrog=16, thin=5, free_mask=mask, seed=seed)
    r = dev_run(data, st, C, n_iter=300, want_draws=False, want_log_post=False, **kw)
    return dev_run(data, r["state"], C, n_iter=n_sample, iter_offset=300, **kw), th


def test_two_free_columns_match_the_grid_quadrature():
    """256 chains x (300 adapting + 375 kept at thin 5) = the host test's 96 000 pooled draws, the same bars."""
    m, sd = R.recorded()["two"]                                       # (tests/test_wiener_hmc_host.py recomputes the recorded yardsticks)
    r, th0 = _fit(R.Y20, 3, R.FIXED_2D)
    assert r["draws"].shape == (256, 375, 5) and not r["flagged"].any()
    assert np.array_equal(r["draws"][:, :, 2:], np.broadcast_to(th0[:, None, 2:].astype(np.float32), (256, 375, 3)))
    check_statistics(r["draws"], [0, 1], m, sd)


def test_five_free_columns_match_importance_sampling_from_the_prior():
    m, sd = R.recorded()["five"]
    assert R.recorded()["five_ess"] >= 20_000
    r, _ = _fit(R.Y10, 31, {})
    assert not r["flagged"].any()
    check_statistics(r["draws"], [0, 1, 2, 3, 4], m, sd)


def test_hmc_fit_end_to_end():
    """8 participants x 40 trials, 4 chains, 300 + 500 iterations: the reference's JAGS layout, Rhat < 1.05 on every variable, and the
    acceptance rate after adaptation inside the sanity band [0.6, 0.95] around the 0.8 target (the host build gives 0.92 - 0.94)."""
    import wiener_hmc_host as H
    from bayesflow_nddms_amd import basic_ddm_dc, diagnostics as Dg
    data = H.example_data(8, 40, 31)
    fit = basic_ddm_dc.fit_hmc(data, chains=4, warmup=300, samples=500, thin=5, seed=8)
    for k in ("alpha", "ndt", "beta", "delta", "varsigma", "log_post"):
        assert fit[k].shape == (8, 100, 4) and fit[k].dtype == np.float64 and np.all(np.isfinite(fit[k]))
    assert fit["accept_rate"].shape == fit["n_divergent"].shape == fit["flagged"].shape == (8, 4) and not fit["flagged"].any()
    dg = Dg.rhat_neff({k: fit[k] for k in ("alpha", "ndt", "beta", "delta", "varsigma")})
    print({k: v["rhat"].max() for k, v in dg.items()}, fit["accept_rate"].min(), fit["accept_rate"].max())
    assert all(np.all(v["rhat"] < 1.05) for v in dg.values())
    assert np.all((fit["accept_rate"] >= 0.6) & (fit["accept_rate"] <= 0.95))
