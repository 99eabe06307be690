"""GPU tests of NDDM_WIENER_CENSORED in the two HMC samplers (engine.wiener_hmc / wiener_hmc_joint(..., censored=True) -> flag 4 of
nddm_wiener_hmc / nddm_wiener_hmc_joint -> wiener_hmc_censored_kernel / wiener_hmc_censored_joint_kernel): the flag changes no bit where no
trial is a timeout, the device chain equals the host build's on data with 10 % timeouts, the statistics tests with timeouts against the
float64 yardsticks (tests/wiener_censored_ref.py) -- which a sampler that dropped the timeouts cannot pass --, hmc_fit end to end on
simulated data, and the shipped code object's resources."""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import wiener_censored_ref as R
from conftest import ROOT
from test_wiener_hmc_host import check_statistics

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tools"))

HAVE_CXX = not (shutil.which("g++") is None and shutil.which("c++") is None and shutil.which("clang++") is None)
SAME = ("draws", "log_post", "divergent", "flagged", "state", "accept")


def dev_run(data, state, chains_per_dataset=1, **kw):
    """engine.wiener_hmc with numpy in and out (the host tool's run())."""
    from bayesflow_nddms_amd import engine
    import torch
    d = torch.as_tensor(np.asarray(data, np.float32)).cuda()              # (device data: the kernel, not the adapter, meets a bad data set)
    r = engine.wiener_hmc(engine.BASIC_DDM_DC, d, np.asarray(state, np.float64), chains_per_dataset=chains_per_dataset, **kw)
    return {k: v.cpu().numpy() for k, v in r.items()}


def dev_run_joint(data, ext, state, sigma, **kw):
    from bayesflow_nddms_amd import engine
    import torch
    d = torch.as_tensor(np.asarray(data, np.float32)).cuda()
    r = engine.wiener_hmc_joint(engine.BASIC_DDM_DC, d, np.asarray(ext, np.float64), np.asarray(state, np.float64), np.asarray(sigma, np.float64), **kw)
    return {k: v.cpu().numpy() for k, v in r.items()}


@pytest.mark.parametrize("N", [1, 20, 65, 130])
def test_the_flag_changes_no_bit_where_no_trial_is_a_timeout(N):
    """Draws, log_post, state, divergent, flagged and accept of the flagged entry equal the unflagged entry's."""
    import wiener_hmc_host as H
    data, theta = H.case(N, C=36, D=4)
    st = H.init_state(theta, data, 9)
    kw = dict(n_iter=12, n_adapt=6, n_leapfrog=5, thin=2, seed=22)
    a, b = dev_run(data, st, 9, **kw), dev_run(data, st, 9, censored=True, **kw)
    assert not a["flagged"].any() and np.all(np.isfinite(a["draws"]))
    for k in SAME:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("S", [1, 3])
def test_the_joint_sampler_takes_the_flag_next_to_sigma_fixed(S):
    """P = 3: flags 4 against 0 and 5 against 1 on data without timeouts are bit-equal; with timeouts the flagged entry samples and the
    unflagged one flags every chain."""
    import wiener_hmc_host as H
    import wiener_hmc_joint_host as J
    data, ext, theta = J.case(20, 3, S)
    sg = np.full(S, J.COMPARE_SIGMA)
    st = H.init_state(theta, data, S, eps0=0.02)
    kw = dict(n_iter=6, n_adapt=3, n_leapfrog=4, seed=13)
    keys = SAME + ("sigma_draws", "sigma_accept", "sigma")
    for fixed in (False, True):
        a, b = dev_run_joint(data, ext, st, sg, sigma_fixed=fixed, **kw), dev_run_joint(data, ext, st, sg, sigma_fixed=fixed, censored=True, **kw)
        assert not a["flagged"].any()
        for k in keys:
            assert np.array_equal(a[k], b[k], equal_nan=True), (fixed, k)
    dc = H.censor(data)
    stc = H.init_state(theta, dc, S, eps0=0.02, censored=True)
    r = dev_run_joint(dc, ext, stc, sg, censored=True, **kw)
    assert not r["flagged"].any() and np.all(np.isfinite(r["draws"])) and np.all(np.isfinite(r["sigma_draws"]))
    assert not np.array_equal(r["state"], stc)
    r0 = dev_run_joint(dc, ext, stc, sg, **kw)
    assert r0["flagged"].all() and np.all(np.isnan(r0["draws"])) and np.array_equal(r0["state"], stc)


@pytest.fixture(scope="module")
def host():
    import wiener_hmc_host as H
    with tempfile.TemporaryDirectory() as td:
        yield H, td, H.build(td, censored=True) if HAVE_CXX else None


@pytest.mark.parametrize("N", [1, 20, 64, 65, 130])
def test_device_equals_the_host_build_with_timeouts(host, N):
    """3 iterations of 4 leapfrog steps from the same state, 256 chains on 4 data sets with about 10 % timeouts.  Tolerance: 4 x what the
    host's float32 build shows against its float64 build FOR THE SAME CASE (profiles/r22_wiener_censored_hmc_host.json), on log_post
    (relative) and the final q (float64, absolute); no accept decision flips."""
    H, td, exe = host
    if exe is None:
        pytest.skip("no host C++ compiler")
    with open(H.CENSORED_PROFILE) as f:
        tol = json.load(f)["device_tolerance"][f"N{N}"]
    data, theta = H.censored_case(N)
    assert np.all((data[..., 1] == 0).sum(1) == max(1, round(0.1 * N)))
    st = H.init_state(theta, data, 64, eps0=0.02, censored=True)
    a, b = dev_run(data, st, 64, censored=True, **H.COMPARE), H.run(exe, td, data, st, 64, **H.COMPARE)
    same, dl, dq = H.compare_q(a, b, theta)
    print("N", N, "flipped", int((~same).sum()), "log_post", dl, tol["log_post_rel"], "q", dq, tol["q_abs"])
    assert not a["flagged"].any() and np.all(np.isfinite(a["draws"]))
    assert same.all()
    assert dl <= tol["log_post_rel"] and dq <= tol["q_abs"]
    assert np.array_equal(a["divergent"], b["divergent"])


def test_bad_data_are_still_flagged_and_neighbours_keep_their_bits():
    import wiener_hmc_host as H
    data, theta = H.case(65, C=32, D=4, seed=17)
    dc = H.censor(data)
    dc[2, :, 0], dc[2, :, 1] = 1.3, 0.0                                  # a data set of timeouts alone: T = 1.5
    st = H.init_state(theta, dc, 8, censored=True)
    kw = dict(n_iter=12, n_adapt=6, n_leapfrog=5, thin=2, seed=22, censored=True)
    whole = dev_run(dc, st, 8, **kw)
    assert not whole["flagged"].any() and np.all(np.isfinite(whole["draws"])) and np.all(whole["draws"][:, :, 3] < 1.5)
    for mutate in (lambda x: x.__setitem__((1, 3, 0), np.nan), lambda x: x.__setitem__((1, 64, 0), 0.0), lambda x: x.__setitem__((1, 0, 1), 2.0),
                   lambda x: x.__setitem__((1, 7, 1), np.nan)):
        x = dc.copy()
        mutate(x)
        r = dev_run(x, st, 8, **kw)
        bad = np.arange(32) // 8 == 1
        assert np.array_equal(r["flagged"], bad.astype(np.int32))
        assert np.all(np.isnan(r["draws"][bad])) and np.all(np.isnan(r["log_post"][bad])) and np.array_equal(r["state"][bad], st[bad])
        for k in SAME:
            assert np.array_equal(r[k][~bad], whole[k][~bad], equal_nan=True), k
    assert dev_run(dc, st, 8, **dict(kw, censored=False))["flagged"].all()


def _fit(data, mask, fixed, C=256, n_sample=1875, seed=3):
    """C chains on one data set from the reference's initial values: 300 adapting iterations, then n_sample at thin 5, unit mass."""
    from bayesflow_nddms_amd import mcmc
    data = data[None]
    th = mcmc.hmc_init(data, C, seed, censored=True).reshape(-1, 5)
    for k, v in fixed.items():
        th[:, mcmc.PARAM_NAMES.index(k)] = v
    st = mcmc.make_state(th, np.repeat(data, C, 0), free=mask, censored=True)
    kw = dict(n_adapt=300, n_leapfrog=16, thin=5, free_mask=mask, seed=seed, censored=True)
    r = dev_run(data, st, C, n_iter=300, want_draws=False, want_log_post=False, **kw)
    return dev_run(data, r["state"], C, n_iter=n_sample, iter_offset=300, **kw), th


def test_two_free_columns_with_four_timeouts_match_the_grid_quadrature():
    """Y20 + four timeouts at rt = 1.5, drift and boundary free: 256 chains x (300 adapting + 375 kept at thin 5), section 17's bars.  The
    posterior without the timeouts lies 0.84 sd (drift) and 1.8 sd (boundary) away: dropping them cannot pass."""
    import wiener_hmc_ref as HR
    rec = R.recorded()
    m, sd = rec["two"]                                                 # (tests/test_wiener_censored_hmc_host.py recomputes it)
    assert np.all(np.abs(m - rec["two_without"][0]) / sd > 0.5)
    r, th0 = _fit(R.with_timeouts(HR.Y20, R.TIMEOUTS_2D), 3, HR.FIXED_2D)
    assert r["draws"].shape == (256, 375, 5) and not r["flagged"].any()
    assert np.array_equal(r["draws"][:, :, 2:], np.broadcast_to(th0[:, None, 2:].astype(np.float32), (256, 375, 3)))
    check_statistics(r["draws"], [0, 1], m, sd)


def test_five_free_columns_with_two_timeouts_match_importance_sampling_from_the_prior():
    import wiener_hmc_ref as HR
    rec = R.recorded()
    m, sd = rec["five"]
    assert rec["five_ess"] >= 20_000
    r, _ = _fit(R.with_timeouts(HR.Y10, R.TIMEOUTS_5D), 31, {})
    assert not r["flagged"].any()
    check_statistics(r["draws"], [0, 1, 2, 3, 4], m, sd)


def test_hmc_fit_end_to_end_on_simulated_data_with_timeouts():
    """8 participants x 40 trials from basic_ddm_dc.batch_simulate_trials at a 1 s horizon, slow enough that several sets hold timeouts;
    4 chains, 300 + 500 iterations, censored=True: no chain flagged, Rhat < 1.05 on every variable (section 17's end-to-end bound).  The
    same data without the keyword: refused as a host array, flagged as a device tensor."""
    import torch
    from bayesflow_nddms_amd import basic_ddm_dc, diagnostics as Dg, engine, mcmc
    rng = np.random.default_rng(31)
    params = np.stack([rng.uniform(-0.8, 0.8, 8), rng.uniform(1.3, 1.8, 8), rng.uniform(0.4, 0.6, 8), rng.uniform(0.2, 0.35, 8), np.ones(8)], 1)
    data = basic_ddm_dc.batch_simulate_trials(params.astype(np.float32), 40, dt=.01, max_steps=100., seed=5, set_offset=0, with_summary=False)["sim_data"]
    n_to = (data[..., 1] == 0).sum(1)
    print("timeouts per set", n_to)
    assert (n_to > 0).sum() >= 3 and np.all(n_to < 40)
    fit = basic_ddm_dc.fit_hmc(data, chains=4, warmup=300, samples=500, thin=5, seed=8, censored=True)
    for k in ("alpha", "ndt", "beta", "delta", "varsigma", "log_post"):
        assert fit[k].shape == (8, 100, 4) and fit[k].dtype == np.float64 and np.all(np.isfinite(fit[k]))
    assert not fit["flagged"].any()
    dg = Dg.rhat_neff({k: fit[k] for k in ("alpha", "ndt", "beta", "delta", "varsigma")})
    print({k: v["rhat"].max() for k, v in dg.items()}, fit["accept_rate"].min(), fit["accept_rate"].max())
    assert all(np.all(v["rhat"] < 1.05) for v in dg.values())
    with pytest.raises(ValueError, match="no gradient here"):
        basic_ddm_dc.fit_hmc(data, chains=4, warmup=300, samples=500, thin=5, seed=8)
    th = mcmc.hmc_init(data, 4, 8, censored=True).reshape(-1, 5)
    st = mcmc.make_state(th, np.repeat(data, 4, 0), censored=True)
    r = engine.wiener_hmc(engine.BASIC_DDM_DC, torch.as_tensor(data).cuda(), st, chains_per_dataset=4, n_iter=2)
    assert np.array_equal(r["flagged"].cpu().numpy().reshape(8, 4).all(1), n_to > 0) and not r["flagged"].cpu().numpy().reshape(8, 4)[n_to == 0].any()


# (kernel, VGPRs + AGPRs, AGPRs, LDS bytes) of the kernels the flag does not reach, as the parent commit's code object has them
DEFAULTS = {"17wiener_hmc_kernelE": (310, 54, 65536), "23wiener_hmc_joint_kernelE": (273, 17, 65536),
            "31wiener_hmc_joint_prepass_kernelE": (58, 0, 16), "29wiener_hmc_joint_sigma_kernelE": (67, 0, 0),
            "18wiener_grad_kernelILi0ELb0ELb0EE": (80, 0, 0), "18wiener_grad_kernelILi0ELb1ELb0EE": (78, 0, 8192),
            "18wiener_grad_kernelILi3ELb0ELb0EE": (79, 0, 0), "18wiener_grad_kernelILi3ELb1ELb0EE": (74, 0, 8192)}
CENSORED = ("26wiener_hmc_censored_kernelE", "32wiener_hmc_censored_joint_kernelE", "18wiener_grad_kernelILi0ELb0ELb1EE",
            "18wiener_grad_kernelILi0ELb1ELb1EE")


def test_resources_of_the_shipped_code_object():
    """Read from the code object inside the library the tests run (its metadata notes).  The kernels without the flag keep the parent's
    VGPR, AGPR and LDS figures and no scratch; the four censored ones have no private segment, no VGPR spill and no dynamic stack either
    (measured: the censored sampler kernels 256 VGPRs + 80 / 40 AGPRs, the gradient kernels 120 / 114 VGPRs)."""
    from bayesflow_nddms_amd.build import SO_PATH
    bindir = next((b for b in ("/opt/rocm/lib/llvm/bin", "/opt/rocm/llvm/bin") if os.path.exists(os.path.join(b, "llvm-readelf"))), None)
    tool = lambda n: os.path.join(bindir, n) if bindir else shutil.which(n)
    if not all(tool(n) for n in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("needs llvm-objcopy, clang-offload-bundler and llvm-readelf")
    with tempfile.TemporaryDirectory() as td:
        fat, co = os.path.join(td, "fat.bin"), os.path.join(td, "k.co")
        subprocess.check_call([tool("llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", SO_PATH, os.path.join(td, "copy.so")])
        subprocess.check_call([tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               f"--output={co}"])
        notes = subprocess.run([tool("llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    rows = {}
    for block in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        rows[name] = {k: re.search(rf"\.{k}:\s+(\S+)", block).group(1) for k in ("private_segment_fixed_size", "vgpr_spill_count", "uses_dynamic_stack",
                                                                               "group_segment_fixed_size", "vgpr_count")}
        rows[name]["agpr_count"] = block.split("\n")[0].strip()
    pick = lambda key: [r for n, r in rows.items() if n.startswith("_ZN4nddm" + key)]
    for key, (vgpr, agpr, lds) in DEFAULTS.items():
        (r,) = pick(key)
        print(key, r)
        assert (int(r["vgpr_count"]), int(r["agpr_count"]), int(r["group_segment_fixed_size"])) == (vgpr, agpr, lds), key
        assert r["private_segment_fixed_size"] == "0" and r["vgpr_spill_count"] == "0" and r["uses_dynamic_stack"] == "false", key
    for key in CENSORED:
        (r,) = pick(key)
        print(key, r)
        assert r["private_segment_fixed_size"] == "0" and r["vgpr_spill_count"] == "0" and r["uses_dynamic_stack"] == "false", key
        assert int(r["vgpr_count"]) - int(r["agpr_count"]) <= 256
