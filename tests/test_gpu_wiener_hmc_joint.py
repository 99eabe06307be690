"""GPU tests of the joint sampler (engine.wiener_hmc_joint -> nddm_wiener_hmc_joint -> the pre-pass, participant and sigma kernels of
csrc/nddm_wiener_hmc_joint.h): the device against the host build of the same header, the tie to nddm_wiener_hmc bit for bit, the bits
tests (cut = uncut, joint-chain independence, flags), the energy bars, both statistics tests of tests/test_wiener_hmc_joint_host.py,
mcmc.hmc_fit_joint end to end, and the kernels' resources read from the shipped library's code object."""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import test_wiener_hmc_joint_host as T
import wiener_hmc_joint_ref as JR
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu
HAVE_CXX = T.HAVE_CXX


@pytest.fixture(scope="module")
def host():
    import wiener_hmc_joint_host as J
    with tempfile.TemporaryDirectory() as td:
        yield J, td, J.build(td) if HAVE_CXX else None


def dev_run(data, ext, state, sigma, **kw):
    """engine.wiener_hmc_joint with numpy (or device tensors) in and numpy out: the host tool's run()."""
    from bayesflow_nddms_amd import engine
    import torch
    d = torch.as_tensor(np.asarray(data, np.float32)).cuda()              # (device data: the kernels, not the adapter, meet a bad data set)
    r = engine.wiener_hmc_joint(engine.BASIC_DDM_DC, d, np.asarray(ext, np.float64), state, sigma, **kw)
    return {k: v.cpu().numpy() for k, v in r.items()}


def modules():
    import wiener_hmc_host as H
    import wiener_hmc_joint_host as J
    return J, H


@pytest.mark.parametrize("N", [1, 20, 64, 65, 130])
@pytest.mark.parametrize("P,S", [(2, 1), (2, 3), (5, 1), (5, 3)])
def test_device_equals_the_host_build_within_the_recorded_tolerance(host, N, P, S):
    """3 iterations of 4 leapfrog steps from the same state, sigma sampled.  Tolerance: 4 x what the host's float32 build shows against its
    float64 build FOR THE SAME CASE (profiles/r18_wiener_hmc_joint_host.json), on log_post (relative), the final q and the final sigma
    (float64, absolute); a chain whose accept decision flipped is left out.  Measured on the MI355X: see DESIGN.md section 18."""
    J, td, exe = host
    if exe is None:
        pytest.skip("no host C++ compiler")
    _, H = modules()
    tol = T._profile()["device_tolerance"][f"N{N}_P{P}_S{S}"]
    data, ext, theta = J.case(N, P, S)
    st = H.init_state(theta, data, S, eps0=0.02)
    sg = np.full(S, J.COMPARE_SIGMA)
    a, b = dev_run(data, ext, st, sg, **J.COMPARE), J.run(exe, td, data, ext, st, sg, **J.COMPARE)
    same, dl, dq, same_k, ds = J.compare(a, b, theta)
    print("N", N, "P", P, "S", S, "left out", int((~same).sum()), int((~same_k).sum()), "log_post", dl, tol["log_post_rel"], "q", dq, tol["q_abs"],
          "sigma", ds, tol["sigma_abs"])
    assert not a["flagged"].any() and np.all(np.isfinite(a["draws"])) and np.all(np.isfinite(a["sigma_draws"]))
    assert (~same).mean() <= 0.02                                       # (at these chain counts: none)
    assert dl <= tol["log_post_rel"] and dq <= tol["q_abs"] and ds <= tol["sigma_abs"]
    assert np.array_equal(a["divergent"][same], b["divergent"][same])


@pytest.mark.parametrize("N", [1, 20, 65, 130])
@pytest.mark.parametrize("S", [1, 3])
def test_a_vanishing_ext_term_gives_the_independent_samplers_bits(N, S):
    """NDDM_HMC_SIGMA_FIXED and sigma = 1e150: draws, log_post, states, divergent counts and accept equal nddm_wiener_hmc's for the same data,
    states, seed and offsets -- 12 participant launches of one iteration against one launch of 12."""
    from bayesflow_nddms_amd import engine
    import torch
    J, H = modules()
    data, ext, theta = J.case(N, 3, S)
    st = H.init_state(theta, data, S)
    a = dev_run(data, ext, st, np.full(S, 1e150), n_iter=12, chain_offset=100, iter_offset=4, sigma_fixed=True, **T.TIE)
    b = engine.wiener_hmc(engine.BASIC_DDM_DC, torch.as_tensor(data).cuda(), st, chains_per_dataset=S, n_iter=12, chain_offset=100, iter_offset=4, **T.TIE)
    b = {k: v.cpu().numpy() for k, v in b.items()}
    for k in ("draws", "log_post", "state", "divergent", "flagged", "accept"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert a["draws"].shape == (3 * S, 6, 5) and np.ptp(a["draws"][:, :, 0], axis=1).min() > 0
    # (out_sigma is float32: 1e150 is +inf there; the float64 sigma is untouched)
    assert np.all(np.isposinf(a["sigma_draws"])) and np.all(a["sigma"] == 1e150) and np.all(np.isnan(a["sigma_accept"]))


def test_cut_runs_give_the_bits_of_the_uncut_run():
    T.check_cut(dev_run, *modules())


def test_joint_chains_do_not_depend_on_their_neighbours():
    """A NaN state and sigma = -1 reach the kernels only in device tensors (the adapter refuses host ones)."""
    import torch
    T.check_neighbours(dev_run, *modules(), device_inputs=lambda st, sg: (torch.as_tensor(st).cuda(), torch.as_tensor(sg).cuda()))


def test_a_bad_data_set_flags_every_chain():
    T.check_bad_data(dev_run, *modules())


def test_device_state_and_sigma_are_updated_in_place():
    from bayesflow_nddms_amd import engine
    import torch
    J, H = modules()
    data, ext, st, sg = T.bits_case(J, H)
    sd, gd = torch.as_tensor(st).cuda(), torch.as_tensor(sg).cuda()
    r = engine.wiener_hmc_joint(engine.BASIC_DDM_DC, data, ext, sd, gd, n_iter=6, n_leapfrog=3, seed=2)
    assert r["state"] is sd and r["sigma"] is gd
    ref = dev_run(data, ext, st, sg, n_iter=6, n_leapfrog=3, seed=2)
    assert np.array_equal(sd.cpu().numpy(), ref["state"]) and np.array_equal(gd.cpu().numpy(), ref["sigma"])


@pytest.mark.parametrize("P", [2, 5, 65, 258])
def test_sigma_draws_equal_the_host_builds_across_the_wave_width(host, P):
    """N = 1, S = 1, no column free (the participants stand still, so SS is the same float64 on both sides): out_sigma of 40 iterations
    bit for bit.  P = 65 and 258 cross one wave's width in the SS reduction (lanes stride over p) and, at 258, one round of 64 Philox
    blocks in the chi-square draw (257 normals = 65 blocks)."""
    J, td, exe = host
    if exe is None:
        pytest.skip("no host C++ compiler")
    _, H = modules()
    data, ext, theta = J.case(1, P, 1)
    st = H.init_state(theta, data, 1, free=0)
    kw = dict(n_iter=40, n_leapfrog=1, free_mask=0, seed=9, chain_offset=3)
    a, b = dev_run(data, ext, st, np.array([1.0]), **kw), J.run(exe, td, data, ext, st, np.array([1.0]), **kw)
    assert np.array_equal(a["sigma_draws"], b["sigma_draws"]) and np.array_equal(a["sigma"], b["sigma"])
    assert np.array_equal(a["sigma_accept"], b["sigma_accept"]) and np.ptp(a["sigma_draws"]) > 0
    assert np.array_equal(a["state"][:, :5], st[:, :5])


@pytest.mark.parametrize("N", [1, 20, 64, 65, 130])
def test_energy_error_with_the_ext_term_stays_under_the_recorded_bar(N):
    """sigma = 0.2, eps = 1e-3, 8 leapfrog steps, 4 iterations, 256 chains: the host test's bar (4 x the host build's largest, per shape)."""
    J, H = modules()
    data, ext, theta = J.energy_case(N)
    r = dev_run(data, ext, H.init_state(theta, data, 64, eps0=1e-3), np.full(64, J.ENERGY_SIGMA), **J.ENERGY)
    worst = float(np.max(r["state"][:, 11]))
    print("N", N, "largest |H1 - H0|", worst)
    assert not r["flagged"].any() and not r["divergent"].any() and np.all(np.isfinite(r["state"][:, 10:]))
    assert worst <= T._profile()["energy_bar"][str(N)]


def test_free_drift_boundary_and_sigma_match_the_nested_quadrature():
    """(a) of the host test on the device: 64 joint chains x 4 participants, 300 + 7500 iterations at thin 5 (two calls of <= 4096)."""
    assert abs(JR.recorded()["a"][0][-1] - 3.0) >= 0.3
    T.check_a(T.fit_joint(dev_run, JR.Y20, JR.EXT_A, 3, JR.FIXED_2D))


def test_five_free_columns_with_sigma_fixed_match_importance_sampling():
    assert min(JR.recorded()["b_ess"]) >= 20_000
    T.check_b(T.fit_joint(dev_run, JR.Y10, JR.EXT_B, 31, {}, sigma=JR.SIGMA_B))


def test_hmc_fit_joint_end_to_end():
    """3 participants x 40 trials, 4 chains, 300 + 500 iterations through alpha_not_scaled.fit_hmc: sigma [1, 100, 4], everything finite,
    Rhat < 1.05, acceptance in [0.6, 0.95]."""
    from bayesflow_nddms_amd import alpha_not_scaled
    data, ext = T.fit_data()
    T.check_fit(alpha_not_scaled.fit_hmc(data[..., 0] * data[..., 1], ext, chains=4, warmup=300, samples=500, thin=5, seed=8), 3)


def test_the_joint_kernels_have_no_scratch():
    """Read from the code object inside the library the tests run (its metadata notes): no private segment, no spills, no dynamic stack."""
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
        rows[name] = {k: re.search(rf"\.{k}:\s+(\S+)", block).group(1) for k in ("private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count",
                                                                               "uses_dynamic_stack", "group_segment_fixed_size", "vgpr_count")}
    mine = {n: r for n, r in rows.items() if "wiener_hmc_joint" in n}
    print(json.dumps(mine, indent=1))
    assert len(mine) == 3 and {n.split("nddm")[1][:2] for n in mine} == {"31", "23", "29"}     # prepass, participant, sigma (mangled lengths)
    for n, r in mine.items():
        assert r["private_segment_fixed_size"] == "0" and r["vgpr_spill_count"] == "0" and r["uses_dynamic_stack"] == "false", n
    assert [r["group_segment_fixed_size"] for n, r in mine.items() if "23wiener_hmc_joint_kernel" in n] == ["65536"]
