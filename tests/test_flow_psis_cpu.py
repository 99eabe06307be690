"""Pareto-smoothed importance weights (amortizer.py: pareto_smooth, pareto_k_threshold, weighted_moments, posterior_importance(smooth=
True); csrc/train_psis.h, csrc/train_psis.hip) as far as a machine without a GPU can hold them: the torch evaluation and the host
build of the kernel's own arithmetic against the definition in NumPy (tests/psis_ref.py), the crafted sets, the properties, the
statistics the smoothing is there for, the library's exports and host refusals, and the public call on the CPU path.

Tolerance of the approximate parts (pareto_k absolute; sigma and the smoothed values relative to max(1, |value|)): 1000 x the largest
difference the definition shows against itself under three summation orders on this file's inputs (psis_ref.tolerances()); measured
3.9e-13 and 4.1e-14, so the bars are 3.9e-10 and 4.1e-11.  Measured against them on the CPU: the torch evaluation 9.7e-14 and 1.0e-14,
the host build of csrc/train_psis.h the same two figures (the device's figures: tests/test_gpu_flow_psis.py)."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import psis_ref as R
from test_flow_wquantile_cpu import OLD_KEYS, _host_likelihood, _small_amortizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


def smooth_np(lw, **kw):
    """amortizer.pareto_smooth on NumPy log weights [B, S] (CPU tensors: the torch evaluation) -> NumPy arrays."""
    import torch
    from bayesflow_nddms_amd.amortizer import pareto_smooth
    return {k: v.numpy() for k, v in pareto_smooth(torch.from_numpy(np.ascontiguousarray(lw, np.float64)), **kw).items()}


def check_crafted(smooth):
    """Every crafted set through `smooth` (log weights [1, S] -> a result in NumPy) against the definition and what the set is for."""
    for name, (lw, want) in R.crafted_cases().items():
        got = smooth(lw[None])
        R.check(got, lw[None], name)
        if want["n_tail"] is not None:
            assert int(got["n_tail"][0]) == want["n_tail"], name
        assert bool(np.isfinite(got["pareto_k"][0])) == want["finite"], (name, got["pareto_k"][0])
        if want["changed"] is not None:
            assert R.same_bits(got["log_w"][0], lw) != want["changed"], name
    eq = smooth(R.crafted_cases()["equal weights"][0][None])
    assert eq["pareto_k"][0] == np.inf and int(eq["n_tail"][0]) == 0
    nothing = np.array([[-np.inf, np.nan, -np.inf, np.inf, np.nan, -np.inf]])
    got = smooth(nothing)
    assert got["pareto_k"][0] == np.inf and int(got["n_tail"][0]) == 0 and R.same_bits(got["log_w"], nothing)
    assert got["cutoff"][0] == R.LOG_DBL_MIN and np.isnan(got["sigma"][0])


def check_properties(smooth):
    """Smoothed values do not decrease in rank, lie in [m + cutoff, m], and a permutation of distinct rows changes no bit."""
    rng = np.random.default_rng(5)
    for S, s in ((26, 1.0), (257, 3.0), (1000, 1.0), (4097, 10.0)):
        lw = rng.normal(0.0, s, S)
        got = smooth(lw[None])
        ref = R.psis(lw)
        assert np.isfinite(got["pareto_k"][0]) and int(got["n_tail"][0]) == R.tail_size(S)
        tail = got["log_w"][0][ref["rows"]]
        m = lw.max()
        assert np.all(np.diff(tail) >= 0.0) and tail.max() <= m and tail.min() >= m + got["cutoff"][0]
        perm = rng.permutation(S)
        again = smooth(lw[perm][None])
        for k in ("pareto_k", "sigma", "cutoff"):
            assert R.same_bits(again[k], got[k]), (S, k)
        assert int(again["n_tail"][0]) == int(got["n_tail"][0]) and R.same_bits(again["log_w"][0], got["log_w"][0][perm]), S


def test_reference_reproduces_the_stated_cases():
    """tests/psis_ref.py itself: M and the threshold; the crafted sets as stated -- equal weights: k = inf, n_tail 0, bits unchanged; one
    positive weight: no fit; exactly 5 and 6 finite weights: the fit runs on 5 and on 6; one weight e^800 above the rest: the cutoff's
    floor applies and n_tail is 1; NaN, +inf and -inf entries weigh nothing and keep their bits."""
    assert [R.tail_size(S) for S in (1, 4, 24, 25, 26, 100, 225, 226, 10_000, 16_384)] == [1, 1, 5, 5, 6, 20, 45, 46, 300, 384]
    assert R.k_threshold(10_000) == 0.7 and abs(R.k_threshold(100) - 0.5) < 1e-15 and R.k_threshold(1000) == min(1.0 - 1.0 / 3.0, 0.7)
    cases = R.crafted_cases()
    r = R.psis(cases["equal weights"][0])
    assert r["pareto_k"] == np.inf and r["n_tail"] == 0 and R.same_bits(r["log_w"], cases["equal weights"][0])
    r = R.psis(cases["one positive weight"][0])
    assert r["pareto_k"] == np.inf and r["n_tail"] == 1 and r["cutoff"] == R.LOG_DBL_MIN
    for n in (5, 6):
        r = R.psis(cases[f"exactly {n} finite weights"][0])
        assert r["n_tail"] == n and np.isfinite(r["pareto_k"]) and r["sigma"] > 0.0
    r = R.psis(cases["one weight e^800 above the rest"][0])
    assert r["cutoff"] == R.LOG_DBL_MIN and r["n_tail"] == 1 and r["pareto_k"] == np.inf
    lw = cases["nan, +inf and -inf entries"][0]
    r = R.psis(lw)
    bad = ~np.isfinite(lw)
    assert bad.sum() == 9 and R.same_bits(r["log_w"][bad], lw[bad]) and not np.isin(np.nonzero(bad)[0], r["rows"]).any()
    assert np.isfinite(r["pareto_k"]) and r["n_tail"] == R.tail_size(400)
    r = R.psis(cases["a tie straddling the cutoff"][0])
    assert r["n_tail"] == R.tail_size(500) - 1
    r = R.psis(cases["no exp difference at the quartile"][0])
    assert not np.isfinite(r["pareto_k"]) and r["n_tail"] == 20 and R.same_bits(r["log_w"], cases["no exp difference at the quartile"][0])


def test_torch_evaluation_against_the_definition():
    """S in {1, 4, 24, 25, 26, 64, 65, 257, 1000, 4097, 10 000} x log weights N(0, s^2), s in {0.3, 1, 3, 10, 30}: n_tail, cutoff and the set
    of changed rows equal exactly, unchanged rows bit for bit, pareto_k, sigma and the smoothed values within the tolerance."""
    tol = R.tolerances()
    print("tolerances", tol)
    assert 1e-11 < tol[0] < 1e-8 and 1e-12 < tol[1] < 1e-8           # (the rule's output, not a bar chosen here)
    worst = (0.0, 0.0)
    for S, s, lw in R.grid():
        got = smooth_np(lw[None])
        assert set(got) == {"pareto_k", "sigma", "cutoff", "n_tail", "log_w"} and got["n_tail"].dtype == np.int64
        assert all(got[k].shape == (1,) and got[k].dtype == np.float64 for k in ("pareto_k", "sigma", "cutoff"))
        w = R.check(got, lw[None], (S, s))
        worst = (max(worst[0], w[0]), max(worst[1], w[1]))
        assert int(got["n_tail"][0]) == R.tail_size(S) and (S < 21 or np.isfinite(got["pareto_k"][0])), (S, s)      # (M >= 5 from S = 21 on)
    print("torch evaluation: largest |k - ref|", worst[0], "largest relative difference of sigma / smoothed values", worst[1])
    # several sets in one call, the diagnostic alone, one set as a vector
    import torch
    from bayesflow_nddms_amd.amortizer import pareto_smooth
    lw = np.stack([R.gaussian_log_w(257, s, 9) for s in (0.3, 3.0, 30.0)])
    got = smooth_np(lw)
    R.check(got, lw, "batch")
    only = smooth_np(lw, want_log_w=False)
    assert "log_w" not in only and all(R.same_bits(only[k], got[k]) for k in ("pareto_k", "sigma", "cutoff", "n_tail"))
    one = pareto_smooth(torch.from_numpy(lw[1]))
    assert one["log_w"].shape == (1, 257) and R.same_bits(one["log_w"].numpy()[0], got["log_w"][1])
    f32 = pareto_smooth(torch.from_numpy(lw.astype(np.float32)))                # (taken to float64 first)
    R.check({k: v.numpy() for k, v in f32.items()}, lw.astype(np.float32).astype(np.float64), "float32 input")
    with pytest.raises(ValueError):
        pareto_smooth(torch.zeros(2, 0, dtype=torch.float64))
    with pytest.raises(ValueError):
        pareto_smooth(torch.zeros(2, 3, 4, dtype=torch.float64))


def test_crafted_sets():
    check_crafted(smooth_np)


def test_properties():
    check_properties(smooth_np)


def test_threshold_and_tail_size():
    from bayesflow_nddms_amd.amortizer import pareto_k_threshold, pareto_tail_size
    for S in (1, 2, 4, 24, 25, 26, 99, 100, 101, 225, 226, 1000, 10_000, 16_384, 16_385, 1_000_000):
        assert pareto_tail_size(S) == R.tail_size(S) == min(math.ceil(S / 5), math.ceil(3 * math.sqrt(S))), S
        assert pareto_k_threshold(S) == R.k_threshold(S), S
    assert pareto_k_threshold(10_000) == 0.7 and pareto_k_threshold(100) == 1.0 - 1.0 / math.log10(100)


HOST_SHIM = r"""
#include "train_psis.h"
using namespace nddm_train;
extern "C" void psis_host(int n, const double *x_sorted, double cutoff, double *pareto_k, double *sigma, double *smoothed)
{
    double y[PSIS_MAX_TAIL];
    const double e_c = exp(cutoff);
    for (int r = 0; r < n; ++r) y[r] = exp(x_sorted[r]) - e_c;
    psis_fit_host(n, y, e_c, pareto_k, sigma, smoothed);
}
"""


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_host_build_of_the_header_against_the_definition(tmp_path):
    """csrc/train_psis.h compiled for the host (no contraction, as the kernel's pragmas have it): the kernel's own arithmetic -- the
    candidates, the 64-lane tree, the profile, the weights, the quantiles -- on the sorted tails of the definition test's inputs and
    of the crafted sets, against the NumPy evaluation on the same tails."""
    src, so = tmp_path / "psis_host.cpp", tmp_path / "psis_host.so"
    src.write_text(HOST_SHIM)
    subprocess.check_call([CXX, "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                           "-I", os.path.join(ROOT, "bayesflow_nddms_amd", "csrc"), "-o", str(so), str(src)])
    H = ctypes.CDLL(str(so))
    H.psis_host.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_double] + [ctypes.c_void_p] * 3
    H.psis_host.restype = None
    tol_k, tol_v = R.tolerances()
    worst_k, worst_v, fits = 0.0, 0.0, 0
    inputs = [((S, s), lw) for S, s, lw in R.grid()] + [(name, lw) for name, (lw, _) in R.crafted_cases().items()]
    for label, lw in inputs:
        ref = R.psis(lw)
        n = ref["n_tail"]
        if n <= 4:
            continue
        m = lw[np.isfinite(lw)].max()
        xs = np.ascontiguousarray(lw[ref["rows"]] - m)
        k, sigma, sm = np.zeros(1), np.zeros(1), np.full(n, np.nan)
        H.psis_host(n, xs.ctypes.data, float(ref["cutoff"]), k.ctypes.data, sigma.ctypes.data, sm.ctypes.data)
        if not np.isfinite(ref["pareto_k"]):
            assert not np.isfinite(k[0]) and np.isnan(sm).all(), label
            continue
        fits += 1
        assert abs(k[0] - ref["pareto_k"]) <= tol_k, (label, k[0], ref["pareto_k"])
        want = ref["log_w"][ref["rows"]] - m
        dv = max(float(R._rel(sigma[0], ref["sigma"])), float(R._rel(sm + m, want + m).max()))
        assert dv <= tol_v, (label, dv, tol_v)
        worst_k, worst_v = max(worst_k, abs(k[0] - ref["pareto_k"])), max(worst_v, dv)
    assert fits >= 45
    print("host build: fits", fits, "largest |k - ref|", worst_k, "largest relative difference of sigma / smoothed values", worst_v)


def _gaussian_case(s, seeds, S=10_000):
    """x ~ N(0, s^2) as the proposal of a standard normal target: log w = log N(x; 0, 1) - log N(x; 0, s^2) up to a constant."""
    x = np.stack([np.random.default_rng(seed).normal(0.0, s, S) for seed in range(seeds)])
    return x, -0.5 * x * x + 0.5 * x * x / (s * s)


@pytest.mark.parametrize("s", [0.5, 0.7, 0.9])
def test_k_hat_estimates_the_tail_index(s):
    """A standard normal target, a normal proposal of standard deviation s, 10 000 draws: the weights' tail index is 1 - s^2.  The mean
    of pareto_k over 40 seeds is within 0.1 of it (the NumPy definition gives 0.065, 0.029 and 0.019)."""
    _, lw = _gaussian_case(s, 40)
    k = smooth_np(lw, want_log_w=False)["pareto_k"]
    print("s", s, "mean k-hat", k.mean(), "+-", k.std(), "truth", 1.0 - s * s)
    assert abs(k.mean() - (1.0 - s * s)) <= 0.1


def test_smoothing_lowers_the_error_of_the_estimate():
    """The same case at s = 0.7, 200 seeds: the root-mean-square error of the self-normalised estimate of E[x^2] = 1 with the smoothed
    weights is at most 0.8 x that with the raw weights (the NumPy definition gives 0.059 against 0.100)."""
    x, lw = _gaussian_case(0.7, 200)
    sm = smooth_np(lw)["log_w"]

    def rmse(l):
        u = np.exp(l - l.max(axis=1, keepdims=True))
        return math.sqrt(np.mean(((u * x * x).sum(axis=1) / u.sum(axis=1) - 1.0) ** 2))

    raw, smoothed = rmse(lw), rmse(sm)
    print("rmse raw", raw, "smoothed", smoothed, "ratio", smoothed / raw)
    assert smoothed <= 0.8 * raw


def test_library_exports_the_entry_and_refuses_bad_arguments_on_the_host():
    """Called with null or dummy pointers, on the host: had the entry read or launched anything, this would not return."""
    from bayesflow_nddms_amd import _train_lib, build
    assert any(p.endswith("train_psis.hip") for p in build.TRAIN_SOURCES) and any(p.endswith("train_psis.h") for p in build.TRAIN_HEADERS)
    L = _train_lib.lib()
    assert L is not None, "libnddm_train.so did not build / load"
    cap = L.nddm_train_pareto_smooth_max_draws()
    assert cap == 16384 == L.nddm_train_weighted_quantiles_max_draws()
    buf = (ctypes.c_char * 64)()
    a, o = ctypes.addressof(buf), ctypes.addressof(buf) + 8

    def rc(B=1, S=100, M=20, log_w=a, out=o, k=a, sigma=a, n_tail=a, cutoff=a):
        return L.nddm_train_pareto_smooth(B, S, M, log_w, out, k, sigma, n_tail, cutoff, None)

    assert rc(B=0) == 1 and rc(S=0) == 1 and rc(S=cap + 1, M=385) == 1 and rc(M=0) == 1 and rc(M=101) == 1
    assert rc(S=512, M=69) == 1 and rc(S=4096, M=193) == 1 and rc(S=cap, M=385) == 1      # (past an instantiation's tail capacity)
    assert rc(log_w=None) == 1 and rc(k=None) == 1 and rc(sigma=None) == 1 and rc(n_tail=None) == 1 and rc(cutoff=None) == 1
    assert rc(out=a) == 1                                                                  # (in place)


def test_weighted_moments_are_importance_weights_on_its_own_log_weights():
    """importance_weights(want_log_w=True) on the special rows of tests/flow_importance_ref.py, then weighted_moments on the returned log_w:
    the same numbers (the torch evaluation both times: the same operations on the same values, bit for bit; n_nan's rows have become
    zero weights, so the two counts are compared by their sum)."""
    import torch
    from flow_importance_ref import special_inputs
    from bayesflow_nddms_amd.amortizer import importance_weights, weighted_moments
    theta, log_q, log_lik = (torch.from_numpy(v) for v in special_inputs(300))
    w = importance_weights(theta, log_q, log_lik, "basic", want_log_w=True)
    got = weighted_moments(theta, w["log_w"])
    assert "log_w" not in got
    for k in ("log_evidence", "ess", "max_share", "mean", "sd"):
        assert R.same_bits(got[k].numpy(), w[k].numpy()), k
    assert torch.equal(got["n_zero"] + got["n_nan"], w["n_zero"] + w["n_nan"])
    one = weighted_moments(theta[2], w["log_w"][2])
    assert one["mean"].shape == (1, 5) and R.same_bits(one["mean"].numpy()[0], w["mean"].numpy()[2])
    with pytest.raises(ValueError):
        weighted_moments(theta, w["log_w"][:, :10])


def test_posterior_importance_smooth_on_the_cpu(monkeypatch):
    """smooth=False returns exactly the old keys.  With smooth=True, under the same seed: `raw` is the smooth=False call bit for bit;
    pareto_k and n_tail are pareto_smooth's on the kept log_w and log_w_smoothed its output; mean / std / ess / max_share / log_evidence are
    weighted_moments' of the draws and the smoothed weights; the quantiles weighted_draw_quantiles' on them; k_threshold is
    pareto_k_threshold(S); with a launch per set (z_bytes=1) every set's pareto_k is still that of its own kept log_w."""
    import torch
    from bayesflow_nddms_amd.amortizer import pareto_k_threshold, pareto_smooth, weighted_draw_quantiles, weighted_moments
    _host_likelihood(monkeypatch)
    B, S = 2, 300
    am, conf = _small_amortizer(B)
    torch.manual_seed(3)
    old = am.posterior_importance(conf, S)
    assert set(old) == OLD_KEYS
    torch.manual_seed(3)
    new = am.posterior_importance(conf, S, smooth=True, keep_draws=True, keep_weights=True, probs=(.025, .5, .975))
    assert set(new) == OLD_KEYS | {"pareto_k", "n_tail", "k_threshold", "raw", "draws", "log_q", "log_w", "log_w_smoothed", "quantiles",
                                   "probs", "median", "95lower", "95upper"}
    assert set(new["raw"]) == {"mean", "std", "ess", "max_share", "log_evidence"}
    for k in new["raw"]:
        assert R.same_bits(new["raw"][k], old[k]), k
    for k in ("n_zero", "n_nan"):
        assert np.array_equal(new[k], old[k])
    assert new["k_threshold"] == pareto_k_threshold(S) and new["pareto_k"].shape == (B,) and new["n_tail"].dtype == np.int64
    draws, lw = torch.from_numpy(new["draws"]), torch.from_numpy(new["log_w"])
    sm = pareto_smooth(lw)
    assert R.same_bits(sm["pareto_k"].numpy(), new["pareto_k"]) and np.array_equal(sm["n_tail"].numpy(), new["n_tail"])
    assert R.same_bits(sm["log_w"].numpy(), new["log_w_smoothed"]) and not R.same_bits(new["log_w_smoothed"], new["log_w"])
    R.check({k: v.numpy() for k, v in sm.items()}, new["log_w"], "public")
    print("public path (cpu): pareto_k", new["pareto_k"], "n_tail", new["n_tail"], "ess raw", new["raw"]["ess"], "smoothed", new["ess"])
    wm = weighted_moments(draws, sm["log_w"])
    for k in ("mean", "sd", "ess", "max_share", "log_evidence"):
        assert R.same_bits(wm[k].numpy(), new["std" if k == "sd" else k]), k
    q = weighted_draw_quantiles(draws, (.025, .5, .975), log_w=sm["log_w"])["quantiles"].numpy()
    assert R.same_bits(q, new["quantiles"]) and R.same_bits(new["median"], q[:, 1])
    split = am.posterior_importance(conf, S, smooth=True, z_bytes=1, keep_weights=True)          # a launch per set
    assert "quantiles" not in split and "draws" not in split
    sm = pareto_smooth(torch.from_numpy(split["log_w"]))
    assert R.same_bits(sm["pareto_k"].numpy(), split["pareto_k"]) and R.same_bits(sm["log_w"].numpy(), split["log_w_smoothed"])
