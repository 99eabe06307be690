"""Pareto-smoothed importance weights on the device (csrc/train_psis.hip: one workgroup per set selects the cutoff by a sort of 64-bit
keys in LDS, ranks the tail, runs the fit with a wave per candidate and writes the tail back by rank; amortizer.py: pareto_smooth,
weighted_moments, posterior_importance(smooth=True)): held to the definition in NumPy (tests/psis_ref.py) at the smallest shapes a
selection kernel goes wrong at -- exactly where the definition is exact, within psis_ref.tolerances() elsewhere -- to the crafted sets,
to its inputs staying unwritten, to independence of neighbours and of row order, and through the public call.

Tolerances (1000 x the definition's own spread over three summation orders): 3.9e-10 for pareto_k, 4.1e-11 relative for sigma and the
smoothed values.  MEASURED on the MI355X over the shapes below (test_kernel_against_the_definition prints them per shape): the kernel
within 1.1e-14 of the definition's pareto_k and 3.1e-15 in sigma and the smoothed values (both at S = 10 000), the torch evaluation on
the device at cap + 1 within 6.4e-15 and 2.0e-15 -- four orders below the bars, as round-off is."""
import numpy as np
import pytest

import psis_ref as R
from test_flow_psis_cpu import check_crafted, check_properties

pytestmark = pytest.mark.gpu


def _lib():
    from bayesflow_nddms_amd import _train_lib
    L = _train_lib.lib()
    assert L is not None, "libnddm_train.so did not build / load"
    return L


def _cap():
    return _lib().nddm_train_pareto_smooth_max_draws()


def _bits(a, b):
    import torch
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def smooth_dev(lw, **kw):
    """amortizer.pareto_smooth on NumPy log weights [B, S] as a device tensor -> NumPy arrays."""
    import torch
    from bayesflow_nddms_amd.amortizer import pareto_smooth
    return {k: v.cpu().numpy() for k, v in pareto_smooth(torch.as_tensor(np.ascontiguousarray(lw, np.float64), device="cuda"), **kw).items()}


@pytest.mark.parametrize("B,S", [(1, 1), (1, 24), (1, 25), (3, 63), (2, 64), (1, 65), (2, 257), (1, 513), (1, 4097), (1, 10000), (1, "cap"),
                                 (1, "cap + 1")], ids=lambda v: str(v))
def test_kernel_against_the_definition(B, S):
    """One draw; M = 5 at its smallest fit (24, 25); either side of a wave and of the padding block of 64; S either side of the
    instantiations' sizes (... 257 take the 512-item kernel, 513 the 4096, 4097, 10 000 and the cap the 16 384); cap + 1 takes the torch
    evaluation and must give the same definition.  Log weights N(0, s^2) with s in {0.3, 3, 30} per shape."""
    import torch
    from bayesflow_nddms_amd import amortizer
    kernel = S != "cap + 1"
    S = {"cap": _cap(), "cap + 1": _cap() + 1}.get(S, S)
    assert (amortizer._psis_lib(torch.zeros(B, S, dtype=torch.float64, device="cuda")) is not None) == kernel
    worst = (0.0, 0.0)
    for j, s in enumerate((0.3, 3.0, 30.0)):
        lw = np.stack([R.gaussian_log_w(S, s, 7000 + 10 * j + b) for b in range(B)])
        got = smooth_dev(lw)
        w = R.check(got, lw, (B, S, s))
        worst = (max(worst[0], w[0]), max(worst[1], w[1]))
        only = smooth_dev(lw, want_log_w=False)
        assert "log_w" not in only and all(R.same_bits(only[k], got[k]) for k in ("pareto_k", "sigma", "cutoff", "n_tail"))
    print(f"B {B} S {S} {'kernel' if kernel else 'torch'}: largest |k - ref| {worst[0]:.3g} (bar {R.tolerances()[0]:.3g}), largest relative "
          f"difference of sigma / smoothed values {worst[1]:.3g} (bar {R.tolerances()[1]:.3g})")


def test_crafted_sets():
    check_crafted(smooth_dev)


def test_properties():
    check_properties(smooth_dev)


@pytest.mark.parametrize("S", [65, 513, 10000])
def test_inputs_are_only_read_and_nothing_is_written_outside_the_outputs(S):
    """log_w and every output are views into sentinel-filled buffers with 4096-element guards: after the launch the input and all guards
    hold their bits and every output element was written."""
    import torch
    L, B, G, sent = _lib(), 2, 4096, -12345.0
    lw_np = np.stack([R.gaussian_log_w(S, 2.0, 40 + b) for b in range(B)])

    def guarded(n, dtype, value):
        big = torch.full((2 * G + n,), value, dtype=dtype, device="cuda")
        return big, big[G:G + n]

    big_in, lw = guarded(B * S, torch.float64, sent)
    lw.copy_(torch.as_tensor(lw_np, device="cuda").reshape(-1))
    keep = big_in.clone()
    bufs = {"out": guarded(B * S, torch.float64, sent), "pareto_k": guarded(B, torch.float64, sent), "sigma": guarded(B, torch.float64, sent),
            "cutoff": guarded(B, torch.float64, sent), "n_tail": guarded(B, torch.int64, -12345)}
    rc = L.nddm_train_pareto_smooth(B, S, R.tail_size(S), lw.data_ptr(), bufs["out"][1].data_ptr(), bufs["pareto_k"][1].data_ptr(),
                                    bufs["sigma"][1].data_ptr(), bufs["n_tail"][1].data_ptr(), bufs["cutoff"][1].data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert _bits(big_in, keep)
    for k, (big, view) in bufs.items():
        s = -12345 if k == "n_tail" else sent
        assert bool((big[:G] == s).all()) and bool((big[G + view.numel():] == s).all()), k
        assert not bool((view == s).any()), k
    got = {k: v[1].cpu().numpy() for k, v in bufs.items() if k != "out"}
    got["log_w"] = bufs["out"][1].view(B, S).cpu().numpy()
    R.check(got, lw_np, S)


def test_a_set_depends_on_its_own_rows_only():
    """A repeated launch repeats every bit; set 1 of a B = 3 launch equals that set launched alone; a permutation of (distinct) rows
    changes nothing -- at a shape of each instantiation."""
    import torch
    from bayesflow_nddms_amd.amortizer import pareto_smooth
    rng = np.random.default_rng(8)
    for S in (300, 2000, 10000):
        lw = torch.as_tensor(np.stack([R.gaussian_log_w(S, s, 60 + i) for i, s in enumerate((0.5, 2.0, 8.0))]), device="cuda")
        a, again = pareto_smooth(lw), pareto_smooth(lw)
        assert all(_bits(a[k], again[k]) for k in a), S
        alone = pareto_smooth(lw[1:2].contiguous())
        assert all(_bits(alone[k][0], a[k][1]) for k in a), S
        perm = torch.as_tensor(rng.permutation(S), device="cuda")
        p = pareto_smooth(lw[:, perm].contiguous())
        assert all(_bits(p[k], a[k]) for k in ("pareto_k", "sigma", "cutoff", "n_tail")) and _bits(p["log_w"], a["log_w"][:, perm]), S
        assert bool(torch.isfinite(a["pareto_k"]).all()) and not _bits(a["log_w"], lw)


def test_weighted_moments_on_the_device():
    """importance_weights' kernel on the special rows of tests/flow_importance_ref.py, then weighted_moments -- the same kernel with a
    neutral prior and a zero log_q -- on that call's own log_w: the same bits (the kernel's log w is then the given number)."""
    import torch
    from flow_importance_ref import special_inputs
    from bayesflow_nddms_amd.amortizer import _importance_lib, importance_weights, weighted_moments
    theta, log_q, log_lik = (torch.as_tensor(v, device="cuda") for v in special_inputs(300))
    assert _importance_lib(theta, log_q, log_lik) is not None
    w = importance_weights(theta, log_q, log_lik, "basic", want_log_w=True)
    got = weighted_moments(theta, w["log_w"])
    for k in ("log_evidence", "ess", "max_share", "mean", "sd"):
        assert _bits(got[k], w[k]), k
    assert torch.equal(got["n_zero"] + got["n_nan"], w["n_zero"] + w["n_nan"])
    assert bool(torch.isfinite(got["mean"][0]).all()) and bool(torch.isnan(got["mean"][1]).all())


def _counted(monkeypatch, L):
    calls = {"pareto": [], "importance": [], "wquantile": []}
    for key, name in (("pareto", "nddm_train_pareto_smooth"), ("importance", "nddm_train_importance"), ("wquantile", "nddm_train_weighted_quantiles")):
        real = getattr(L, name)
        monkeypatch.setattr(L, name, lambda *a, _real=real, _key=key: calls[_key].append(a[:3]) or _real(*a))
    return calls


def test_public_path_against_an_independent_float64_posterior(monkeypatch):
    """The end-to-end set-up of tests/test_gpu_flow_importance.py: one basic_ddm_dc data set of 12 trials whose posterior mean and sd an
    independent float64 importance sampler computed (tests/golden/flow_importance.npz), the proposal flow_importance_ref.proposal_flow,
    16 384 draws (the kernel's cap).  smooth=False launches what it launched before and nothing else; with smooth=True `raw` is that
    call bit for bit under the same seed, the smoothing kernel ran once and the weight-and-reduce kernel twice, the smoothed weighted
    means stay within that test's bound -- four Monte-Carlo standard errors, |mean - mean_ref| <= 4 sd_ref sqrt(1 / ESS + 1 / ESS_ref) with
    the smoothed weights' own ESS -- pareto_k is pareto_smooth's on the kept log_w and below the threshold, and the reference's summary is
    there."""
    import torch
    from flow_importance_ref import GOLDEN, mean_bound, proposal_flow
    from bayesflow_nddms_amd.amortizer import AmortizedPosterior, InvariantNetwork, pareto_smooth
    g = np.load(GOLDEN)
    S, probs = _cap(), (.005, .025, .5, .975, .995)
    am = AmortizedPosterior(proposal_flow(g["mean"], g["sd"]), InvariantNetwork()).cuda().eval()
    monkeypatch.setattr(am, "_conditions", lambda d: torch.zeros(1, 11, device="cuda"))
    conf = {"summary_conditions": torch.as_tensor(g["trials"], device="cuda")[None]}
    calls = _counted(monkeypatch, _lib())
    torch.manual_seed(7)
    old = am.posterior_importance(conf, S, probs=probs)
    assert calls == {"pareto": [], "importance": [(1, S, 5)], "wquantile": [(1, S, 5)]} and "pareto_k" not in old and "raw" not in old
    torch.manual_seed(7)
    new = am.posterior_importance(conf, S, probs=probs, smooth=True, keep_weights=True)
    assert calls == {"pareto": [(1, S, R.tail_size(S))], "importance": [(1, S, 5)] * 3, "wquantile": [(1, S, 5)] * 2}
    for k in ("mean", "std", "ess", "max_share", "log_evidence"):
        assert R.same_bits(new["raw"][k], old[k]), k
    sm = pareto_smooth(torch.as_tensor(new["log_w"], device="cuda"))
    assert R.same_bits(sm["pareto_k"].cpu().numpy(), new["pareto_k"]) and R.same_bits(sm["log_w"].cpu().numpy(), new["log_w_smoothed"])
    R.check({k: v.cpu().numpy() for k, v in sm.items()}, new["log_w"], "public")
    ess, ess_ref = float(new["ess"][0]), float(g["ess"])
    bound = mean_bound(g["sd"], ess, ess_ref)
    err, err_raw = np.abs(new["mean"][0] - g["mean"]), np.abs(old["mean"][0] - g["mean"])
    print("pareto_k", new["pareto_k"], "threshold", new["k_threshold"], "n_tail", new["n_tail"], "ess raw", old["ess"], "smoothed", new["ess"])
    print("smoothed |mean - ref| / bound", err / bound, "raw", err_raw / bound)
    assert int(new["n_nan"][0]) == 0 and ess >= 0.05 * S
    assert np.all(err <= bound), (err, bound)
    assert new["k_threshold"] == 0.7 and np.isfinite(new["pareto_k"][0]) and new["pareto_k"][0] < 0.7 and int(new["n_tail"][0]) == R.tail_size(S)
    for name in ("median", "95lower", "95upper", "99lower", "99upper"):
        assert new[name].shape == (1, 5) and np.isfinite(new[name]).all()
    assert np.all(new["99lower"] <= new["median"]) and np.all(new["median"] <= new["99upper"])


def test_public_path_takes_a_ragged_batch(monkeypatch):
    """observed_batch's input (12, 9 and 7 trials), 2000 draws, one launch and a launch per set: the smoothing kernel runs once per
    launch, `raw` is the smooth=False call's bits, and every set's pareto_k is pareto_smooth's on its own kept log weights."""
    import torch
    from test_gpu_flow_wquantile import _people
    from bayesflow_nddms_amd.amortizer import pareto_smooth
    B, S, P = 3, 2000, 5
    am, conf = _people(True)
    calls = _counted(monkeypatch, _lib())
    torch.manual_seed(21)
    old = am.posterior_importance(conf, S)
    assert not calls["pareto"] and calls["importance"] == [(B, S, P)]
    torch.manual_seed(21)
    new = am.posterior_importance(conf, S, smooth=True, keep_weights=True)
    assert calls["pareto"] == [(B, S, R.tail_size(S))] and len(calls["importance"]) == 3 and not calls["wquantile"]
    for k in ("mean", "std", "ess", "max_share", "log_evidence"):
        assert R.same_bits(new["raw"][k], old[k]), k
    sm = pareto_smooth(torch.as_tensor(new["log_w"], device="cuda"))
    assert R.same_bits(sm["pareto_k"].cpu().numpy(), new["pareto_k"]) and R.same_bits(sm["log_w"].cpu().numpy(), new["log_w_smoothed"])
    R.check({k: v.cpu().numpy() for k, v in sm.items()}, new["log_w"], "ragged")
    print("ragged: pareto_k", new["pareto_k"], "n_tail", new["n_tail"], "ess raw", old["ess"], "smoothed", new["ess"])
    n = len(calls["pareto"])
    split = am.posterior_importance(conf, S, smooth=True, z_bytes=1)
    assert calls["pareto"][n:] == [(1, S, R.tail_size(S))] * 3 and split["pareto_k"].shape == (B,)
