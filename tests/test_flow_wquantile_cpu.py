"""Weighted posterior quantiles (csrc/train_wquantile.hip, amortizer.py: quantize_weights / weighted_draw_quantiles /
posterior_importance(probs=...)) as far as a machine without a GPU can hold them: the library's exports and host refusals, and the
PyTorch evaluation of the definition -- the path every CPU tensor takes and the one the kernel is held to bit for bit
(tests/test_gpu_flow_wquantile.py) -- against tests/wquantile_ref.py's recomputation in Python integers (bit-equal), against
draw_quantiles at equal weights (bit-equal), and end to end against the independent float64 posterior of tests/flow_importance_ref.py."""
import ctypes
import math

import numpy as np
import pytest

from wquantile_ref import GOLDEN, ONE, bits, check, crafted_cases, quantize, reference, skewed_log_w

PROBS = (0.0, .005, .025, .1, 1.0 / 3.0, .5, .975, .995, 1.0)
DEFAULT = (.005, .025, .5, .975, .995)
NAMES = {.5: "median", .025: "95lower", .975: "95upper", .005: "99lower", .995: "99upper"}
OLD_KEYS = {"mean", "std", "ess", "log_evidence", "max_share", "n_zero", "n_nan", "n_samples"}


def _same(a, b):
    return all(np.array_equal(bits(a[k].numpy()), bits(b[k].numpy())) for k in ("quantiles", "order", "n_positive"))


def check_properties(res, theta, W):
    """p = 0 gives the smallest inside value and p = 1 the largest; the quantile does not decrease in p (PROBS ascends)."""
    q, o = res["quantiles"].cpu().numpy(), res["order"].cpu().numpy()
    inside = np.isfinite(theta).all(axis=-1) & (W >= 1)
    for b in range(theta.shape[0]):
        if inside[b].any():
            x = theta[b][inside[b]]
            assert np.array_equal(q[b, 0], x.min(axis=0).astype(np.float64)) and np.array_equal(q[b, -1], x.max(axis=0).astype(np.float64))
            assert np.array_equal(o[b, 0, 0], x.min(axis=0)) and np.array_equal(o[b, -1, 1], x.max(axis=0))
            assert np.all(np.diff(q[b], axis=0) >= 0)


@pytest.mark.parametrize("S", [1, 2, 3, 64, 65, 257, 1000])
def test_weighted_draw_quantiles_on_cpu_tensors(S):
    import torch
    from bayesflow_nddms_amd.amortizer import quantize_weights, weighted_draw_quantiles
    rng = np.random.default_rng(S)
    for D in (1, 5, 8):
        for scale in (1e-3, 1.0, 1e4):
            theta = (rng.normal(size=(2, S, D)) * scale).astype(np.float32)
            lw = skewed_log_w(rng, 2, S)
            res = weighted_draw_quantiles(torch.from_numpy(theta), PROBS, log_w=torch.from_numpy(lw), want_weights=True)
            assert all(not v.is_cuda for v in res.values())
            W = res["weights"].numpy()
            assert np.array_equal(W, quantize_weights(torch.from_numpy(lw)).numpy())
            check(res, theta, W, PROBS)
            check_properties(res, theta, W)
            again = weighted_draw_quantiles(torch.from_numpy(theta), PROBS, weights=torch.from_numpy(W))
            assert "weights" not in again and _same(res, again)
    one = weighted_draw_quantiles(torch.from_numpy(theta[0]), PROBS, log_w=torch.from_numpy(lw[0]))     # [S, D]: one set
    assert one["quantiles"].shape == (1, len(PROBS), 8) and torch.equal(one["quantiles"][0], res["quantiles"][0])


def test_quantize_weights_against_numpy():
    """The largest weight of a set is exactly 2^36, every weight within 1 of NumPy's (torch's exp against NumPy's), rows that are not
    finite weigh 0, and a set without a finite log weight is all zeros."""
    import torch
    from bayesflow_nddms_amd.amortizer import WEIGHT_ONE, quantize_weights
    assert WEIGHT_ONE == ONE
    rng = np.random.default_rng(5)
    lw = skewed_log_w(rng, 4, 3000)
    lw[1, 17], lw[1, 18], lw[2, 0] = np.nan, np.inf, np.nan
    lw[3] = -np.inf
    lw[3, ::3] = np.nan
    W, ref = quantize_weights(torch.from_numpy(lw)).numpy(), quantize(lw)
    assert W.dtype == np.int64 and W.shape == lw.shape
    assert W[:3].max(axis=1).tolist() == [ONE] * 3 and W.min() >= 0 and not W[3].any()
    assert not W[~np.isfinite(lw)].any() and np.abs(W - ref).max() <= 1
    assert np.array_equal(quantize_weights(torch.from_numpy(lw[0])).numpy(), W[0])
    assert np.array_equal(quantize_weights(torch.from_numpy(lw[:3].astype(np.float32))).numpy(), quantize(lw[:3].astype(np.float32)))


@pytest.mark.parametrize("S", [1, 2, 3, 64, 65, 1000, 10000])
def test_equal_weights_give_draw_quantiles_bits(S):
    import torch
    from bayesflow_nddms_amd.amortizer import draw_quantiles, weighted_draw_quantiles
    rng = np.random.default_rng(S)
    theta = rng.normal(size=(2, S, 3)).astype(np.float32)
    theta[0, 0, 1] = np.nan if S > 1 else 0.5
    t = torch.from_numpy(theta)
    plain = draw_quantiles(t, PROBS)
    for level in (0.0, -731.25):
        res = weighted_draw_quantiles(t, PROBS, log_w=torch.full((2, S), level, dtype=torch.float64))
        assert np.array_equal(bits(res["quantiles"].numpy()), bits(plain["quantiles"].numpy()))
        assert np.array_equal(bits(res["order"].numpy()), bits(plain["order"].numpy()))
        assert torch.equal(res["n_positive"], plain["n_inside"])


def test_zero_weight_rows_and_row_order_do_not_matter():
    """Deleting the rows of weight zero changes no bit; neither does permuting the rows of a set whose values are distinct."""
    import torch
    from bayesflow_nddms_amd.amortizer import weighted_draw_quantiles
    rng = np.random.default_rng(11)
    S, D = 500, 4
    theta = rng.normal(size=(1, S, D)).astype(np.float32)
    assert all(len(np.unique(theta[0, :, d])) == S for d in range(D))
    lw = skewed_log_w(rng, 1, S)
    lw[0, rng.random(S) < 0.3] = -np.inf
    W = quantize(lw)
    res = weighted_draw_quantiles(torch.from_numpy(theta), PROBS, weights=torch.from_numpy(W))
    keep = W[0] >= 1
    assert 0 < keep.sum() < S
    less = weighted_draw_quantiles(torch.from_numpy(theta[:, keep]), PROBS, weights=torch.from_numpy(W[:, keep]))
    perm = rng.permutation(S)
    mixed = weighted_draw_quantiles(torch.from_numpy(theta[:, perm]), PROBS, weights=torch.from_numpy(W[:, perm]))
    assert _same(res, less) and _same(res, mixed)


def check_crafted(name, res, theta, lw, W):
    """What each crafted case must show, beyond equality with the reference."""
    q, o, n = res["quantiles"].cpu().numpy(), res["order"].cpu().numpy(), res["n_positive"].cpu().numpy()
    if name == "ties with different weights":
        # tie order is visible: with the rows of a set reversed (ties then come in the other order) some quantile moves
        other = reference(theta[:, ::-1], W[:, ::-1], PROBS)[0]
        assert not np.array_equal(bits(other), bits(q))
    if name == "zeros":
        assert not np.signbit(o[o == 0]).any()
    if name == "nan / inf components":
        assert n.tolist() == [147, 149] and np.all(np.isfinite(q))
    if name == "log_w -inf, +inf, nan":
        assert n.tolist() == [66] and not W[0, [5, 6, 7, 69]].any() and W.max() == ONE
    if name == "all-zero sets":
        assert n.tolist() == [0, 0] and np.isnan(q).all() and np.isnan(o).all()
    if name == "one dominating weight":
        assert n.tolist() == [1, 1]
        for b, r in ((0, 41), (1, 199)):
            assert np.all(q[b] == theta[b, r].astype(np.float64)[None, :]) and np.all(o[b] == theta[b, r])
    if name == "weights over 2^30":
        assert W.min() == 2 ** 6 and W.max() == ONE


def test_crafted_rows():
    import torch
    from bayesflow_nddms_amd.amortizer import weighted_draw_quantiles
    for name, theta, lw in crafted_cases():
        res = weighted_draw_quantiles(torch.from_numpy(theta), PROBS, log_w=torch.from_numpy(lw), want_weights=True)
        W = res["weights"].numpy()
        assert np.abs(W - quantize(lw)).max() <= 1, name
        check(res, theta, W, PROBS)
        check_properties(res, theta, W)
        check_crafted(name, res, theta, lw, W)


def test_library_exports_the_entry_and_refuses_bad_arguments_on_the_host():
    """Called with null or dummy pointers, on the host: had the entry read or launched anything, this would not return."""
    from bayesflow_nddms_amd import _train_lib, build
    raw = ctypes.CDLL(build.build_train())
    assert hasattr(raw, "nddm_train_weighted_quantiles") and hasattr(raw, "nddm_train_weighted_quantiles_max_draws")
    L = _train_lib.lib()
    assert L is not None, "libnddm_train.so did not build / load"
    cap = L.nddm_train_weighted_quantiles_max_draws()
    assert cap == 16384
    good = (ctypes.c_double * 17)(*([0.5] * 17))
    buf = (ctypes.c_char * 64)()
    a = ctypes.addressof(buf)

    def rc(B=1, S=100, D=5, K=5, probs=ctypes.addressof(good), theta=a, log_w=a, w_in=None, quant=a):
        return L.nddm_train_weighted_quantiles(B, S, D, theta, log_w, w_in, probs, K, quant, None, None, None, None)

    assert rc(S=cap + 1) == 1 and rc(K=17) == 1 and rc(D=9) == 1
    assert rc(log_w=a, w_in=a) == 1 and rc(log_w=None, w_in=None) == 1
    for bad in (-0.1, 1.5, float("nan")):
        p = (ctypes.c_double * 5)(0.5, 0.5, bad, 0.5, 0.5)
        assert rc(probs=ctypes.addressof(p)) == 1 and rc(probs=ctypes.addressof(p), log_w=None, w_in=a) == 1, bad
    assert rc(B=0) == 1 and rc(S=0) == 1 and rc(D=0) == 1 and rc(K=0) == 1 and rc(probs=None) == 1
    assert rc(theta=None) == 1 and rc(quant=None) == 1


def test_python_validation():
    import torch
    from bayesflow_nddms_amd.amortizer import weighted_draw_quantiles
    th, lw, W = torch.zeros(2, 4, 3), torch.zeros(2, 4, dtype=torch.float64), torch.ones(2, 4, dtype=torch.int64)
    for kw in ({}, {"log_w": lw, "weights": W}):                                        # neither, both
        with pytest.raises(ValueError, match="exactly one"):
            weighted_draw_quantiles(th, [0.5], **kw)
    for probs in ([0.5, 2.0], [-0.1], [float("nan")], []):
        with pytest.raises(ValueError, match="probabilities"):
            weighted_draw_quantiles(th, probs, log_w=lw)
    with pytest.raises(ValueError):
        weighted_draw_quantiles(th, [0.5], log_w=lw[:, :3])
    with pytest.raises(ValueError):
        weighted_draw_quantiles(th, [0.5], weights=W[:1])
    with pytest.raises(ValueError, match="int64"):
        weighted_draw_quantiles(th, [0.5], weights=W.double())
    with pytest.raises(ValueError):
        weighted_draw_quantiles(torch.zeros(4), [0.5], log_w=lw)
    with pytest.raises(ValueError):
        weighted_draw_quantiles(torch.zeros(2, 0, 3), [0.5], log_w=torch.zeros(2, 0, dtype=torch.float64))


def _host_likelihood(monkeypatch):
    """engine.wiener_log_likelihood needs a device; on CPU tensors tests/wiener_ref.py's float64 density stands in for it."""
    import torch
    from bayesflow_nddms_amd import engine
    from flow_importance_ref import log_lik_basic

    def host(model, params, data, draws_per_dataset=1, device=None, **kw):
        assert model == engine.BASIC_DDM_DC and not params.is_cuda
        th, S = params.double().numpy(), draws_per_dataset
        ll = np.concatenate([log_lik_basic(th[b * S:(b + 1) * S], data[b].double().numpy()) for b in range(data.shape[0])])
        return {"loglik": torch.from_numpy(ll)}

    monkeypatch.setattr(engine, "wiener_log_likelihood", host)


def _small_amortizer(B, n=12, seed=0):
    """An untrained flow centred on basic_ddm_dc's prior (tests/test_gpu_flow_importance.py's), and B data sets of n trials."""
    import torch
    from flow_importance_ref import TRUE_PARAMS, simulate
    from bayesflow_nddms_amd.amortizer import AmortizedPosterior, InvariantNetwork, InvertibleNetwork
    torch.manual_seed(seed)
    am = AmortizedPosterior(InvertibleNetwork(num_params=5), InvariantNetwork()).eval()
    with torch.no_grad():
        width = torch.tensor([1.0, 0.3, 0.15, 0.1, 0.3])
        am.inference_net.an_scale[0].copy_(-torch.log(width))
        am.inference_net.an_bias[0].copy_(-torch.tensor([0.0, 1.0, 0.5, 0.3, 1.0]) / width)
    rng = np.random.default_rng(seed)
    trials = np.stack([simulate(TRUE_PARAMS, n, rng) for _ in range(B)]).astype(np.float32)
    assert np.all(trials[:, :, 1] != 0.0)
    return am, {"summary_conditions": torch.from_numpy(trials), "direct_conditions": torch.full((B, 1), float(np.log(n)))}


def test_posterior_importance_keys_and_quantiles_on_the_cpu(monkeypatch):
    """probs=None returns exactly the old keys; with probs every old number keeps its bits under the same seed, the quantiles are
    weighted_draw_quantiles' on the call's own draws and log weights, the named keys are the rows of `quantiles`, and two launches
    (z_bytes=1 ... one set each) consume the random stream as one set per call does."""
    import torch
    from bayesflow_nddms_amd.amortizer import weighted_draw_quantiles
    _host_likelihood(monkeypatch)
    B, S = 2, 300
    am, conf = _small_amortizer(B)
    torch.manual_seed(3)
    old = am.posterior_importance(conf, S)
    assert set(old) == OLD_KEYS
    torch.manual_seed(3)
    new = am.posterior_importance(conf, S, probs=DEFAULT, keep_draws=True, keep_weights=True)
    assert set(new) == OLD_KEYS | {"quantiles", "probs", "draws", "log_q", "log_w"} | set(NAMES.values())
    for k in OLD_KEYS - {"n_samples"}:
        assert np.array_equal(bits(old[k]), bits(new[k])), k
    assert new["quantiles"].shape == (B, 5, 5) and new["quantiles"].dtype == np.float64 and np.array_equal(new["probs"], np.asarray(DEFAULT))
    ref = weighted_draw_quantiles(torch.from_numpy(new["draws"]), DEFAULT, log_w=torch.from_numpy(new["log_w"]), want_weights=True)
    assert np.array_equal(bits(ref["quantiles"].numpy()), bits(new["quantiles"]))
    check(ref, new["draws"], ref["weights"].numpy(), DEFAULT)
    for k, p in enumerate(DEFAULT):
        assert np.array_equal(bits(new[NAMES[p]]), bits(new["quantiles"][:, k]))
    assert np.isfinite(new["quantiles"]).all() and int(ref["n_positive"].min()) > 10
    torch.manual_seed(3)
    part = am.posterior_importance(conf, S, probs=(.5, .1))
    assert "95lower" not in part and np.array_equal(bits(part["median"]), bits(new["median"])) and part["quantiles"].shape == (B, 2, 5)
    with pytest.raises(ValueError, match="probabilities"):
        am.posterior_importance(conf, S, probs=(.5, 1.5))
    with pytest.raises(NotImplementedError, match="single_trial_logpdf"):
        am.posterior_importance(conf, S, model="single", probs=DEFAULT)


def median_bound(sd_ref, ess_dev, ess_ref):
    """4 standard errors of the difference of two weighted medians, each 1.2533 sd / sqrt(ESS): the normal-theory standard error of a
    median, and the factor tests/flow_importance_ref.py::mean_bound uses."""
    return 4.0 * 1.2533 * np.asarray(sd_ref) * np.sqrt(1.0 / ess_dev + 1.0 / ess_ref)


def test_end_to_end_against_an_independent_float64_posterior():
    """The setting of tests/test_gpu_flow_importance.py's end-to-end test on the CPU path: the data set and the prior-proposal
    posterior of tests/flow_importance_ref.py (tests/golden/flow_importance.npz), whose weighted median tests/wquantile_ref.py computed
    from the same 1 000 000 prior draws (tests/golden/flow_wquantile.npz); q is proposal_flow, half an sd off in beta; the draws are the
    CPU generator's under PROPOSAL_SEED.  Per column |median_dev - median_ref| <= 4 sqrt(se_ref^2 + se_dev^2) with se = 1.2533 sd / sqrt(ESS).
    The UNWEIGHTED median of the same draws misses that bound in the beta column: without the weights the test fails."""
    import torch
    from flow_importance_ref import GOLDEN as GOLDEN_IS, PROPOSAL_DRAWS, PROPOSAL_SEED, log_lik_basic, proposal_flow
    from bayesflow_nddms_amd.amortizer import draw_quantiles, importance_weights, weighted_draw_quantiles
    g, gq = np.load(GOLDEN_IS), np.load(GOLDEN)
    assert np.allclose(g["mean"], gq["mean"], rtol=1e-9, atol=0) and np.isclose(float(g["ess"]), float(gq["ess"]), rtol=1e-9)      # the same yardstick
    net = proposal_flow(g["mean"], g["sd"])
    z = torch.randn(1, PROPOSAL_DRAWS, 5, generator=torch.Generator().manual_seed(PROPOSAL_SEED))
    with torch.no_grad():
        th, lq = net.inverse_per_set(z, torch.zeros(1, 11), log_density=True)
    ll = log_lik_basic(th[0].double().numpy(), g["trials"].astype(np.float64))
    w = importance_weights(th, lq, torch.as_tensor(ll)[None], "basic", want_log_w=True)
    ess, ess_ref = float(w["ess"][0]), float(g["ess"])
    med = weighted_draw_quantiles(th, (.5,), log_w=w["log_w"])["quantiles"][0, 0].numpy()
    plain = draw_quantiles(th, (.5,))["quantiles"][0, 0].numpy()
    bound = median_bound(g["sd"], ess, ess_ref)
    err, err_plain = np.abs(med - gq["median"]), np.abs(plain - gq["median"])
    print("ess", ess, "ref", ess_ref, "weighted |median - ref| / bound", err / bound, "unweighted", err_plain / bound)
    assert ess >= 0.05 * PROPOSAL_DRAWS
    assert np.all(err <= bound), (err, bound)
    assert err_plain[2] > bound[2], (err_plain, bound)
    assert math.isfinite(float(w["log_evidence"][0]))
