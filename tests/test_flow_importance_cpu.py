"""Importance weights of the amortizer's draws, the host side (no GPU): the flow's log density out of the PyTorch inverse
(InvertibleNetwork.inverse_with_log_density) against a float64 copy of the same network, the prior densities
(priors.log_prior_density, priors.prior_table) against scipy.stats column by column, and the torch evaluation of
amortizer.importance_weights against a NumPy recomputation on inputs that hold every special row of its rule."""
import copy
import math

import numpy as np
import pytest

from flow_importance_ref import numpy_importance, special_inputs


def _net(D, C, layers):
    import torch
    from bayesflow_nddms_amd.amortizer import InvertibleNetwork
    torch.manual_seed(layers)
    net = InvertibleNetwork(num_params=D, cond_dim=C, num_coupling_layers=layers, seed=layers).eval()
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(1.5)
        for p in list(net.an_scale) + list(net.an_bias):
            p.copy_(0.3 * torch.randn_like(p))
    return net


@pytest.mark.parametrize("layers,D,C", [(1, 2, 1), (6, 5, 11), (3, 8, 4)])
def test_inverse_with_log_density_against_float64(layers, D, C):
    """theta is `inverse`'s, bit for bit; log_q = -|z|^2 / 2 - (D / 2) log 2 pi + log|det| with log|det| from the float64 FORWARD at the
    float64 inverse of the same z (the identity: the forward's log-scales are the inverse's).  In float64 the two agree to round-off
    (1e-10); the float32 composition agrees with float64 to float32 round-off of a sum of 2 L D terms of size <= clamp (1e-3 relative
    to the magnitude 1 + |log_q| is 1000 x that)."""
    import torch
    net = _net(D, C, layers)
    net64 = copy.deepcopy(net).double()
    torch.manual_seed(11)
    z, cond = torch.randn(40, D), torch.randn(40, C)
    with torch.no_grad():
        theta, lq = net.inverse_with_log_density(z, cond)
        assert torch.equal(theta, net.inverse(z, cond)) and lq.shape == (40,) and lq.dtype == torch.float32
        th64, lq64 = net64.inverse_with_log_density(z.double(), cond.double())
        z_back, log_det = net64(th64, cond.double())
    ref = -0.5 * (z.double() ** 2).sum(-1) - 0.5 * D * math.log(2.0 * math.pi) + log_det
    assert float((z_back - z.double()).abs().max()) < 1e-9
    assert float((lq64 - ref).abs().max()) < 1e-10 * (1.0 + float(ref.abs().max()))
    assert float((lq.double() - ref).abs().max()) < 1e-3 * (1.0 + float(ref.abs().max()))


def test_inverse_per_set_log_density_is_the_composition_on_expanded_rows():
    import torch
    net = _net(5, 11, 2)
    torch.manual_seed(12)
    z, cond = torch.randn(3, 7, 5), torch.randn(3, 11)
    with torch.no_grad():
        th, lq = net.inverse_per_set(z, cond, log_density=True)
        th2, lq2 = net.inverse_with_log_density(z.reshape(21, 5), cond.repeat_interleave(7, dim=0))
        assert torch.equal(th, net.inverse_per_set(z, cond))
    assert th.shape == (3, 7, 5) and lq.shape == (3, 7)
    assert torch.equal(th.reshape(21, 5), th2) and torch.equal(lq.reshape(21), lq2)


def _scipy_columns(model):
    from scipy import stats
    tn = lambda m, s, lo, hi: stats.truncnorm((lo - m) / s, (hi - m) / s, loc=m, scale=s)      # noqa: E731
    basic = [stats.norm(0.0, 2.0), tn(1.0, .5, 0.0, 10.0), stats.beta(2.0, 2.0), tn(.5, .25, 0.0, 1.5), tn(1.0, .5, 0.0, 10.0)]
    single = basic[:4] + [tn(1.0, .5, 0.0, 3.0), tn(1.0, .5, 0.0, 10.0), stats.uniform(0.0, 5.0)]
    return {"basic": basic, "single": single, "scale": single + [stats.uniform(0.0, 2.0)]}[model]


@pytest.mark.parametrize("model", ["basic", "single", "scale"])
def test_log_prior_density_against_scipy(model):
    """Column by column against scipy.stats' logpdf on the prior's own draws (relative 1e-12), at both edges of every support (scipy's
    value there: finite for the truncated normals and the uniforms, -inf for Beta(2, 2)), and one point outside each support, a NaN
    and an inf (-inf); the table has one row per column."""
    from bayesflow_nddms_amd import priors
    cols = _scipy_columns(model)
    P = len(cols)
    table = priors.prior_table(model)
    assert table.shape == (P, 6) and table.dtype == np.float64
    inside = (priors.basic_prior_matrix(200) if model == "basic" else priors.single_prior_matrix(200)[:, :P]).astype(np.float64)
    if model == "scale":
        inside[:, 7] = np.random.default_rng(3).uniform(0.0, 2.0, 200)
    got = priors.log_prior_density(model, inside)
    ref = sum(c.logpdf(inside[:, d]) for d, c in enumerate(cols))
    assert got.shape == (200,) and np.all(np.isfinite(got))
    assert np.all(np.abs(got - ref) <= 1e-12 * (1.0 + np.abs(ref)))
    mid = inside[0]
    for d, c in enumerate(cols):
        lo, hi = c.support()
        pts = [v for v in (lo, hi) if np.isfinite(v)]
        outside = [v for v in (lo - 1e-9, hi + 1e-9) if np.isfinite(v)] + [np.nan, np.inf, -np.inf]
        for v in pts + outside:
            th = mid.copy()
            th[d] = v
            want = sum(cc.logpdf(th[k]) for k, cc in enumerate(cols)) if v in pts else -np.inf
            g = priors.log_prior_density(model, th)
            assert (g == want) if np.isinf(want) else abs(g - want) <= 1e-12 * (1.0 + abs(want)), (model, d, v, g, want)
    # the one-column description form, with the kinds no model above uses at these values
    assert priors.log_prior_density([("fixed", 1.0)], np.array([[1.0], [1.5]])).tolist() == [0.0, -np.inf]
    assert priors.log_prior_density([("beta", 1.0, 3.0)], np.array([[0.0]]))[0] == pytest.approx(math.log(3.0), abs=1e-14)


def test_torch_fallback_against_numpy():
    """The torch float64 evaluation of importance_weights on the special rows: the counts are equal as integers and land where the
    rule says; log_w equal where finite to 1e-13 relative and -inf at the same rows; every reduced number within 1e-11 relative (S =
    300 float64 terms, either order: S 2^-52 = 7e-14 of sum|terms|); the all-zero set has nan moments, ess 0 and log_evidence -inf;
    the dominated set neither overflows nor underflows: ess and max_share within e^-40 of 1."""
    import torch
    from bayesflow_nddms_amd.amortizer import importance_weights
    S = 300
    theta, log_q, log_lik = special_inputs(S)
    ref = numpy_importance(theta, log_q, log_lik)
    got = importance_weights(torch.as_tensor(theta), torch.as_tensor(log_q), torch.as_tensor(log_lik), "basic", want_log_w=True)
    got = {k: v.numpy() for k, v in got.items()}
    assert set(got) == set(ref)
    assert got["n_zero"].tolist() == ref["n_zero"].tolist() and got["n_nan"].tolist() == ref["n_nan"].tolist()
    assert got["n_nan"].tolist() == [2, 0, 0] and got["n_zero"].tolist() == [3, S, 0]
    lw = got["log_w"]
    assert np.isneginf(lw[0, [3, 5, 7, 9, 11]]).all() and np.isneginf(lw[1]).all() and np.isfinite(lw[2]).all()
    assert np.array_equal(np.isneginf(lw), np.isneginf(ref["log_w"]))
    fin = np.isfinite(lw)
    assert np.all(np.abs(lw[fin] - ref["log_w"][fin]) <= 1e-13 * np.abs(ref["log_w"][fin]))
    for k in ("log_evidence", "ess", "max_share", "mean", "sd"):
        g, r = got[k], ref[k]
        assert np.array_equal(np.isnan(g), np.isnan(r)), k
        ok = np.isfinite(r)
        assert np.array_equal(g[~ok & ~np.isnan(r)], r[~ok & ~np.isnan(r)]), k
        assert np.all(np.abs(g[ok] - r[ok]) <= 1e-11 * (1.0 + np.abs(r[ok]))), (k, g, r)
    assert np.isnan(got["mean"][1]).all() and np.isnan(got["sd"][1]).all() and got["ess"][1] == 0.0 and np.isneginf(got["log_evidence"][1])
    assert np.isfinite(got["log_evidence"][2]) and got["log_evidence"][2] < -600.0
    assert abs(got["ess"][2] - 1.0) < S * math.exp(-40.0) and abs(got["max_share"][2] - 1.0) < S * math.exp(-40.0)
    buf = torch.empty(3, 5, dtype=torch.float64)
    again = importance_weights(torch.as_tensor(theta), torch.as_tensor(log_q), torch.as_tensor(log_lik), "basic", out={"mean": buf})
    assert again["mean"] is buf and np.array_equal(buf.numpy(), got["mean"], equal_nan=True)
    # one set as [S, D]
    one = importance_weights(torch.as_tensor(theta[0]), torch.as_tensor(log_q[0]), torch.as_tensor(log_lik[0]), "basic")
    assert one["mean"].shape == (1, 5) and "log_w" not in one and np.array_equal(one["mean"].numpy()[0], got["mean"][0])


def test_posterior_importance_refuses_the_models_it_has_no_likelihood_for():
    from bayesflow_nddms_amd.amortizer import AmortizedPosterior, InvariantNetwork, InvertibleNetwork
    am = AmortizedPosterior(InvertibleNetwork(num_params=7), InvariantNetwork())
    with pytest.raises(NotImplementedError, match="single_trial_logpdf"):
        am.posterior_importance({}, 10, model="single")


def test_log_posterior_is_the_forward_density():
    """log_posterior on [B, P] and on [B, S, P] parameters: the forward's -|z|^2 / 2 - (P / 2) log 2 pi + log|det|, and on the draws of
    inverse_per_set(log_density=True) the density those came with, to float32 round-off."""
    import torch
    from bayesflow_nddms_amd.amortizer import AmortizedPosterior, InvariantNetwork, InvertibleNetwork
    torch.manual_seed(4)
    am = AmortizedPosterior(InvertibleNetwork(num_params=5), InvariantNetwork()).eval()
    conf = {"summary_conditions": torch.randn(2, 30, 2), "direct_conditions": torch.full((2, 1), math.log(30.0))}
    with torch.no_grad():
        cond = am._conditions(conf)
        th, lq = am.inference_net.inverse_per_set(torch.randn(2, 9, 5), cond, log_density=True)
        z, ld = am.inference_net(th[:, 0], cond)
    a = am.log_posterior(dict(conf, parameters=th[:, 0]))
    b = am.log_posterior(dict(conf, parameters=th))
    assert isinstance(a, np.ndarray) and a.shape == (2,) and b.shape == (2, 9)
    assert np.allclose(a, (-0.5 * (z ** 2).sum(-1) - 2.5 * math.log(2.0 * math.pi) + ld).numpy(), rtol=0, atol=1e-6)
    assert np.allclose(b, lq.numpy(), rtol=0, atol=1e-4 * (1.0 + float(lq.abs().max())))
