"""CPU tests of the single-trial model's importance target (amortizer.single_trial_target, posterior_importance(..., target=...)): the
restricted prior against scipy.stats, the target's and the engine's argument checks (every one before any device work), and the pins of
the call without a target."""
import numpy as np
import pytest
import torch


def test_restricted_prior_against_scipy():
    from scipy import stats
    from bayesflow_nddms_amd import priors
    assert priors.MARGINAL_DOMAIN == {"std_alpha": 0.02, "dc": 0.05, "sigma1": 0.02}
    for model, P in (("single", 7), ("scale", 8)):
        dens = priors.restricted_density(model)
        assert len(dens) == P and dens[:4] == priors.PRIOR_DENSITY[model][:4] and dens[7:] == priors.PRIOR_DENSITY[model][7:]
        assert dens[4] == ("truncnormal", 1.0, 0.5, 0.02, 3.0) and dens[5] == ("truncnormal", 1.0, 0.5, 0.05, 10.0) and dens[6] == ("uniform", 0.02, 5.0)
        table = priors.prior_table(dens)
        # the normalisers on the raised bounds
        for col, (mean, sd, lo, hi) in ((4, (1.0, 0.5, 0.02, 3.0)), (5, (1.0, 0.5, 0.05, 10.0))):
            mass = stats.norm.cdf((hi - mean) / sd) - stats.norm.cdf((lo - mean) / sd)
            assert table[col, 3] == lo and table[col, 4] == hi
            assert abs(table[col, 5] - (np.log(sd) + 0.5 * np.log(2 * np.pi) + np.log(mass))) <= 1e-14
        assert table[6, 3] == 0.02 and abs(table[6, 5] - np.log(5.0 - 0.02)) <= 1e-15
        # the density against scipy's truncnorm / uniform / beta / norm, inside
        rng = np.random.default_rng(P)
        th = np.stack([rng.normal(0, 2, 200), rng.uniform(0.1, 3, 200), rng.uniform(0.05, 0.95, 200), rng.uniform(0.01, 1.4, 200),
                       rng.uniform(0.02, 3, 200), rng.uniform(0.05, 4, 200), rng.uniform(0.02, 5, 200)] + ([rng.uniform(0, 2, 200)] if P == 8 else []), 1)
        tn = lambda x, m, s, lo, hi: stats.truncnorm.logpdf(x, (lo - m) / s, (hi - m) / s, loc=m, scale=s)      # noqa: E731
        ref = (stats.norm.logpdf(th[:, 0], 0, 2) + tn(th[:, 1], 1.0, 0.5, 0.0, 10.0) + stats.beta.logpdf(th[:, 2], 2, 2) + tn(th[:, 3], 0.5, 0.25, 0.0, 1.5)
               + tn(th[:, 4], 1.0, 0.5, 0.02, 3.0) + tn(th[:, 5], 1.0, 0.5, 0.05, 10.0) + stats.uniform.logpdf(th[:, 6], 0.02, 4.98)
               + (stats.uniform.logpdf(th[:, 7], 0, 2) if P == 8 else 0.0))
        got = priors.log_prior_density(dens, th)
        assert np.all(np.isfinite(got)) and np.max(np.abs(got - ref)) <= 1e-12
        # -inf below the raised bounds, finite at them; the unrestricted prior is finite there
        for col, low in ((4, 0.02), (5, 0.05), (6, 0.02)):
            x = th[:3].copy()
            x[:, col] = np.nextafter(low, 0.0)
            assert np.all(np.isneginf(priors.log_prior_density(dens, x))) and np.all(np.isfinite(priors.log_prior_density(model, x)))
            x[:, col] = low
            assert np.all(np.isfinite(priors.log_prior_density(dens, x)))
    # other bounds, and the refusals
    d = priors.restricted_density("single", {"dc": 0.2})
    assert d[5] == ("truncnormal", 1.0, 0.5, 0.2, 10.0) and d[4] == priors.PRIOR_DENSITY["single"][4]
    assert priors.restricted_density("single", {"dc": -1.0})[5] == priors.PRIOR_DENSITY["single"][5]      # never lowered
    with pytest.raises(ValueError, match="single-trial"):
        priors.restricted_density("basic")
    with pytest.raises(ValueError, match="std_alpha, dc and sigma1"):
        priors.restricted_density("single", {"beta": 0.1})
    with pytest.raises(ValueError, match="upper end"):
        priors.restricted_density("single", {"std_alpha": 3.0})


def _amortizer(P):
    from bayesflow_nddms_amd.amortizer import AmortizedPosterior, InvariantNetwork, InvertibleNetwork
    torch.manual_seed(0)
    return AmortizedPosterior(InvertibleNetwork(num_params=P), InvariantNetwork()).eval()


def test_target_validation():
    from bayesflow_nddms_amd import priors
    from bayesflow_nddms_amd.amortizer import single_trial_target
    t = single_trial_target(4.0)
    assert (t.t_censor, t.gamma, t.model, t.num_params) == (4.0, 1.0, "single", 7) and t.domain == priors.MARGINAL_DOMAIN
    assert t.density == priors.restricted_density("single")
    s = single_trial_target(None, gamma=None)
    assert (s.t_censor, s.gamma, s.model, s.num_params) == (0.0, None, "scale", 8) and s.density == priors.restricted_density("scale")
    assert single_trial_target(1.0, domain={"dc": 0.2}).density[5][3] == 0.2
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="t_censor"):
            single_trial_target(bad)
    with pytest.raises(ValueError, match="gamma"):
        single_trial_target(4.0, gamma=0.5)
    data = {"summary_conditions": torch.zeros(2, 9, 2), "direct_conditions": torch.full((2, 1), float(np.log(9.0)))}
    # the flow's width against gamma, the data's last dimension, the target's type: all before any device work
    with pytest.raises(ValueError, match="takes a flow of 7 parameters; this one has 8"):
        _amortizer(8).posterior_importance(data, 16, target=t)
    with pytest.raises(ValueError, match="takes a flow of 8 parameters; this one has 7"):
        _amortizer(7).posterior_importance(data, 16, target=s)
    with pytest.raises(ValueError, match="takes a flow of 7 parameters; this one has 5"):
        _amortizer(5).posterior_importance(data, 16, target=t)
    with pytest.raises(ValueError, match=r"\(choicert, z1\) trials \[B, N, 2\]"):
        _amortizer(7).posterior_importance(dict(data, summary_conditions=torch.zeros(2, 9, 3)), 16, target=t)
    with pytest.raises(TypeError, match="single_trial_target"):
        _amortizer(7).posterior_importance(data, 16, target="single")
    with pytest.raises(ValueError, match="contradicts"):
        _amortizer(7).posterior_importance(data, 16, model="scale", target=t)


def test_engine_refuses_host_counts_before_any_device_work(monkeypatch):
    from bayesflow_nddms_amd import engine
    monkeypatch.setattr(engine, "require_device", lambda: pytest.fail("device work before the host checks"))
    good = np.array([[0.8, 1.2, 0.45, 0.2, 0.5, 1.1, 0.7, 1.0]] * 2)
    data = np.tile(np.array([[[0.6, 1.0], [-0.7, 1.3], [0.9, 1.1]]]), (2, 1, 1))
    wl = lambda c: engine.wiener_marginal_log_likelihood(engine.SINGLE_TRIAL, good, data, t_censor=1.0, counts=c)      # noqa: E731
    for c in ([0, 3], [1, 4], [-1, 2], np.array([3, 0], np.int32), torch.tensor([4, 1])):
        with pytest.raises(ValueError, match=r"\[1, n_trials = 3\]"):
            wl(c)
    for c in ([1, 2, 3], [[1, 2]], [1.5, 2.0], 3):
        with pytest.raises(ValueError, match="counts must be integers"):
            wl(c)
    # host rows keep the one documented shape
    with pytest.raises(ValueError, match=r"\[R, 8\]"):
        engine.wiener_marginal_log_likelihood(engine.SINGLE_TRIAL, good[:, :7], data, counts=[1, 2])


def test_the_call_without_a_target_is_pinned_and_a_target_needs_the_device():
    from bayesflow_nddms_amd.amortizer import single_trial_target

    class Unread(dict):
        def __getitem__(self, k):
            raise AssertionError("the dict was read")
        get = __getitem__

    am = _amortizer(7)
    with pytest.raises(NotImplementedError, match="single_trial_logpdf"):
        am.posterior_importance(Unread(), 16, model="single")
    with pytest.raises(NotImplementedError, match="single_trial_logpdf"):
        am.posterior_importance(Unread(), 16, model="scale", probs=(.5,), smooth=True, resample=4)
    if not torch.cuda.is_available():
        data = {"summary_conditions": torch.zeros(1, 9, 2), "direct_conditions": torch.full((1, 1), float(np.log(9.0)))}
        with pytest.raises(RuntimeError, match="ROCm GPU|HIP library"):
            am.posterior_importance(data, 16, target=single_trial_target(4.0))
        with pytest.raises(RuntimeError, match="ROCm GPU|HIP library"):
            am.sample_exact(data, 16, target=single_trial_target(4.0))
