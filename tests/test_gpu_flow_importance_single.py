"""The single-trial model through the exact-posterior chain (AmortizedPosterior.posterior_importance / sample_exact with target=
single_trial_target(...)): the public path against its parts; the wiring -- log w + log q - log prior is the marginal likelihood --
against the independent float64 yardstick; a ragged batch of participants (counts to the kernel, padding never read); the scale model
(gamma the flow's 8th column); sample_exact; and the chain end to end against an independent float64 posterior under the restricted
prior (tests/flow_importance_single_ref.py, tests/golden/flow_importance_single.npz)."""
import math

import numpy as np
import pytest

import flow_importance_single_ref as F
import wiener_marginal_ref as M
from flow_importance_ref import mean_bound

pytestmark = pytest.mark.gpu

TC = 4.0                  # the simulators' default decision-time cap: max_steps 400 x dt .01
CENTRE = [0.0, 1.0, 0.5, 0.3, 1.0, 1.0, 1.5, 1.0]
WIDTH = [1.0, 0.3, 0.15, 0.1, 0.3, 0.3, 0.5, 0.3]


def _amortizer(P, centre=CENTRE, width=WIDTH):
    """An untrained flow centred on the prior (most draws inside its support), as tests/test_gpu_flow_importance.py::test_public_path's."""
    import torch
    from bayesflow_nddms_amd.amortizer import AmortizedPosterior, InvariantNetwork, InvertibleNetwork
    torch.manual_seed(0)
    am = AmortizedPosterior(InvertibleNetwork(num_params=P), InvariantNetwork()).cuda().eval()
    with torch.no_grad():
        w = torch.tensor(width[:P], device="cuda")
        am.inference_net.an_scale[0].copy_(-torch.log(w))
        am.inference_net.an_bias[0].copy_(-torch.tensor(centre[:P], device="cuda") / w)
    return am


def _conf(B):
    import torch
    from bayesflow_nddms_amd import single_trial_alpha_not_scaled as st
    torch.manual_seed(0)
    np.random.seed(2023)
    gm = st.make_generative_model(batched=True, device_prior=True, as_numpy=False)
    return st.configurator(gm(B))


def _parts(am, conf, r, model, S):
    """importance_weights on the call's own draws with the engine call's likelihood and the restricted prior's table."""
    import torch
    from bayesflow_nddms_amd import engine, priors
    from bayesflow_nddms_amd.amortizer import importance_weights
    draws, B = torch.as_tensor(r["draws"], device="cuda"), r["draws"].shape[0]
    data = torch.as_tensor(conf["summary_conditions"]).to("cuda", torch.float32)
    ll = engine.wiener_marginal_log_likelihood(engine.SINGLE_TRIAL, draws.view(B * S, -1), data, draws_per_dataset=S, t_censor=TC)["loglik"].view(B, S)
    return importance_weights(draws, torch.as_tensor(r["log_q"], device="cuda"), ll, priors.prior_table(priors.restricted_density(model)),
                              want_log_w=True)


def test_public_path():
    """keep_draws returns the draws of sample(fused=True) under the same seed, bit for bit; the numbers are importance_weights' on those
    draws with the engine call's likelihood and prior_table(restricted_density("single")); the result names its domain; the call without
    a target still refuses the model."""
    import torch
    from bayesflow_nddms_amd import priors
    from bayesflow_nddms_amd.amortizer import single_trial_target
    B, S, P = 2, 257, 7
    am, conf = _amortizer(P), _conf(B)
    tgt = single_trial_target(TC)
    torch.manual_seed(21)
    draws = am.sample(conf, S, fused=True, to_numpy=False)
    torch.manual_seed(21)
    r = am.posterior_importance(conf, S, target=tgt, keep_draws=True, keep_weights=True)
    assert r["n_samples"] == S and r["mean"].shape == (B, P) and r["std"].shape == (B, P) and r["draws"].dtype == np.float32
    assert r["domain"] == priors.MARGINAL_DOMAIN
    assert np.array_equal(r["draws"], draws.cpu().numpy()) and r["log_w"].shape == (B, S) and r["log_q"].shape == (B, S)
    w = _parts(am, conf, r, "single", S)
    for k in ("mean", "sd", "ess", "log_evidence", "max_share", "n_zero", "n_nan", "log_w"):
        assert np.array_equal(w[k].cpu().numpy(), r["std" if k == "sd" else k], equal_nan=True), k
    assert np.array_equal(r["n_zero"] + r["n_nan"], np.isneginf(r["log_w"]).sum(axis=1)) and not np.isnan(r["log_w"]).any()
    assert np.isfinite(r["log_evidence"]).all() and (r["ess"] >= 1.0).all()
    # a draw outside the restricted support has weight 0, whatever the unrestricted prior says
    lp = priors.log_prior_density(priors.restricted_density("single"), r["draws"].astype(np.float64))
    assert np.array_equal(np.isneginf(lp) | np.isneginf(r["log_w"]), np.isneginf(r["log_w"])) and (r["n_zero"] >= np.isneginf(lp).sum(axis=1)).all()
    print("public path: ess", r["ess"], "n_zero", r["n_zero"], "n_nan", r["n_nan"], "log evidence", r["log_evidence"])
    with pytest.raises(NotImplementedError, match="single_trial_logpdf"):
        am.posterior_importance(conf, S, model="single")


# the wiring test's data set: six responses on both boundaries and two timeouts, z1 around the boundary
WIRING_TRIALS = np.array([[0.71, 1.15], [-0.93, 1.32], [0.0, 1.4], [1.35, 0.9], [0.52, 1.05], [0.0, 1.1], [-0.64, 1.25], [0.88, 1.5]], np.float32)
WIRING_CENTRE = [1.0, 1.2, 0.5, 0.3, 0.3, 1.0, 0.5]
WIRING_WIDTH = [0.3, 0.1, 0.05, 0.03, 0.05, 0.1, 0.08]


def test_the_weights_hold_the_marginal_likelihood_of_the_float64_yardstick():
    """64 draws x 8 trials, two of them timeouts at t_censor = 4: log w + log q - log prior, the likelihood the weights were made of,
    against wiener_marginal_ref.log_lik summed over the trials.  Bound: n_trials x DEVICE_BAR["box"] (the kernel's wider bar per trial;
    a wiring error -- another set, a column shifted, gamma, t_censor, the prior -- is O(1)).  Rows the yardstick refuses ("not
    converged") are left out; CONDITION: at most 10 % of them (on the CPU the yardstick converged on all 64 rows of this narrow flow's
    draws under seeds 0, 1 and 2)."""
    import torch
    from bayesflow_nddms_amd import priors
    from bayesflow_nddms_amd.amortizer import single_trial_target
    S, P = 64, 7
    am = _amortizer(P, WIRING_CENTRE, WIRING_WIDTH)
    conf = {"summary_conditions": torch.as_tensor(WIRING_TRIALS)[None].cuda(), "direct_conditions": torch.full((1, 1), math.log(8.0), device="cuda")}
    torch.manual_seed(31)
    r = am.posterior_importance(conf, S, target=single_trial_target(TC), keep_draws=True, keep_weights=True)
    th = r["draws"][0].astype(np.float64)
    lp = priors.log_prior_density(priors.restricted_density("single"), th)
    assert int(r["n_nan"][0]) == 0 and int(r["n_zero"][0]) == 0 and np.all(np.isfinite(lp))
    got = r["log_w"][0] + r["log_q"][0].astype(np.float64) - lp
    ref = F.independent_rows(th, WIRING_TRIALS.astype(np.float64), t_censor=TC)
    conv = np.isfinite(ref).all(axis=1)
    err = np.abs(got[conv] - ref[conv].sum(axis=1))
    bound = WIRING_TRIALS.shape[0] * M.DEVICE_BAR["box"]
    print(f"wiring: {int(conv.sum())} of {S} rows converged, max |log lik - yardstick| = {err.max():.3g} (bound {bound:g}), log lik in "
          f"[{got.min():.1f}, {got.max():.1f}]")
    assert conv.mean() >= 0.9
    assert err.max() <= bound


def test_a_ragged_batch_gives_every_set_its_own_numbers(monkeypatch):
    """observed_batch of three participants with 5, 64 and 70 trials, one set per launch (a small z_bytes), the conditions fixed (the
    summary network is taken out of the comparison): every set's numbers are those of a B = 1 call on its own unpadded trials at the
    same place of the random stream, bit for bit; padding poisoned with NaN gives the same bits."""
    import torch
    from bayesflow_nddms_amd import single_trial_alpha_not_scaled as st
    from bayesflow_nddms_amd.amortizer import observed_batch, single_trial_target
    n, S, P = (5, 64, 70), 130, 7
    theta = np.array([[0.8, 1.2, 0.5, 0.3, 0.3, 1.0, 0.5], [-0.5, 1.0, 0.45, 0.25, 0.4, 0.9, 0.8], [1.5, 1.4, 0.55, 0.35, 0.2, 1.1, 0.3]], np.float32)
    sim = st.batch_simulate_trials(theta, 70, seed=2023, set_offset=0, with_summary=False)["sim_data"]
    sets = [np.asarray(sim[b, :k], dtype=np.float32) for b, k in enumerate(n)]
    am, tgt = _amortizer(P), single_trial_target(TC)
    ob = observed_batch(sets, device="cuda")
    assert ob["summary_counts"].tolist() == list(n) and ob["summary_conditions"].shape == (3, 70, 2)
    with torch.no_grad():
        cond_all = am._conditions(ob)
    monkeypatch.setattr(am, "_conditions", lambda d: cond_all[d["rows"]])
    keys = ("mean", "std", "ess", "log_evidence", "max_share", "n_zero", "n_nan", "draws", "log_q", "log_w")
    torch.manual_seed(22)
    split = am.posterior_importance(dict(ob, rows=slice(0, 3)), S, z_bytes=1, target=tgt, keep_draws=True, keep_weights=True)
    assert np.isfinite(split["log_evidence"]).all() and (split["ess"] >= 1.0).all()
    torch.manual_seed(22)
    for b, s in enumerate(sets):                                         # (the stream goes on where the call before left it)
        one = am.posterior_importance({"rows": slice(b, b + 1), "summary_conditions": torch.as_tensor(s, device="cuda")[None]}, S, target=tgt,
                                      keep_draws=True, keep_weights=True)
        for k in keys:
            assert np.array_equal(split[k][b], one[k][0], equal_nan=True), (b, k)
    poisoned = ob["summary_conditions"].clone()
    for b, k in enumerate(n):
        poisoned[b, k:] = float("nan")
    torch.manual_seed(22)
    again = am.posterior_importance(dict(ob, rows=slice(0, 3), summary_conditions=poisoned), S, z_bytes=1, target=tgt, keep_draws=True,
                                    keep_weights=True)
    for k in keys:
        assert np.array_equal(split[k], again[k], equal_nan=True), k
    # without the counts the padding is scored: zero rows are timeouts censored at t_censor to this model, not nothing
    torch.manual_seed(22)
    padded = am.posterior_importance({"rows": slice(0, 3), "summary_conditions": ob["summary_conditions"]}, S, z_bytes=1, target=tgt)
    assert not np.array_equal(padded["log_evidence"][:2], split["log_evidence"][:2]) and padded["log_evidence"][2] == split["log_evidence"][2]
    print("ragged: ess", split["ess"], "log evidence", split["log_evidence"])


def test_the_scale_model_takes_gamma_from_the_flow():
    import torch
    from bayesflow_nddms_amd import priors
    from bayesflow_nddms_amd.amortizer import single_trial_target
    B, S, P = 2, 130, 8
    am, conf = _amortizer(P), _conf(B)
    torch.manual_seed(23)
    r = am.posterior_importance(conf, S, target=single_trial_target(TC, gamma=None), keep_draws=True, keep_weights=True)
    assert r["draws"].shape == (B, S, P) and r["domain"] == priors.MARGINAL_DOMAIN and np.isfinite(r["log_evidence"]).all()
    w = _parts(am, conf, r, "scale", S)
    for k in ("mean", "sd", "ess", "log_evidence", "max_share", "n_zero", "n_nan", "log_w"):
        assert np.array_equal(w[k].cpu().numpy(), r["std" if k == "sd" else k], equal_nan=True), k
    with pytest.raises(ValueError, match="takes a flow of 7 parameters"):
        am.posterior_importance(conf, S, target=single_trial_target(TC))


def test_sample_exact_with_a_target():
    import torch
    from bayesflow_nddms_amd.amortizer import resample_draws, resample_words, single_trial_target
    B, n, P = 2, 300, 7
    am, conf, tgt = _amortizer(P), _conf(B), single_trial_target(TC)
    torch.manual_seed(24)
    got = am.sample_exact(conf, n, target=tgt, seed=9, to_numpy=False)
    assert torch.is_tensor(got) and got.is_cuda and got.shape == (B, n, P) and bool(torch.isfinite(got).all())
    assert set(am.last_exact) >= {"ess", "n_unique", "pareto_k", "k_threshold", "n_proposals"} and am.last_exact["n_proposals"] == n
    assert am.last_exact["ess"].shape == (B,) and am.last_exact["pareto_k"].shape == (B,)
    torch.manual_seed(24)
    r = am.posterior_importance(conf, n, target=tgt, smooth=True, keep_draws=True, keep_weights=True)
    ref = resample_draws(torch.as_tensor(r["draws"], device="cuda"), n, log_w=torch.as_tensor(r["log_w_smoothed"], device="cuda"),
                         words=resample_words(B, 9))
    assert torch.equal(got, ref["draws"]) and np.array_equal(am.last_exact["n_unique"], ref["n_unique"].cpu().numpy())
    torch.manual_seed(24)
    host = am.sample_exact(conf, n, target=tgt, seed=9)
    assert isinstance(host, np.ndarray) and np.array_equal(host, got.cpu().numpy())


def test_end_to_end_against_an_independent_float64_posterior():
    """One data set of 8 response-only trials (tests/golden/flow_importance_single.npz) whose posterior mean, sd and log evidence UNDER
    THE RESTRICTED PRIOR the committed script tests/flow_importance_single_ref.py computed in float64 by adaptive importance sampling
    (pilot from the prior, three rounds of a Student-t proposal; ess_ref = 3403 of 40 000; its likelihood re-scored with the independent
    yardstick on the 2000 heaviest and 500 random rows: 1.5e-8 apart per trial at most, none unconverged).  q is the script's
    proposal_flow: a near-identity 7-column flow 1.25 sd wide, half an sd off in the beta column; the base normals are the CPU generator's
    under PROPOSAL_SEED.  The public call: sampler with log q -> the ragged marginal kernel on the 7-column draws -> weight-and-reduce.
    CONDITION (fixture): ess_ref >= 2000.  CONDITION (device): ESS >= 2.5 % of the 20 000 draws; the script's check_proposal on the CPU
    gave 1469, 989 and 1017 over seeds 7, 8, 9 (at the basic model's width of 1.5 sd: 534, 544, 500 -- the width was narrowed, not the
    bar).  Bounds, four Monte-Carlo standard errors of the difference: per column |mean_dev - mean_ref| <= 4 sd_ref sqrt(1 / ESS_dev + 1 /
    ESS_ref); |log evidence_dev - log evidence_ref| <= 4 sqrt(1 / ESS_dev + 1 / ESS_ref).  The UNWEIGHTED mean of the same draws misses the
    first bound in the beta column (by a factor of 3.5 to 4 on the CPU): without the weights the test fails.  On one MI355X: ESS 1468.7,
    the seven weighted means within 0.48, 0.21, 0.55, 0.22, 0.47, 0.03, 0.38 of their bounds, the log evidence -20.1221 against -20.1161
    (bound 0.125), the unweighted mean 4.02 x its bound in beta."""
    import torch
    from bayesflow_nddms_amd.amortizer import AmortizedPosterior, InvariantNetwork, single_trial_target
    g = np.load(F.GOLDEN)
    assert float(g["ess_ref"]) >= F.ESS_REF_MIN and float(g["unconverged"]) <= 0.01 and float(g["scheme_max_diff"]) <= 1e-6
    assert not np.any(g["trials"][:, 0] == 0)
    am = AmortizedPosterior(F.proposal_flow(g["mean"], g["sd"]), InvariantNetwork()).cuda().eval()
    z = torch.randn(1, F.PROPOSAL_DRAWS, 7, generator=torch.Generator().manual_seed(F.PROPOSAL_SEED)).cuda()
    conf = {"summary_conditions": torch.as_tensor(g["trials"], device="cuda")[None],
            "direct_conditions": torch.full((1, 1), math.log(g["trials"].shape[0]), device="cuda")}
    real = torch.randn
    try:                                                                # the call's base normals: the ones the CPU check of the proposal saw
        torch.randn = lambda *a, **kw: z.view(-1, 7) if a == (F.PROPOSAL_DRAWS, 7) else real(*a, **kw)
        r = am.posterior_importance(conf, F.PROPOSAL_DRAWS, target=single_trial_target(float(g["t_censor"])), keep_draws=True)
    finally:
        torch.randn = real
    ess, ess_ref = float(r["ess"][0]), float(g["ess_ref"])
    print("ess", ess, "of", F.PROPOSAL_DRAWS, "n_zero", int(r["n_zero"][0]), "n_nan", int(r["n_nan"][0]), "max_share", float(r["max_share"][0]))
    assert int(r["n_nan"][0]) == 0
    assert ess >= F.ESS_DEV_MIN * F.PROPOSAL_DRAWS, ess
    bound = mean_bound(g["sd"], ess, ess_ref)
    err, err_plain = np.abs(r["mean"][0] - g["mean"]), np.abs(r["draws"][0].astype(np.float64).mean(axis=0) - g["mean"])
    print("weighted |mean - ref| / bound", err / bound, "unweighted", err_plain / bound)
    print("log evidence", float(r["log_evidence"][0]), "ref", float(g["log_evidence"]), "bound", 4.0 * math.sqrt(1.0 / ess + 1.0 / ess_ref))
    assert np.all(err <= bound), (err, bound)
    assert abs(float(r["log_evidence"][0]) - float(g["log_evidence"])) <= 4.0 * math.sqrt(1.0 / ess + 1.0 / ess_ref)
    assert np.any(err_plain > bound), (err_plain, bound)
