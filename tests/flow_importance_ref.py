"""Yardsticks of the importance-weight tests (tests/test_flow_importance_cpu.py, tests/test_gpu_flow_importance.py).  Test
infrastructure only: nothing in the product imports it.

  special_inputs, numpy_importance   inputs that hold every special row of amortizer.importance_weights' rule, and the rule itself
                                     in NumPy float64
  log_lik_basic                      basic_ddm_dc's exact log-likelihood of a data set at parameter rows, from tests/wiener_ref.py
  python tests/flow_importance_ref.py   writes tests/golden/flow_importance.npz: ONE basic_ddm_dc data set of 12 trials simulated at
                                     [1.0, 1.2, 0.5, 0.3, 1.0] (the model's Euler scheme in NumPy, dt = 0.01) and its posterior mean, sd
                                     and log evidence under the model's own prior by self-normalised importance sampling FROM THE PRIOR
                                     in float64 (N_REF draws), with that estimate's own effective sample size.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "flow_importance.npz")
TRUE_PARAMS = (1.0, 1.2, 0.5, 0.3, 1.0)
N_TRIALS, N_REF = 12, 1_000_000


def special_inputs(S, D=5, seed=0):
    """theta [3, S, D] float32 inside basic_ddm_dc's support, log_q [3, S] float32, log_lik [3, S] float64 with the special rows of the
    weight rule: set 0 -- a -inf likelihood (row 3), a NaN likelihood with a finite prior (row 5), a draw outside the support with a NaN
    likelihood (row 7), a NaN log_q (row 9), a non-finite draw (row 11); set 1 -- every weight zero (half by a -inf likelihood, half
    outside the support with a finite one); set 2 -- one weight dominating by more than e^50 on top of likelihoods near -745 (exp of
    any of them alone is a denormal or 0)."""
    from bayesflow_nddms_amd import priors
    rng = np.random.default_rng(seed)
    theta = np.stack([priors.basic_prior_matrix(S, seed=seed + b) for b in range(3)])[:, :, :D].astype(np.float32)
    log_q = rng.normal(-3.0, 1.0, (3, S)).astype(np.float32)
    log_lik = rng.normal(-20.0, 2.0, (3, S))
    log_lik[0, 3] = -np.inf
    log_lik[0, 5] = np.nan
    log_lik[0, 7], theta[0, 7, 1] = np.nan, -0.25
    log_q[0, 9] = np.nan
    theta[0, 11, 0] = np.inf
    log_lik[1] = -np.inf
    log_lik[1, ::2], theta[1, ::2, 2] = 1.0, 1.5
    log_lik[2] = rng.normal(-745.0, 1.0, S)
    log_lik[2, S // 2] += 80.0
    return theta, log_q, log_lik


def numpy_importance(theta, log_q, log_lik, model="basic"):
    """amortizer.importance_weights' definition in NumPy float64, sets one at a time -> the same keys, "log_w" included."""
    from bayesflow_nddms_amd import priors
    out = {k: [] for k in ("log_evidence", "ess", "max_share", "mean", "sd", "n_zero", "n_nan", "log_w")}
    for th, lq, ll in zip(np.asarray(theta, np.float64), np.asarray(log_q, np.float64), np.asarray(log_lik, np.float64)):
        lp = priors.log_prior_density(model, th)
        with np.errstate(all="ignore"):
            lw = ll + lp - lq
        zero_prior = np.isneginf(lp)
        nan = ~zero_prior & (np.isnan(ll) | np.isnan(lq))
        nan |= ~zero_prior & ~nan & ~np.isneginf(ll) & (np.isnan(lw) | np.isposinf(lw))
        lw = np.where(zero_prior | nan | np.isneginf(ll), -np.inf, lw)
        S, m = len(lw), lw.max()
        pos = np.isfinite(lw)
        u = np.zeros(S)
        u[pos] = np.exp(lw[pos] - m)
        sw, ok = u.sum(), bool(pos.any())
        with np.errstate(all="ignore"):
            mean = (u[pos, None] * th[pos]).sum(0) / sw
            var = (u[pos, None] * th[pos] ** 2).sum(0) / sw - mean * mean
            out["log_evidence"].append(m + np.log(sw / S) if ok else -np.inf)
            out["ess"].append(sw * sw / (u * u).sum() if ok else 0.0)
            out["max_share"].append(1.0 / sw if ok else np.nan)
        out["mean"].append(mean if ok else np.full(th.shape[1], np.nan))
        out["sd"].append(np.sqrt(np.maximum(var, 0.0)) if ok else np.full(th.shape[1], np.nan))
        out["n_zero"].append(int((np.isneginf(lw) & ~nan).sum()))
        out["n_nan"].append(int(nan.sum()))
        out["log_w"].append(lw)
    return {k: np.asarray(v) for k, v in out.items()}


def log_lik_basic(theta, trials, chunk=4000):
    """log p(trials | theta) of basic_ddm_dc, float64: theta [R, 5] = drift, boundary, beta, tau, dc; trials [N, 2] = (rt, choice +-1) ->
    [R].  -inf where a trial's rt <= tau; rows outside the parameters' domain (boundary, dc <= 0, beta outside (0, 1)) give NaN."""
    import wiener_ref as W
    theta, trials = np.asarray(theta, np.float64), np.asarray(trials, np.float64)
    out = np.empty(theta.shape[0])
    rt, up = trials[None, :, 0], trials[None, :, 1] > 0
    for i in range(0, theta.shape[0], chunk):
        v, a, w, tau, s = (theta[i:i + chunk, k][:, None] for k in range(5))
        bad = ((a <= 0) | (s <= 0) | (w <= 0) | (w >= 1))[:, 0]
        t = rt - tau
        ok = (t > 0) & ~bad[:, None]
        with np.errstate(all="ignore"):
            lf = W.log_f(np.where(ok, t, 1.0), up, np.where(bad[:, None], 1.0, a), v, np.where(bad[:, None], 0.5, w), np.where(bad[:, None], 1.0, s))
        ll = np.where(ok, lf, -np.inf).sum(axis=1)
        out[i:i + chunk] = np.where(bad, np.nan, ll)
    return out


def simulate(params, n, rng, dt=0.01, max_steps=400):
    """basic_ddm_dc's trial loop: evidence from beta * boundary, + drift dt + dc sqrt(dt) N(0, 1) per step until it leaves (0, boundary);
    rt = steps * dt + tau, choice +1 at the upper boundary and -1 at the lower."""
    drift, boundary, beta, tau, dc = params
    out = np.zeros((n, 2))
    for i in range(n):
        x, k = beta * boundary, 0
        while 0.0 < x < boundary and k < max_steps:
            x += drift * dt + dc * np.sqrt(dt) * rng.standard_normal()
            k += 1
        out[i] = (k * dt + tau, 1.0 if x >= boundary else -1.0 if x <= 0.0 else 0.0)
    return out


def posterior_from_the_prior(trials, n=N_REF, seed=2):
    """Self-normalised importance sampling with the prior as the proposal (weight = likelihood): -> mean [5], sd [5], log_evidence, ess."""
    from bayesflow_nddms_amd import priors
    theta = priors.basic_prior_matrix(n, seed=seed).astype(np.float64)
    ll = np.full(n, -np.inf)
    live = theta[:, 3] < trials[:, 0].min()                   # (elsewhere a trial lies at or before tau: likelihood 0)
    ll[live] = log_lik_basic(theta[live], trials)
    m = ll.max()
    u = np.exp(ll - m)
    sw = u.sum()
    mean = (u[:, None] * theta).sum(0) / sw
    sd = np.sqrt((u[:, None] * theta ** 2).sum(0) / sw - mean ** 2)
    return mean, sd, m + np.log(sw / n), sw * sw / (u * u).sum()


PROPOSAL_SHIFT, PROPOSAL_WIDTH, PROPOSAL_SEED, PROPOSAL_DRAWS = (0.0, 0.0, 0.5, 0.0, 0.0), 1.5, 7, 20_000


def proposal_flow(mean, sd):
    """The end-to-end test's proposal q, a wide Gaussian-like flow without any training: the default InvertibleNetwork (6 layers, D = 5,
    C = 11) with its coupling weights scaled by 0.01 -- a near-identity -- and the first ActNorm (the last step of the inverse) set so
    that theta = centre + PROPOSAL_WIDTH sd u for the inverse's u: centre = the yardstick's mean + PROPOSAL_SHIFT sd, half an sd off in the beta column (a
    proposal centred ON the posterior mean would give an unweighted mean the weights have nothing to correct; half an sd off in
    every column left an effective size of 450 .. 820 of 20 000 over four seeds, in this one column 1250 .. 1280)."""
    import torch
    from bayesflow_nddms_amd.amortizer import InvertibleNetwork
    with torch.random.fork_rng(devices=[]):                   # (the weights' initialisation draws from the global CPU generator)
        torch.manual_seed(0)
        net = InvertibleNetwork(num_params=5).eval()
    width =PROPOSAL_WIDTH * np.asarray(sd, np.float64)
    centre = np.asarray(mean, np.float64) + np.asarray(PROPOSAL_SHIFT) * np.asarray(sd, np.float64)
    with torch.no_grad():
        for layer in net.layers:
            for p in layer.parameters():
                p.mul_(0.01)
        net.an_scale[0].copy_(torch.as_tensor(-np.log(width), dtype=torch.float32))
        net.an_bias[0].copy_(torch.as_tensor(-centre / width, dtype=torch.float32))
    return net


def mean_bound(sd_ref, ess_dev, ess_ref):
    """4 Monte-Carlo standard errors of the difference of two self-normalised estimates of a posterior mean."""
    return 4.0 * np.asarray(sd_ref) * np.sqrt(1.0 / ess_dev + 1.0 / ess_ref)


def check_proposal():
    """On the CPU, through importance_weights' torch evaluation with tests/wiener_ref.py as the likelihood: the proposal's ESS at
    PROPOSAL_DRAWS draws, the weighted and the unweighted mean against the yardstick's bound."""
    import torch
    from bayesflow_nddms_amd.amortizer import importance_weights
    g = np.load(GOLDEN)
    net = proposal_flow(g["mean"], g["sd"])
    z = torch.randn(1, PROPOSAL_DRAWS, 5, generator=torch.Generator().manual_seed(PROPOSAL_SEED))
    with torch.no_grad():
        th, lq = net.inverse_per_set(z, torch.zeros(1, 11), log_density=True)
    ll = log_lik_basic(th[0].double().numpy(), g["trials"].astype(np.float64))
    w = importance_weights(th, lq, torch.as_tensor(ll)[None], "basic")
    ess = float(w["ess"][0])
    bound = mean_bound(g["sd"], ess, float(g["ess"]))
    print("ess", ess, "n_zero", int(w["n_zero"][0]), "n_nan", int(w["n_nan"][0]), "log evidence", float(w["log_evidence"][0]), "ref", float(g["log_evidence"]),
          "bound", 4.0 * np.sqrt(1.0 / ess + 1.0 / float(g["ess"])))
    print("weighted   |mean - ref| / bound", np.abs(w["mean"][0].numpy() - g["mean"]) / bound)
    print("unweighted |mean - ref| / bound", np.abs(th[0].double().mean(0).numpy() - g["mean"]) / bound)


def main():
    sys.path.insert(0, os.path.dirname(HERE))
    trials = simulate(TRUE_PARAMS, N_TRIALS, np.random.default_rng(2023)).astype(np.float32).astype(np.float64)      # (as stored)
    assert np.all(trials[:, 1] != 0.0)
    mean, sd, log_ev, ess = posterior_from_the_prior(trials)
    print("trials", trials.tolist(), "\nmean", mean, "\nsd", sd, "\nlog evidence", log_ev, "ess", ess, "of", N_REF)
    np.savez(GOLDEN, trials=trials.astype(np.float32), true_params=np.asarray(TRUE_PARAMS), mean=mean, sd=sd, log_evidence=log_ev, ess=ess,
             n_ref=N_REF)


if __name__ == "__main__":
    main()
