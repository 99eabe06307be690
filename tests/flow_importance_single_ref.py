"""Yardstick of the single-trial model's importance-weight tests (tests/test_gpu_flow_importance_single.py).  Test infrastructure only:
nothing in the product imports it.

  set_log_lik                        the marginal log-likelihood of one data set at parameter rows [R, 7] (gamma = 1), float64: the shipped
                                     quadrature's float64 restatement (wiener_marginal_ref.scheme_log_lik) summed over the trials
  python tests/flow_importance_single_ref.py   writes tests/golden/flow_importance_single.npz: ONE data set of 8 response-only trials
                                     simulated at (1.0, 1.2, 0.5, 0.3, 0.3, 1.0, 0.5), gamma 1 (Euler-Maruyama at 1 ms in NumPy), and its
                                     posterior mean, sd and log evidence under the RESTRICTED prior (priors.restricted_density("single"))
                                     by adaptive importance sampling in float64: a pilot drawn from the prior, then ROUNDS rounds of a
                                     multivariate Student-t proposal (df 5, covariance 1.5 x the previous round's weighted covariance), the
                                     last with N_FINAL draws.  The heaviest 2000 and 500 random rows of the last round are scored again with
                                     the independent yardstick (wiener_marginal_ref.log_lik) and must agree to 1e-6 per trial; rows it does
                                     not converge on are reported and capped at 1 %.  No timeouts: the yardstick's survival does not converge
                                     at strong drift.  Then check_proposal: the device test's proposal on the CPU over three seeds.
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLDEN = os.path.join(HERE, "golden", "flow_importance_single.npz")
TRUE_PARAMS = (1.0, 1.2, 0.5, 0.3, 0.3, 1.0, 0.5)
N_TRIALS, T_CENSOR = 8, 4.0
N_PILOT, N_ROUND, N_FINAL, ROUNDS = 200_000, 20_000, 40_000, 3
T_DF, T_INFLATE = 5.0, 1.5
ESS_REF_MIN = 2000.0


def with_gamma(theta):
    theta = np.asarray(theta, np.float64)
    return np.concatenate([theta, np.ones((theta.shape[0], 1))], 1)


def set_log_lik(theta, trials, t_censor=T_CENSOR, rule=None, chunk=20_000):
    """log p(trials | theta), float64 [R]: theta [R, 7] valid rows, trials [N, 2] = (choicert, z1)."""
    import wiener_marginal_ref as M
    rule = M.scheme_log_lik if rule is None else rule
    out = np.zeros(np.shape(theta)[0])
    with np.errstate(all="ignore"):
        for i in range(0, out.size, chunk):
            p = with_gamma(theta[i:i + chunk])
            for y, z in np.asarray(trials, np.float64):
                out[i:i + chunk] += rule(p, np.full(p.shape[0], y), np.full(p.shape[0], z), t_censor)
    return out


def log_prior(theta):
    from bayesflow_nddms_amd import priors
    return priors.log_prior_density(priors.restricted_density("single"), theta)


def log_target(theta, trials):
    """log of (likelihood x restricted prior), -inf outside the prior's support or where a trial lies at or before ter."""
    lp = log_prior(theta)
    live = np.isfinite(lp) & (theta[:, 3] < np.abs(trials[:, 0]).min())
    out = np.full(theta.shape[0], -np.inf)
    if np.any(live):
        out[live] = set_log_lik(theta[live], trials) + lp[live]
    return out


def summarise(theta, lw):
    """Self-normalised estimates from log weights: mean, covariance, log of the mean weight, effective sample size."""
    m = lw.max()
    u = np.exp(lw - m)
    sw = u.sum()
    mean = (u[:, None] * theta).sum(0) / sw
    c = theta - mean
    cov = (u[:, None, None] * c[:, :, None] * c[:, None, :]).sum(0) / sw
    return mean, cov, m + math.log(sw / len(lw)), sw * sw / (u * u).sum()


def student_t(rng, n, mean, cov, df=T_DF):
    """n draws of the multivariate Student-t and their log density."""
    d = len(mean)
    L = np.linalg.cholesky(cov)
    zn = rng.standard_normal((n, d))
    g = rng.chisquare(df, n)
    x = mean + (zn @ L.T) / np.sqrt(g / df)[:, None]
    sol = np.linalg.solve(L, (x - mean).T)
    delta2 = (sol * sol).sum(0)
    lq = (math.lgamma(0.5 * (df + d)) - math.lgamma(0.5 * df) - 0.5 * d * math.log(df * math.pi) - np.log(np.diag(L)).sum()
          - 0.5 * (df + d) * np.log1p(delta2 / df))
    return x, lq


def independent_rows(theta, trials, t_censor=T_CENSOR):
    """The independent yardstick per (row, trial), NaN where its rule does not converge (its AssertionError): halves until it passes."""
    import wiener_marginal_ref as M
    out = np.full((theta.shape[0], trials.shape[0]), np.nan)

    def go(idx):
        p = with_gamma(theta[idx])
        try:
            with np.errstate(all="ignore"):
                for k, (y, z) in enumerate(trials):
                    out[idx, k] = M.log_lik(p, np.full(len(idx), y), np.full(len(idx), z), t_censor)
        except AssertionError:
            out[idx] = np.nan
            if len(idx) > 1:
                go(idx[:len(idx) // 2])
                go(idx[len(idx) // 2:])
    go(np.arange(theta.shape[0]))
    return out


def simulate_trials(seed=2023):
    import wiener_marginal_ref as M
    rng = np.random.default_rng(seed)
    p = np.tile(np.asarray(TRUE_PARAMS + (1.0,), np.float64), (N_TRIALS, 1))
    y, z = M._simulate(p, rng, cap=T_CENSOR)
    trials = np.stack([y, z], 1).astype(np.float32).astype(np.float64)      # (as stored)
    assert np.all(trials[:, 0] != 0.0), "a timeout: choose another seed (the yardstick's survival does not converge at strong drift)"
    return trials


def reference_posterior(trials, seed=3):
    import wiener_marginal_ref as M
    from bayesflow_nddms_amd import priors
    rng = np.random.default_rng(seed)
    rows = priors.single_prior_matrix(N_PILOT, seed=seed)[:, :7].astype(np.float64)
    rows = rows[np.isfinite(log_prior(rows))]                            # the prior's draws inside the domain: draws of the restricted prior
    live = rows[:, 3] < np.abs(trials[:, 0]).min()
    lw = np.full(rows.shape[0], -np.inf)
    lw[live] = set_log_lik(rows[live], trials)
    mean, cov, log_ev, ess = summarise(rows, lw)
    print(f"pilot: {rows.shape[0]} prior draws, ess {ess:.1f}, log evidence {log_ev:.4f}")
    for r in range(ROUNDS):
        n = N_FINAL if r == ROUNDS - 1 else N_ROUND
        theta, lq = student_t(rng, n, mean, T_INFLATE * cov)
        lw = log_target(theta, trials) - lq
        mean, cov, log_ev, ess = summarise(theta, lw)
        print(f"round {r + 1}: {n} draws, ess {ess:.1f}, log evidence {log_ev:.4f}, mean {np.round(mean, 4).tolist()}")
    # the scheme against the independent yardstick where the weight is, and on random rows
    pos = np.flatnonzero(np.isfinite(lw))
    heavy = pos[np.argsort(lw[pos])[::-1][:2000]]
    rand = rng.choice(pos, 500, replace=False)
    idx = np.unique(np.concatenate([heavy, rand]))
    ind = independent_rows(theta[idx], trials)
    conv = np.isfinite(ind).all(1)
    p = with_gamma(theta[idx][conv])
    sch = np.stack([M.scheme_log_lik(p, np.full(p.shape[0], y), np.full(p.shape[0], z), T_CENSOR) for y, z in trials], 1)
    diff = float(np.abs(sch - ind[conv]).max())
    unconv = 1.0 - conv.mean()
    print(f"scheme against the independent yardstick on {idx.size} rows: max |difference| per trial {diff:.3g}, not converged {unconv:.4f}")
    assert diff <= 1e-6, diff
    assert unconv <= 0.01, unconv
    assert ess >= ESS_REF_MIN, ess
    return mean, np.sqrt(np.diag(cov)), log_ev, ess, n, unconv, diff


PROPOSAL_SHIFT, PROPOSAL_WIDTH, PROPOSAL_SEED, PROPOSAL_DRAWS = (0.0, 0.0, 0.5, 0.0, 0.0, 0.0, 0.0), 1.25, 7, 20_000
ESS_DEV_MIN = 0.025


def proposal_flow(mean, sd):
    """The end-to-end test's proposal q (flow_importance_ref.proposal_flow with 7 columns): the default InvertibleNetwork with its coupling
    weights scaled by 0.01 -- a near-identity -- and the first ActNorm set so that theta = centre + PROPOSAL_WIDTH sd u: 1.25 sd wide and
    half an sd off in the beta column.  (1.5 sd wide, the basic model's width, puts 42 % of the draws outside the restricted prior's
    support -- this posterior of 8 trials leans on its prior's edges -- and left an effective size of 500 .. 544 of 20 000 over three
    seeds, one of them below the test's condition of 2.5 %; 1.25 sd wide: 989 .. 1469; 1.1: 614 .. 1995, too narrow to be steady.)"""
    import torch
    from bayesflow_nddms_amd.amortizer import InvertibleNetwork
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        net = InvertibleNetwork(num_params=7).eval()
    width = PROPOSAL_WIDTH * np.asarray(sd, np.float64)
    centre = np.asarray(mean, np.float64) + np.asarray(PROPOSAL_SHIFT) * np.asarray(sd, np.float64)
    with torch.no_grad():
        for layer in net.layers:
            for p in layer.parameters():
                p.mul_(0.01)
        net.an_scale[0].copy_(torch.as_tensor(-np.log(width), dtype=torch.float32))
        net.an_bias[0].copy_(torch.as_tensor(-centre / width, dtype=torch.float32))
    return net


def check_proposal(seeds=(PROPOSAL_SEED, PROPOSAL_SEED + 1, PROPOSAL_SEED + 2)):
    """On the CPU, through importance_weights' torch evaluation with set_log_lik as the likelihood: the proposal's ESS at PROPOSAL_DRAWS
    draws, the weighted and the unweighted mean against the yardstick's bound.  -> the effective sizes."""
    import torch
    from bayesflow_nddms_amd import priors
    from bayesflow_nddms_amd.amortizer import importance_weights
    from flow_importance_ref import mean_bound
    g = np.load(GOLDEN)
    net = proposal_flow(g["mean"], g["sd"])
    trials = g["trials"].astype(np.float64)
    table = priors.prior_table(priors.restricted_density("single"))
    out = []
    for seed in seeds:
        z = torch.randn(1, PROPOSAL_DRAWS, 7, generator=torch.Generator().manual_seed(seed))
        with torch.no_grad():
            th, lq = net.inverse_per_set(z, torch.zeros(1, 11), log_density=True)
        th64 = th[0].double().numpy()
        ok = np.isfinite(log_prior(th64))
        ll = np.zeros(PROPOSAL_DRAWS)                                   # (outside the prior's support the weight is 0 whatever the likelihood)
        ll[ok] = set_log_lik(th64[ok], trials)
        w = importance_weights(th, lq, torch.as_tensor(ll)[None], table)
        ess = float(w["ess"][0])
        bound = mean_bound(g["sd"], ess, float(g["ess_ref"]))
        print("seed", seed, "ess", ess, "of", PROPOSAL_DRAWS, "n_zero", int(w["n_zero"][0]), "n_nan", int(w["n_nan"][0]), "log evidence",
              float(w["log_evidence"][0]), "ref", float(g["log_evidence"]), "bound", 4.0 * np.sqrt(1.0 / ess + 1.0 / float(g["ess_ref"])))
        print("   weighted   |mean - ref| / bound", np.round(np.abs(w["mean"][0].numpy() - g["mean"]) / bound, 3))
        print("   unweighted |mean - ref| / bound", np.round(np.abs(th64.mean(0) - g["mean"]) / bound, 3))
        out.append(ess)
    assert min(out) >= ESS_DEV_MIN * PROPOSAL_DRAWS, out
    return out


def main():
    sys.path.insert(0, os.path.dirname(HERE))
    trials = simulate_trials()
    mean, sd, log_ev, ess, n, unconv, diff = reference_posterior(trials)
    print("trials", trials.tolist(), "\nmean", mean, "\nsd", sd, "\nlog evidence", log_ev, "ess", ess, "of", n)
    from bayesflow_nddms_amd import priors
    np.savez(GOLDEN, trials=trials.astype(np.float32), true_params=np.asarray(TRUE_PARAMS), t_censor=T_CENSOR, mean=mean, sd=sd, log_evidence=log_ev,
             ess_ref=ess, n_ref=n, unconverged=unconv, scheme_max_diff=diff,
             domain=np.asarray([priors.MARGINAL_DOMAIN[k] for k in ("std_alpha", "dc", "sigma1")]))
    check_proposal()


if __name__ == "__main__":
    main()
