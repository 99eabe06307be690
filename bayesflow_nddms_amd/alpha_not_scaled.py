"""Drop-in for the data-generation section of the reference's alpha_not_scaled.py (lines 52-128): a dcDDM with
per-participant parameters, per-trial drift ~ N(delta, deltatrialsd), and one external datum per participant
extdata[p] ~ N(alpha[p], sigma) that identifies the diffusion coefficient.

The reference generates the choice-RTs with pyhddmjagsutils.simulratcliff, an EXACT first-passage sampler
(pyhddmjagsutils.py:47-176), not with Euler-Maruyama.  Here the same process is integrated by the Euler-Maruyama
HIP kernel (north_star).  Plain Euler-Maruyama monitors the boundaries only on the time grid and therefore detects
crossings late by O(sqrt(dt)) (KS ~0.07 vs the exact sampler at dt=.001 for fast trials); by default this module
switches on the kernel's Brownian-bridge boundary correction (bridge=True), which samples the between-grid-point
crossings with their exact conditional probability and brings the KS distance to the exact sampler below 0.01 at
dt=.001 (tests/test_gpu_distribution.py).  bridge=False gives the plain scheme of the other models.

Since round 6 the reference's own generator exists on the device as well: `simulratcliff(...)` below and `generate_data(...,
method="exact")` run pyhddmjagsutils.simulratcliff's algorithm -- the random walk on spheres with its rejection step, no time grid --
through nddm_simulratcliff (include/nddm.h; csrc/nddm_ratcliff.h), bit-equal to its CPU restatement in exact mode and at the
two-sample noise floor against the reference's own draws (tests/golden/ratcliff.npz).  The Euler-Maruyama forms stay: they are what
north_star names, and `method="em"` remains the default of generate_data.
"""
import numpy as np

from . import engine

PARAM_NAMES = ("Nu", "Alpha", "Beta", "Tau", "Eta", "Varsigma")
SIGMA_OF_TEST = {1: .5, 2: .1, 3: .01, 4: .2}   # alpha_not_scaled.py:73-81


def simulratcliff_em(N=100, Alpha=1, Tau=.4, Nu=1, Beta=.5, Eta=.3, Varsigma=1, dt=.001, max_steps=4000,
                     seed=None, set_offset=None, fast=None, bridge=True):
    """Same call shape as simulratcliff(N, Alpha, Tau, Nu, Beta, Eta=, Varsigma=) (pyhddmjagsutils.py:47) without
    the range* arguments the generator never uses: signed RTs float64 [N] (negative = response B)."""
    if (Nu < -5) or (Nu > 5):          # pyhddmjagsutils.py:102-103
        Nu = np.sign(Nu) * 5
    r = engine.simulate(engine.ALPHA_NOT_SCALED, [[Nu, Alpha, Beta, Tau, Eta, Varsigma]], N, dt=dt,
                        max_steps=max_steps, seed=seed, set_offset=set_offset, fast=fast, bridge=bridge,
                        want_summary=False)
    return r["trials"][0, :, 0].cpu().numpy().astype(np.float64)


def simulratcliff(N=100, Alpha=1, Tau=.4, Nu=1, Beta=.5, rangeTau=0, rangeBeta=0, Eta=.3, Varsigma=1, seed=None, set_offset=None, fast=None):
    """pyhddmjagsutils.simulratcliff (:47-176) with its own signature, on the device: signed RTs float64 [N] (negative = response B)
    from the exact first-passage sampler.  rangeTau / rangeBeta must be 0 (the generator never passes them: alpha_not_scaled.py:96-97).
    A trial the sampler cannot finish (parameters beyond its domain: engine.simulratcliff) is NaN."""
    if rangeTau != 0 or rangeBeta != 0:
        raise ValueError("the device sampler takes rangeTau = rangeBeta = 0 (as alpha_not_scaled.py:96-97 calls it)")
    r = engine.simulratcliff([[Nu, Alpha, Beta, Tau, Eta, Varsigma]], N, seed=seed, set_offset=set_offset, fast=fast, want_summary=False)
    return r["trials"][0, :, 0].cpu().numpy().astype(np.float64)


def draw_participants(nparts=100, seed=2021):
    """alpha_not_scaled.py:64-72, 83-88: participant-level parameters on the global NumPy stream, index 17 fixed."""
    np.random.seed(seed)
    ndt = np.random.uniform(.15, .6, size=nparts)
    alpha = np.random.uniform(.8, 1.4, size=nparts)
    beta = np.random.uniform(.3, .7, size=nparts)
    delta = np.random.uniform(-4, 4, size=nparts)
    varsigma = np.random.uniform(.8, 1.4, size=nparts)
    deltatrialsd = np.random.uniform(0, 2, size=nparts)
    if nparts > 17:
        ndt[17], alpha[17], beta[17], delta[17], varsigma[17], deltatrialsd[17] = .4, 1.2, .5, 3.5, 1.2, 1
    return dict(ndt=ndt, alpha=alpha, beta=beta, delta=delta, varsigma=varsigma, deltatrialsd=deltatrialsd)


def generate_data(test_num=2, nparts=100, ntrials=100, seed=2021, dt=.001, max_steps=4000, sim_seed=None,
                  set_offset=None, fast=None, bridge=True, method="em"):
    """alpha_not_scaled.py:52-128 in one launch: returns the `genparam` dictionary the reference saves to .mat
    (same keys), all participants simulated as one batch of `nparts` parameter sets x `ntrials` trials.
    method="em": the Euler-Maruyama kernel (with the bridge correction by default); method="exact": the reference's own generator,
    simulratcliff, on the device (dt / max_steps / bridge are then unused)."""
    if method not in ("em", "exact"):
        raise ValueError("method must be 'em' or 'exact'")
    sigma = SIGMA_OF_TEST[test_num]
    par = draw_participants(nparts, seed)
    P = np.stack([np.clip(par["delta"], -5, 5), par["alpha"], par["beta"], par["ndt"], par["deltatrialsd"],
                  par["varsigma"]], axis=1)
    if method == "exact":
        r = engine.simulratcliff(P, ntrials, seed=seed if sim_seed is None else sim_seed, set_offset=0 if set_offset is None else set_offset,
                                 fast=fast, ext_sigma=sigma, ext_mode=1 if test_num == 4 else 0, want_ext=True, want_summary=False)
    else:
        r = engine.simulate(engine.ALPHA_NOT_SCALED, P, ntrials, dt=dt, max_steps=max_steps,
                            seed=seed if sim_seed is None else sim_seed, set_offset=0 if set_offset is None else set_offset,
                            fast=fast, bridge=bridge, ext_sigma=sigma, ext_mode=1 if test_num == 4 else 0, want_ext=True,
                            want_summary=False)
    y = engine.to_host(r["trials"][..., 0]).astype(np.float64).reshape(-1)
    N = nparts * ntrials
    var_alpha = (1 / 12) * (1.4 - .8) ** 2
    genparam = dict(par)
    genparam.update(sigma=sigma, var_alpha=var_alpha, prop_cog_var=var_alpha / (var_alpha + sigma ** 2),
                    rt=np.abs(y), acc=(np.sign(y) + 1) / 2, y=y,
                    extdata=r["ext"].cpu().numpy().astype(np.float64),
                    participant=np.repeat(np.arange(1, nparts + 1), ntrials).astype(np.float64),
                    nparts=nparts, ntrials=ntrials, N=N)
    return genparam


def fit_hmc(genparam_or_y, extdata=None, **kw):
    """The reference's JAGS fit of this model (alpha_not_scaled.py:138-259: per participant delta, alpha, beta, ndt, varsigma; extdata[p] ~
    N(alpha[p], sigma); one shared sigma ~ N(3, 1) T(0, 10)) on the device: mcmc.hmc_fit_joint's arguments and its result, the reference's
    sample layout plus 'sigma' [1, samples // thin, chains].  Takes generate_data's `genparam` dictionary, or the signed response times y
    [P, n_trials] (y = +-rt, positive = upper boundary) with extdata [P]."""
    from . import mcmc
    if isinstance(genparam_or_y, dict):
        g = genparam_or_y
        y = np.asarray(g["y"], dtype=np.float64).reshape(int(g["nparts"]), int(g["ntrials"]))
        extdata = g["extdata"] if extdata is None else extdata
    else:
        y = np.atleast_2d(np.asarray(genparam_or_y.detach().cpu().numpy() if hasattr(genparam_or_y, "detach") else genparam_or_y, dtype=np.float64))
    if extdata is None:
        raise ValueError("extdata [P] is required with signed response times")
    if y.ndim != 2:
        raise ValueError(f"y must have shape [P, n_trials], got {y.shape}")
    return mcmc.hmc_fit_joint(np.stack([np.abs(y), np.sign(y)], -1).astype(np.float32), extdata, **kw)


def log_likelihood(params, y, per_trial=False):
    """log p(y | params) of the generator's model (drift ~ N(Nu, Eta) integrated out, Nu clipped to +-5 as the generator does), one
    launch: params [R, 6] (or [6]) = Nu, Alpha, Beta, Tau, Eta, Varsigma; y [D, n_trials] (or [n_trials]) the signed RTs
    (y = +-rt, positive = upper boundary; alpha_not_scaled.py:98-100), R = D * S -- row r is scored against data set r // S.  y == 0
    (the Euler-Maruyama form's timeout) carries no time and gives NaN.  Returns float64 [R] on the device (and float32 [R, n_trials]
    per-trial values with per_trial=True)."""
    p = params if hasattr(params, "is_cuda") else np.asarray(params, dtype=np.float64).reshape(-1, 6)
    if hasattr(y, "is_cuda"):
        import torch
        yy = y[None] if y.ndim == 1 else y
        d = torch.stack([yy, (torch.sign(yy) + 1) / 2], -1)
    else:
        yy = np.asarray(y, dtype=np.float64)
        yy = yy[None] if yy.ndim == 1 else yy
        d = np.stack([yy, (np.sign(yy) + 1) / 2], -1)
    R, D = (p.shape[0] if p.ndim == 2 else 1), d.shape[0]
    if R % D:
        raise ValueError(f"{R} parameter rows cannot be split over {D} data sets")
    r = engine.wiener_log_likelihood(engine.ALPHA_NOT_SCALED, p, d, draws_per_dataset=R // D, per_trial=per_trial)
    return (r["loglik"], r["trial_logp"]) if per_trial else r["loglik"]


def log_likelihood_and_grad(params, y):
    """log p(y | params) and its gradient in (Nu, Alpha, Beta, Tau, Eta, Varsigma), one launch (engine.wiener_log_likelihood_grad): the
    arguments of log_likelihood.  Returns (float64 [R], float64 [R, 6]) on the device; the first has log_likelihood's bits.  Where Nu is
    clipped to +-5 its gradient is 0; y == 0 gives NaN in both.  For a differentiable torch value see likelihood.wiener_loglik."""
    p = params if hasattr(params, "is_cuda") else np.asarray(params, dtype=np.float64).reshape(-1, 6)
    if hasattr(y, "is_cuda"):
        import torch
        yy = y[None] if y.ndim == 1 else y
        d = torch.stack([yy, (torch.sign(yy) + 1) / 2], -1)
    else:
        yy = np.asarray(y, dtype=np.float64)
        yy = yy[None] if yy.ndim == 1 else yy
        d = np.stack([yy, (np.sign(yy) + 1) / 2], -1)
    R, D = (p.shape[0] if p.ndim == 2 else 1), d.shape[0]
    if R % D:
        raise ValueError(f"{R} parameter rows cannot be split over {D} data sets")
    r = engine.wiener_log_likelihood_grad(engine.ALPHA_NOT_SCALED, p, d, draws_per_dataset=R // D)
    return r["loglik"], r["grad"]


def cdf(params, y):
    """P(T <= |y| - Tau, the boundary the sign of y names | params) of the generator's model (drift ~ N(Nu, Eta) integrated out, Nu clipped
    to +-5), one launch (engine.wiener_cdf): the arguments of log_likelihood.  y == 0 gives NaN.  Returns float32 [R, n_trials] on the
    device."""
    p = params if hasattr(params, "is_cuda") else np.asarray(params, dtype=np.float64).reshape(-1, 6)
    if hasattr(y, "is_cuda"):
        import torch
        yy = y[None] if y.ndim == 1 else y
        d = torch.stack([yy, (torch.sign(yy) + 1) / 2], -1)
    else:
        yy = np.asarray(y, dtype=np.float64)
        yy = yy[None] if yy.ndim == 1 else yy
        d = np.stack([yy, (np.sign(yy) + 1) / 2], -1)
    R, D = (p.shape[0] if p.ndim == 2 else 1), d.shape[0]
    if R % D:
        raise ValueError(f"{R} parameter rows cannot be split over {D} data sets")
    return engine.wiener_cdf(engine.ALPHA_NOT_SCALED, p, d, draws_per_dataset=R // D, want_p_upper=False)["cdf"]


def quantile(params, probs=(.1, .3, .5, .7, .9)):
    """Response-time quantiles of each boundary's own responses under params, one launch (engine.wiener_quantile, conditional): params
    [R, 6] (or [6]), probs 1-D -> float32 [R, 2, Q] on the device, [:, 0] the lower boundary and [:, 1] the upper one: the predicted
    side of a quantile-probability plot, beside cdf."""
    p = params if hasattr(params, "is_cuda") else np.asarray(params, dtype=np.float64).reshape(-1, 6)
    pr = np.asarray(probs, dtype=np.float64).reshape(-1)
    R, Q = (p.shape[0] if p.ndim == 2 else 1), pr.shape[0]
    req = np.stack([np.concatenate([pr, pr]), np.concatenate([-np.ones(Q), np.ones(Q)])], -1)[None]
    return engine.wiener_quantile(engine.ALPHA_NOT_SCALED, p, req, draws_per_dataset=max(R, 1), conditional=True)["quantile"].reshape(R, 2, Q)
