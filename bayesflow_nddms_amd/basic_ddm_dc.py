"""Drop-in for the generative-model section of the reference's basic_ddm_dc.py (lines 50-160): same function
names, argument order and return shapes; the simulator runs on the MI355X through the C ABI.

    from bayesflow_nddms_amd.basic_ddm_dc import draw_prior, prior_N, simulate_trials, configurator
    prior = Prior(prior_fun=draw_prior); ...; generative_model = GenerativeModel(prior, simulator)

or, batched (one kernel launch per batch, device-resident output):

    generative_model = make_generative_model(batched=True)
"""
import numpy as np

from . import engine
from .priors import RNG, DevicePrior, draw_prior_basic as draw_prior, prior_N, truncnorm_better  # noqa: F401
from .simulation import ContextGenerator, GenerativeModel, Prior, Simulator, build_generative_model  # noqa: F401

MODEL = engine.BASIC_DDM_DC
PARAM_NAMES = ("drift", "boundary", "beta", "tau", "dc")   # basic_ddm_dc.py:118 -- the order is the ABI
num_params = 5


def diffusion_trial(drift, boundary, beta, tau, dc, dt=.01, max_steps=400., seed=None, set_offset=None, fast=None, state_f64=False):
    """One trial (basic_ddm_dc.py:85-112) -> (rt, choice).  choice is 0 on timeout (the reference leaves it unbound).
    state_f64=True (here and below): the evidence recurrence in the reference's float64 arithmetic (NDDM_STATE_F64)."""
    r = engine.simulate(MODEL, [drift, boundary, beta, tau, dc], 1, dt=dt, max_steps=max_steps, seed=seed,
                        set_offset=set_offset, fast=fast, want_summary=False, state_f64=state_f64)
    rt, choice = r["trials"][0, 0].tolist()
    return rt, int(choice)


def simulate_trials(params, n_trials, dt=.01, max_steps=400., seed=None, set_offset=None, fast=None, state_f64=False):
    """simulate_trials(params, n_trials) -> float64 [n_trials, 2] = (rt, choice)  (basic_ddm_dc.py:114-125)."""
    r = engine.simulate(MODEL, np.asarray(params, dtype=np.float64).reshape(1, 5), n_trials, dt=dt,
                        max_steps=max_steps, seed=seed, set_offset=set_offset, fast=fast, want_summary=False, state_f64=state_f64)
    return r["trials"][0].cpu().numpy().astype(np.float64)


def batch_simulate_trials(params, n_trials, dt=.01, max_steps=400., seed=None, set_offset=None, fast=None,
                          as_numpy=True, with_summary=True, state_f64=False):
    """Whole batch in one launch: params [B, 5] (numpy or device tensor) -> {'sim_data': [B, n_trials, 2] float32,
    'summary_stats': [B, 10]} (numpy by default -- large batches then travel to pinned host memory chunk by chunk beside the
    simulation of the next chunk, engine.simulate_to_host; device tensors with as_numpy=False)."""
    run = engine.simulate_to_host if as_numpy else engine.simulate
    r = run(MODEL, params, n_trials, dt=dt, max_steps=max_steps, seed=seed, set_offset=set_offset, fast=fast, want_summary=with_summary,
            state_f64=state_f64)
    out = {"sim_data": r["trials"]}
    if with_summary:
        out["summary_stats"] = r["summary"]
    return out


def configurator(sim_dict):
    """basic_ddm_dc.py:139-160: dict -> {'summary_conditions', 'direct_conditions', 'parameters'} (float32).
    Accepts numpy arrays or device tensors (tensors stay on the device)."""
    out = dict()
    data = sim_dict['sim_data']
    n_obs = np.log(sim_dict['sim_non_batchable_context'])
    if hasattr(data, "detach"):
        import torch
        data = data.to(torch.float32)
        out['summary_conditions'] = data
        out['direct_conditions'] = torch.full((data.shape[0], 1), float(n_obs), dtype=torch.float32, device=data.device)
        pd = sim_dict['prior_draws']
        out['parameters'] = pd.to(torch.float32) if hasattr(pd, "detach") else torch.as_tensor(
            np.asarray(pd), dtype=torch.float32, device=data.device)
        return out
    data = data.astype(np.float32)
    out['summary_conditions'] = data
    # float32 as on the reference's pinned NumPy 1.23.5 (value-based casting); NumPy >= 2 would promote to float64
    out['direct_conditions'] = (n_obs * np.ones((data.shape[0], 1), dtype=np.float32)).astype(np.float32)
    out['parameters'] = np.asarray(sim_dict['prior_draws']).astype(np.float32)
    return out


def make_generative_model(batched=True, device_prior=False, dt=.01, max_steps=400., fast=None, as_numpy=True,
                          seed=None, skip_test=False):
    """The reference's wrapper block (basic_ddm_dc.py:130-134).  batched=False keeps the per-set simulator_fun loop
    exactly as BayesFlow runs it; batched=True hands the whole batch to one kernel launch (and, with
    device_prior=True, also draws the parameters on the device)."""
    return build_generative_model("basic", "basic_ddm_dc", PARAM_NAMES, draw_prior, simulate_trials, batch_simulate_trials, batched,
                                  device_prior, dt, max_steps, fast, as_numpy, seed, skip_test)


def log_likelihood(params, sim_data, per_trial=False):
    """log p(sim_data | params) under the Wiener first-passage density, one launch (engine.wiener_log_likelihood): params [R, 5] (or
    [5]), sim_data [D, n_trials, 2] (or [n_trials, 2]) = (rt, choice) as simulate_trials writes it, R = D * S -- row r is scored
    against data set r // S.  A timeout (choice 0) counts as right-censored, log P(T > rt - tau).  Returns float64 [R] on the device
    (and float32 [R, n_trials] per-trial values with per_trial=True)."""
    p = params if hasattr(params, "is_cuda") else np.asarray(params, dtype=np.float64).reshape(-1, 5)
    d = sim_data if hasattr(sim_data, "is_cuda") else np.asarray(sim_data, dtype=np.float64)
    R = p.shape[0] if p.ndim == 2 else 1
    D = d.shape[0] if d.ndim == 3 else 1
    if R % D:
        raise ValueError(f"{R} parameter rows cannot be split over {D} data sets")
    r = engine.wiener_log_likelihood(MODEL, p, d, draws_per_dataset=R // D, per_trial=per_trial)
    return (r["loglik"], r["trial_logp"]) if per_trial else r["loglik"]


def log_likelihood_and_grad(params, sim_data, censored=False):
    """log p(sim_data | params) and its gradient in (drift, boundary, beta, tau, dc), one launch (engine.wiener_log_likelihood_grad): the
    arguments of log_likelihood.  Returns (float64 [R], float64 [R, 5]) on the device; the first has log_likelihood's bits.
    censored=True: a censored timeout (choice 0, as simulate_trials writes it) adds the gradient of log P(T > rt - tau), so data straight
    from the simulator have a finite gradient.  With the default that is NOT IMPLEMENTED -- a row that holds a timeout keeps its value and
    gets NaN in every gradient column.  For a differentiable torch value see likelihood.wiener_loglik."""
    p = params if hasattr(params, "is_cuda") else np.asarray(params, dtype=np.float64).reshape(-1, 5)
    d = sim_data if hasattr(sim_data, "is_cuda") else np.asarray(sim_data, dtype=np.float64)
    R = p.shape[0] if p.ndim == 2 else 1
    D = d.shape[0] if d.ndim == 3 else 1
    if R % D:
        raise ValueError(f"{R} parameter rows cannot be split over {D} data sets")
    r = engine.wiener_log_likelihood_grad(MODEL, p, d, draws_per_dataset=R // D, **({"censored": True} if censored else {}))
    return r["loglik"], r["grad"]


def cdf(params, sim_data):
    """P(T <= rt - tau, the boundary each trial ended on | params), one launch (engine.wiener_cdf): the arguments of log_likelihood.  A
    timeout (choice 0) gives P(T <= rt - tau) over both boundaries.  Returns float32 [R, n_trials] on the device."""
    p = params if hasattr(params, "is_cuda") else np.asarray(params, dtype=np.float64).reshape(-1, 5)
    d = sim_data if hasattr(sim_data, "is_cuda") else np.asarray(sim_data, dtype=np.float64)
    R = p.shape[0] if p.ndim == 2 else 1
    D = d.shape[0] if d.ndim == 3 else 1
    if R % D:
        raise ValueError(f"{R} parameter rows cannot be split over {D} data sets")
    return engine.wiener_cdf(MODEL, p, d, draws_per_dataset=R // D, want_p_upper=False)["cdf"]


def quantile(params, probs=(.1, .3, .5, .7, .9)):
    """Response-time quantiles of each boundary's own responses under params, one launch (engine.wiener_quantile, conditional): params
    [R, 5] (or [5]), probs 1-D -> float32 [R, 2, Q] on the device, [:, 0] the lower boundary and [:, 1] the upper one: the predicted
    side of a quantile-probability plot, beside cdf."""
    p = params if hasattr(params, "is_cuda") else np.asarray(params, dtype=np.float64).reshape(-1, 5)
    pr = np.asarray(probs, dtype=np.float64).reshape(-1)
    R, Q = (p.shape[0] if p.ndim == 2 else 1), pr.shape[0]
    req = np.stack([np.concatenate([pr, pr]), np.concatenate([-np.ones(Q), np.ones(Q)])], -1)[None]
    return engine.wiener_quantile(MODEL, p, req, draws_per_dataset=max(R, 1), conditional=True)["quantile"].reshape(R, 2, Q)


def fit_hmc(data, **kw):
    """The reference's likelihood-based fit of this model (basic_ddm_dc_pyjags.py: JAGS over dwiener) by batched Hamiltonian Monte Carlo on
    the device: mcmc.hmc_fit's arguments and its result, the reference's JAGS-sample layout (alpha, ndt, beta, delta, varsigma, each
    [participants, samples, chains]) that diagnostics.rhat_neff reads.  censored=True: data straight from simulate_trials /
    batch_simulate_trials, timeouts (choice 0 at rt = max_steps * dt + tau) included, scored right-censored; without it a data set that
    holds a timeout is refused (a host array) or flagged (a device tensor)."""
    from . import mcmc
    return mcmc.hmc_fit(data, **kw)
