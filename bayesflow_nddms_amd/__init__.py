"""MI355X-native Euler-Maruyama drift-diffusion trial simulators behind the generative-model interface of
mdnunez/bayesflow_nddms (basic_ddm_dc / single_trial_alpha_not_scaled / alpha_not_scaled).

Host code is Python; the arithmetic lives in hand-written HIP kernels for gfx950 reached through a C ABI
(include/nddm.h).  There is no CPU fallback: without the built HIP library and a ROCm device the simulators raise.
"""
from .engine import (ALPHA_NOT_SCALED, BASIC_DDM_DC, EXPLICIT_BOUNDARY, SINGLE_TRIAL, SINGLE_TRIAL_ALT, SUMMARY_COLS,
                     SUMMARY_K, GLOBAL_STREAM, StreamState, draw_prior_device, seed, simulate, wiener_cdf, wiener_log_likelihood, wiener_log_likelihood_grad,
                     wiener_hmc, wiener_hmc_joint, wiener_marginal_log_likelihood, wiener_marginal_log_likelihood_grad, wiener_quantile)
from .diagnostics import rhat_neff
from .mcmc import hmc_fit, hmc_fit_joint, hmc_init, hmc_init_joint, q_to_theta, theta_to_q
from .likelihood import (diffusion_lpdf, dwiener_logpdf, pwiener, qwiener, single_trial_loglik, single_trial_logpdf, wiener_choice_prob,
                         wiener_loglik, wiener_rt_quantiles)

__all__ = ["ALPHA_NOT_SCALED", "BASIC_DDM_DC", "EXPLICIT_BOUNDARY", "SINGLE_TRIAL", "SINGLE_TRIAL_ALT",
           "SUMMARY_COLS", "SUMMARY_K", "GLOBAL_STREAM", "StreamState", "draw_prior_device", "seed", "simulate",
           "wiener_log_likelihood", "dwiener_logpdf", "diffusion_lpdf", "wiener_cdf", "pwiener", "wiener_choice_prob",
           "wiener_quantile", "qwiener", "wiener_rt_quantiles", "wiener_log_likelihood_grad", "wiener_loglik",
           "wiener_marginal_log_likelihood", "single_trial_logpdf", "wiener_marginal_log_likelihood_grad", "single_trial_loglik",
           "wiener_hmc", "hmc_fit", "hmc_init", "theta_to_q", "q_to_theta", "rhat_neff", "wiener_hmc_joint", "hmc_fit_joint",
           "hmc_init_joint"]
__version__ = "0.1.0"
