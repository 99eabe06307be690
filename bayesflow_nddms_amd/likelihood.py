"""The Wiener first-passage log density in the parameterisations the reference's likelihood-based fits use, batched on the device
(include/nddm.h: nddm_wiener_log_likelihood; the math in csrc/nddm_wiener.h and DESIGN.md section 11):

    dwiener_logpdf(y, alpha, tau, beta, delta)                  JAGS dwiener (basic_ddm_dc_pyjags.py:129-133, alpha_not_scaled.py:170-176)
    diffusion_lpdf(Y, boundary, ter, bias, drift, dc)           the Stan function of basic_ddm_dc_pystan2.py:119-131
    pwiener(q, alpha, tau, beta, delta)                         RWiener / HDDM pwiener, dwiener's distribution function (nddm_wiener_cdf)
    qwiener(p, alpha, tau, beta, delta, resp)                   RWiener / HDDM qwiener, pwiener's inverse (nddm_wiener_quantile)
    wiener_rt_quantiles(probs, alpha, tau, beta, delta, ...)    the response-time quantiles of each boundary's own responses
    wiener_choice_prob(alpha, beta, delta, eta, varsigma)       P(upper boundary), drift variability integrated out
    wiener_loglik(model, params, data, draws_per_dataset)       a row's log-likelihood, DIFFERENTIABLE in params (nddm_wiener_log_likelihood_grad)
    single_trial_logpdf(y, z, drift, mu_alpha, beta, ter, ...)  the single-trial model's joint log density of (choicert, z1), the latent
                                                                boundary integrated out (nddm_wiener_marginal_log_likelihood)
    single_trial_loglik(params, data, draws_per_dataset, ...)   a row's marginal log-likelihood under the single-trial model, DIFFERENTIABLE in
                                                                params (nddm_wiener_marginal_log_likelihood_grad)

The first two take numpy arrays, scalars or device tensors, broadcast them against each other (numpy rules), score every element in ONE kernel
launch and return a float32 device tensor of the broadcast shape.  The sign of y / Y is the response: positive = upper boundary.
Invalid parameters give NaN, an RT at or below the non-decision time -inf (the math; see `stan_floor` for Stan's substitution).
"""
import numpy as np

from . import engine


def _dev(x, dev):
    torch = engine.require_device()
    if isinstance(x, torch.Tensor):
        return x.to(device=dev, dtype=torch.float32)
    return torch.as_tensor(np.asarray(x, dtype=np.float32), device=dev)


def _basic_rows(y, drift, boundary, beta, tau, dc, dev):
    """Signed RTs and the basic model's parameters, every argument broadcast (numpy rules) -> (params [R, 5], data [R, n, 2] in the
    simulator's format, the broadcast shape): one row per leading index where the parameters are constant along the last axis, else one
    row per element."""
    torch = engine.require_device()
    y = _dev(y, dev)
    cols = [_dev(c, dev) for c in (drift, boundary, beta, tau, dc)]
    shape = tuple(torch.broadcast_shapes(y.shape, *(c.shape for c in cols)))
    full = shape if shape else (1,)
    pad = lambda x: x.reshape((1,) * (len(full) - x.dim()) + tuple(x.shape))
    y, cols = pad(y), [pad(c) for c in cols]
    n, lead = full[-1], full[:-1]
    if all(c.shape[-1] == 1 for c in cols):       # parameters constant along the last axis: one row per leading index, n trials each
        p = torch.stack([c.expand(lead + (1,)) for c in cols], -1).reshape(-1, 5)
        yy = y.expand(full).reshape(-1, n)
    else:                                         # one row per element
        p = torch.stack([c.expand(full) for c in cols], -1).reshape(-1, 5)
        yy = y.expand(full).reshape(-1, 1)
    data = torch.stack([yy.abs(), torch.where(yy >= 0, 1.0, -1.0).to(torch.float32)], -1).contiguous()
    return p.contiguous(), data, shape


def _basic_logpdf(y, drift, boundary, beta, tau, dc, device=None):
    """log f of signed RTs under the basic model's parameters (no clipping, no censoring), every argument broadcast."""
    torch = engine.require_device()
    dev = engine._device(device)
    p, data, shape = _basic_rows(y, drift, boundary, beta, tau, dc, dev)
    if p.shape[0] == 0 or data.shape[1] == 0:
        return torch.empty(shape, dtype=torch.float32, device=dev)
    out = engine.wiener_log_likelihood(engine.BASIC_DDM_DC, p, data, per_trial=True, want_sum=False, device=dev)
    return out["trial_logp"].reshape(shape)


def dwiener_logpdf(y, alpha, tau, beta, delta, device=None):
    """JAGS `y ~ dwiener(alpha, tau, beta, delta)`: log density of the signed RT y (positive: upper boundary) with boundary separation
    alpha, non-decision time tau, relative start beta and drift delta, all in units of a diffusion coefficient of 1 -- the reference
    passes alpha/varsigma and delta/varsigma (basic_ddm_dc_pyjags.py:129-133).  Returns float32 log f, broadcast shape."""
    return _basic_logpdf(y, delta, alpha, beta, tau, 1.0, device=device)


def diffusion_lpdf(Y, boundary, ter, bias, drift, dc, stan_floor=False, device=None):
    """The reference's Stan function diffusion_lpdf(Y | boundary, ter, bias, drift, dc) (basic_ddm_dc_pystan2.py:119-131): Stan's
    wiener_lpdf with boundary/dc and drift/dc, the upper boundary for Y >= 0, the lower (the upper one of the mirrored process) for Y < 0.

    stan_floor=False (the default): the math -- |Y| <= ter gives -inf.  stan_floor=True: the reference's substitution for |Y| < ter,
    wiener_lpdf(ter + 0.0001 | ...) at the UPPER boundary whatever the sign of Y (:122-123), for like-for-like comparison with its fits."""
    torch = engine.require_device()
    dev = engine._device(device)
    Y = _dev(Y, dev)
    if stan_floor:
        t = _dev(ter, dev)
        Y = torch.where(Y.abs() < t, t + torch.tensor(0.0001, dtype=torch.float32, device=dev), Y)
    return _basic_logpdf(Y, drift, boundary, bias, ter, dc, device=dev)


def pwiener(q, alpha, tau, beta, delta, device=None):
    """RWiener / HDDM `pwiener(q, alpha, tau, beta, delta)`: the distribution function of dwiener, P(RT <= |q|, the boundary the sign of q
    names) -- positive q: upper boundary -- in units of a diffusion coefficient of 1.  DEFECTIVE: its limit in |q| is the boundary's
    probability, so pwiener(q) + pwiener(-q) -> 1.  Broadcasts as dwiener_logpdf does, one kernel launch; returns a float32 device
    tensor of the broadcast shape (0 for |q| <= tau, NaN for invalid parameters)."""
    torch = engine.require_device()
    dev = engine._device(device)
    p, data, shape = _basic_rows(q, delta, alpha, beta, tau, 1.0, dev)
    if p.shape[0] == 0 or data.shape[1] == 0:
        return torch.empty(shape, dtype=torch.float32, device=dev)
    return engine.wiener_cdf(engine.BASIC_DDM_DC, p, data, want_p_upper=False, device=dev)["cdf"].reshape(shape)


def wiener_choice_prob(alpha, beta, delta, eta=0.0, varsigma=1.0, device=None):
    """P(upper boundary) of a diffusion with boundary separation alpha, relative start beta, drift ~ N(delta, eta^2) and diffusion
    coefficient varsigma, every argument broadcast: float32 device tensor of the broadcast shape (one launch, no trials read).  No
    clipping of the drift: a |delta| beyond the alpha_not_scaled kernel's +-5 is brought inside by rescaling alpha, delta, eta and
    varsigma together, which leaves the process unchanged."""
    torch = engine.require_device()
    dev = engine._device(device)
    cols = [_dev(c, dev) for c in (delta, alpha, beta, 0.0, eta, varsigma)]
    k = 5.0 / cols[0].abs().clamp(min=5.0)
    cols = [cols[0] * k, cols[1] * k, cols[2], cols[3], cols[4] * k, cols[5] * k]
    shape = tuple(torch.broadcast_shapes(*(c.shape for c in cols)))
    p = torch.stack([c.expand(shape) for c in cols], -1).reshape(-1, 6).contiguous()
    if p.shape[0] == 0:
        return torch.empty(shape, dtype=torch.float32, device=dev)
    data = torch.zeros((p.shape[0], 1, 2), dtype=torch.float32, device=dev)
    return engine.wiener_cdf(engine.ALPHA_NOT_SCALED, p, data, want_cdf=False, device=dev)["p_upper"].reshape(shape)


_RESP_CODE = {"upper": 1.0, "lower": -1.0, "both": 0.0}


def qwiener(p, alpha, tau, beta, delta, resp="upper", device=None):
    """RWiener / HDDM `qwiener(p, alpha, tau, beta, delta, resp)`: the inverse of pwiener, the response time q with P(RT <= q, the boundary
    `resp` names) = p -- resp "upper", "lower" or "both" (either boundary) -- in units of a diffusion coefficient of 1.  p is DEFECTIVE as
    pwiener's values are: beyond the boundary's probability there is no such time and the result is NaN (+inf at it, tau at p = 0).
    Broadcasts exactly as pwiener does, one kernel launch; returns a float32 device tensor of the broadcast shape (NaN for invalid
    parameters)."""
    if resp not in _RESP_CODE:
        raise ValueError(f"resp must be one of {tuple(_RESP_CODE)}, got {resp!r}")
    torch = engine.require_device()
    dev = engine._device(device)
    rows, data, shape = _basic_rows(p, delta, alpha, beta, tau, 1.0, dev)
    if rows.shape[0] == 0 or data.shape[1] == 0:
        return torch.empty(shape, dtype=torch.float32, device=dev)
    # _basic_rows split p into (|p|, sign): put the sign back (a negative p is NaN in the kernel) and name the boundary
    req = torch.stack([data[..., 0] * data[..., 1], torch.full_like(data[..., 1], _RESP_CODE[resp])], -1).contiguous()
    return engine.wiener_quantile(engine.BASIC_DDM_DC, rows, req, device=dev)["quantile"].reshape(shape)


def _boundary_requests(probs, dev):
    """A shared 1-D `probs` as the request set [1, 2Q, 2] of both boundaries: Q on the lower one (code -1), then Q on the upper one."""
    torch = engine.require_device()
    pr = _dev(probs, dev).reshape(-1)
    code = torch.cat([torch.full_like(pr, -1.0), torch.full_like(pr, 1.0)])
    return torch.stack([torch.cat([pr, pr]), code], -1)[None].contiguous(), int(pr.shape[0])


def wiener_rt_quantiles(probs, alpha, tau, beta, delta, eta=0.0, varsigma=1.0, device=None):
    """Response-time quantiles of each boundary's OWN responses (conditional on the boundary: what a quantile-probability plot and the
    chi-square / G^2 quantile fits use): probs 1-D, shared; the parameters broadcast against each other (drift ~ N(delta, eta^2),
    diffusion coefficient varsigma) -> float32 device tensor [..., 2, Q], [..., 0, :] the lower boundary and [..., 1, :] the upper one.
    One launch, the request set shared by every row.  No clipping of the drift: |delta| > 5 is rescaled as wiener_choice_prob does."""
    torch = engine.require_device()
    dev = engine._device(device)
    cols = [_dev(c, dev) for c in (delta, alpha, beta, tau, eta, varsigma)]
    k = 5.0 / cols[0].abs().clamp(min=5.0)
    cols = [cols[0] * k, cols[1] * k, cols[2], cols[3], cols[4] * k, cols[5] * k]
    shape = tuple(torch.broadcast_shapes(*(c.shape for c in cols)))
    p = torch.stack([c.expand(shape) for c in cols], -1).reshape(-1, 6).contiguous()
    req, Q = _boundary_requests(probs, dev)
    if p.shape[0] == 0 or Q == 0:
        return torch.empty(shape + (2, Q), dtype=torch.float32, device=dev)
    out = engine.wiener_quantile(engine.ALPHA_NOT_SCALED, p, req, draws_per_dataset=p.shape[0], conditional=True, device=dev)["quantile"]
    return out.reshape(shape + (2, Q))


_WienerLoglik = None


def _wiener_loglik_function():
    """The torch.autograd.Function behind wiener_loglik (made on first use: importing this module does not import torch)."""
    global _WienerLoglik
    if _WienerLoglik is None:
        torch = engine._torch()

        class WienerLoglik(torch.autograd.Function):
            @staticmethod
            def forward(ctx, params, data, model, draws_per_dataset, device, censored):
                kw = {"censored": True} if censored else {}             # (the default makes the engine call it always made)
                r = engine.wiener_log_likelihood_grad(model, params.detach(), data.detach() if hasattr(data, "detach") else data,
                                                      draws_per_dataset=draws_per_dataset, device=device, **kw)
                ctx.save_for_backward(r["grad"])
                ctx.params_shape, ctx.params_dtype, ctx.params_device = params.shape, params.dtype, params.device
                return r["loglik"]

            @staticmethod
            def backward(ctx, grad_output):
                (grad,) = ctx.saved_tensors                             # the forward's launch computed it: nothing is launched here
                g = (grad_output.to(grad.dtype)[:, None] * grad).reshape(ctx.params_shape)
                return g.to(device=ctx.params_device, dtype=ctx.params_dtype), None, None, None, None, None

        _WienerLoglik = WienerLoglik
    return _WienerLoglik


def wiener_loglik(model, params, data, draws_per_dataset=1, device=None, censored=False):
    """A row's log-likelihood under the Wiener first-passage density, float64 [R] on the device, DIFFERENTIABLE with respect to `params`
    (a torch tensor; [R, P] in the model's column order): the arguments of engine.wiener_log_likelihood_grad, whose ONE launch the forward
    makes; it keeps the gradient, and the backward is grad_output[:, None] * grad cast to params' dtype -- no second launch.  `data` gets no
    gradient.  With nothing requiring grad the values are the same.

        loss = -likelihood.wiener_loglik(engine.BASIC_DDM_DC, theta, data, censored=True).sum(); loss.backward()

    alpha_not_scaled's Nu is clipped to +-5 (zero gradient where the clip is active).  basic_ddm_dc's censored timeouts (choice 0): with
    censored=True (BASIC_DDM_DC only) the value is differentiable through rows that hold them, still in the one launch.  With the default
    that is NOT IMPLEMENTED -- such a row's value is right and its gradient is NaN in every column, never a partial one."""
    torch = engine._torch()                                             # (the engine call refuses bad host input before it asks for a device)
    if not isinstance(params, torch.Tensor):
        params = torch.as_tensor(np.asarray(params, dtype=np.float64))
    return _wiener_loglik_function().apply(params, data, model, int(draws_per_dataset), device, bool(censored))


_SingleTrialLoglik = None


def _single_trial_loglik_function():
    """The torch.autograd.Function behind single_trial_loglik (made on first use: importing this module does not import torch)."""
    global _SingleTrialLoglik
    if _SingleTrialLoglik is None:
        torch = engine._torch()

        class SingleTrialLoglik(torch.autograd.Function):
            @staticmethod
            def forward(ctx, params, data, draws_per_dataset, t_censor, device):
                r = engine.wiener_marginal_log_likelihood_grad(engine.SINGLE_TRIAL, params.detach(), data.detach() if hasattr(data, "detach") else data,
                                                               draws_per_dataset=draws_per_dataset, t_censor=t_censor, device=device)
                ctx.save_for_backward(r["grad"])
                ctx.params_shape, ctx.params_dtype, ctx.params_device = params.shape, params.dtype, params.device
                return r["loglik"]

            @staticmethod
            def backward(ctx, grad_output):
                (grad,) = ctx.saved_tensors                             # the forward's launch computed it: nothing is launched here
                g = (grad_output.to(grad.dtype)[:, None] * grad).reshape(ctx.params_shape)
                return g.to(device=ctx.params_device, dtype=ctx.params_dtype), None, None, None, None

        _SingleTrialLoglik = SingleTrialLoglik
    return _SingleTrialLoglik


def single_trial_loglik(params, data, draws_per_dataset=1, t_censor=None, device=None):
    """A row's marginal log-likelihood under the single-trial model, float64 [R] on the device, DIFFERENTIABLE with respect to `params` (a
    torch tensor; [R, 8] = drift, mu_alpha, beta, ter, std_alpha, dc, sigma1, gamma): the arguments of
    engine.wiener_marginal_log_likelihood_grad, whose ONE launch the forward makes; it keeps the gradient, and the backward is
    grad_output[:, None] * grad cast to params' dtype and device -- no second launch.  `data` gets no gradient.  With nothing requiring grad
    the values are the same.  Timeouts (choicert 0) are censored at t_censor and have a gradient.

        loss = -likelihood.single_trial_loglik(theta, data, t_censor=4.0).sum(); loss.backward()"""
    torch = engine._torch()                                             # (the engine call refuses bad host input before it asks for a device)
    if not isinstance(params, torch.Tensor):
        params = torch.as_tensor(np.asarray(params, dtype=np.float64))
    return _single_trial_loglik_function().apply(params, data, int(draws_per_dataset), t_censor, device)


def single_trial_logpdf(y, z, drift, mu_alpha, beta, ter, std_alpha, dc, sigma1, gamma=1.0, t_censor=None, device=None):
    """Joint log density of one trial (choicert y, external datum z) of the single-trial model, the per-trial boundary
    a ~ N(mu_alpha, std_alpha^2) | a > 0 integrated out (engine.wiener_marginal_log_likelihood).  Every argument
    broadcasts as dwiener_logpdf's do (numpy rules), one kernel launch; returns a float32 device tensor of the broadcast shape.
    y == 0 is a timeout, scored as log P(no response before t_censor) -- NaN with t_censor=None; |y| <= ter gives -inf, invalid parameters NaN."""
    torch = engine.require_device()
    dev = engine._device(device)
    y, z = _dev(y, dev), _dev(z, dev)
    cols = [_dev(c, dev) for c in (drift, mu_alpha, beta, ter, std_alpha, dc, sigma1, gamma)]
    shape = tuple(torch.broadcast_shapes(y.shape, z.shape, *(c.shape for c in cols)))
    full = shape if shape else (1,)
    pad = lambda x: x.reshape((1,) * (len(full) - x.dim()) + tuple(x.shape))
    y, z, cols = pad(y), pad(z), [pad(c) for c in cols]
    n, lead = full[-1], full[:-1]
    if all(c.shape[-1] == 1 for c in cols):       # parameters constant along the last axis: one row per leading index, n trials each
        p = torch.stack([c.expand(lead + (1,)) for c in cols], -1).reshape(-1, 8)
        data = torch.stack([y.expand(full).reshape(-1, n), z.expand(full).reshape(-1, n)], -1)
    else:                                         # one row per element
        p = torch.stack([c.expand(full) for c in cols], -1).reshape(-1, 8)
        data = torch.stack([y.expand(full).reshape(-1, 1), z.expand(full).reshape(-1, 1)], -1)
    if p.shape[0] == 0 or data.shape[1] == 0:
        return torch.empty(shape, dtype=torch.float32, device=dev)
    out = engine.wiener_marginal_log_likelihood(engine.SINGLE_TRIAL, p.contiguous(), data.contiguous(), t_censor=t_censor, per_trial=True,
                                                want_sum=False, device=dev)
    return out["trial_logp"].reshape(shape)
