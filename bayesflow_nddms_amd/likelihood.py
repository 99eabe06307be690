"""The Wiener first-passage log density in the parameterisations the reference's likelihood-based fits use, batched on the device
(include/nddm.h: nddm_wiener_log_likelihood; the math in csrc/nddm_wiener.h and DESIGN.md section 11):

    dwiener_logpdf(y, alpha, tau, beta, delta)                  JAGS dwiener (basic_ddm_dc_pyjags.py:129-133, alpha_not_scaled.py:170-176)
    diffusion_lpdf(Y, boundary, ter, bias, drift, dc)           the Stan function of basic_ddm_dc_pystan2.py:119-131

Both take numpy arrays, scalars or device tensors, broadcast them against each other (numpy rules), score every element in ONE kernel
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


def _basic_logpdf(y, drift, boundary, beta, tau, dc, device=None):
    """log f of signed RTs under the basic model's parameters (no clipping, no censoring), every argument broadcast."""
    torch = engine.require_device()
    dev = engine._device(device)
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
    if p.shape[0] == 0 or data.shape[1] == 0:
        return torch.empty(shape, dtype=torch.float32, device=dev)
    out = engine.wiener_log_likelihood(engine.BASIC_DDM_DC, p.contiguous(), data, per_trial=True, want_sum=False, device=dev)
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
