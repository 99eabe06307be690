"""Batched device entry of the DDM trial simulators: Python adapter over the C ABI (include/nddm.h).

PyTorch is plumbing here (device memory and streams); all arithmetic happens in the HIP kernels.
There is no CPU path: calls raise if no ROCm device / HIP library is available.
"""
import math
import os
import threading

import numpy as np

from . import _lib

BASIC_DDM_DC, SINGLE_TRIAL, SINGLE_TRIAL_ALT, ALPHA_NOT_SCALED, EXPLICIT_BOUNDARY = range(5)
SUMMARY_K = 10
SUMMARY_COLS = ("n_upper", "n_lower", "n_missing", "mean_rt", "var_rt", "mean_rt_upper", "var_rt_upper",
                "mean_z", "var_z", "choice_mean")
NPARAMS = {BASIC_DDM_DC: 5, SINGLE_TRIAL: 8, SINGLE_TRIAL_ALT: 8, ALPHA_NOT_SCALED: 6, EXPLICIT_BOUNDARY: 4}
# columns that must be > 0 for the process to be defined (boundary / diffusion coefficient), per model
_POSITIVE_COLS = {BASIC_DDM_DC: (1, 4), SINGLE_TRIAL: (5,), SINGLE_TRIAL_ALT: (1,), ALPHA_NOT_SCALED: (1, 5),
                  EXPLICIT_BOUNDARY: (3,)}

# default Gaussian transform of the product path; tests pin the exact one against the oracle bit for bit
DEFAULT_FAST = True


def _torch():
    import torch
    return torch


def require_device():
    """Fail loudly when the HIP path cannot run (no silent CPU fallback)."""
    torch = _torch()
    _lib.lib()
    if not torch.cuda.is_available():
        raise RuntimeError("bayesflow_nddms_amd needs a ROCm GPU (torch.cuda.is_available() is False); "
                           "there is no CPU fallback")
    return torch


def _device(device):
    """The torch.device a call runs on: the one named, or the current ROCm device."""
    torch = _torch()
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _ptr(t):
    return None if t is None else t.data_ptr()


def _u64(v):
    """Seeds and set offsets are uint64 in the ABI: a negative or oversized Python int wraps as it would there."""
    return int(v) & 0xFFFFFFFFFFFFFFFF


# what simulate() and simulate_to_host() take as params: (dimensions, size of the last one, the refusal's text)
_SIM_ROWS = {m: (2, P, f"params must have shape [B, {P}] for this model") for m, P in NPARAMS.items()}


def _check_shape(shape, ndim, last, label):
    # the leading dimension may be empty (no rows is a batch), the inner ones may not
    if len(shape) != ndim or shape[-1] != last or 0 in shape[1:-1]:
        raise ValueError(f"{label}, got {tuple(shape)}")


def _host_rows(x, ndim, last, label):
    """Host input (array-like or CPU tensor) as a float64 array, a single item promoted to a batch of one, shape-checked: what the
    callers' value checks read.  None for a device tensor: those are never read on the host.  `label`: the caller's refusal."""
    if getattr(x, "is_cuda", False):
        return None
    a = np.ascontiguousarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=np.float64)
    if a.ndim == ndim - 1:
        a = a[None]
    _check_shape(a.shape, ndim, last, label)
    return a


def _device_rows(x, host, dev, ndim, last, label):
    """The float32 contiguous device tensor the kernels read: the upload of `host` (what _host_rows made of x, after the caller's
    value checks), or the device tensor x itself -- promoted, shape-checked and cast, its values never looked at."""
    torch = _torch()
    if host is not None:
        return torch.as_tensor(host, dtype=torch.float32).contiguous().to(dev)
    if x.ndim == ndim - 1:
        x = x[None]
    _check_shape(x.shape, ndim, last, label)
    return x.to(dtype=torch.float32).contiguous()


def _out_buffer(want, buf, shape, dev):
    """A float32 output of `shape`: allocated when it is wanted and the caller brought none; a buffer the caller brought is used
    as it is or refused."""
    torch = _torch()
    if buf is None:
        return torch.empty(shape, dtype=torch.float32, device=dev) if want else None
    if tuple(buf.shape) != shape or buf.dtype != torch.float32 or not buf.is_contiguous() or not buf.is_cuda:
        raise ValueError(f"output buffer must be a contiguous float32 device tensor of shape {shape}")
    return buf


def _bounds_device(bounds, B, n_trials, dev):
    """The explicit-boundary model's per-trial boundaries as f32 [B, n_trials] on the device; host values are checked first."""
    torch = _torch()
    if getattr(bounds, "is_cuda", False):
        return bounds.to(dtype=torch.float32).reshape(B, n_trials).contiguous()
    b_np = np.ascontiguousarray(np.asarray(bounds, dtype=np.float64).reshape(B, n_trials))
    if np.any(b_np < 0) or not np.all(np.isfinite(b_np)):
        raise ValueError("Trial-level boundary cannot be less than zero")
    return torch.as_tensor(b_np, dtype=torch.float32).contiguous().to(dev)


class StreamState:
    """Functional RNG position: (seed, next set index).  The simulators are stateless apart from this pair, so a
    resumed run continues the stream by restoring it (checkpoint/resume)."""

    def __init__(self, seed=0, offset=0):
        self._lock = threading.Lock()
        self.seed = int(seed)
        self.offset = int(offset)

    def take(self, n_sets):
        with self._lock:
            off = self.offset
            self.offset += int(n_sets)
            return self.seed, off

    def get_state(self):
        return {"seed": self.seed, "offset": self.offset}

    def set_state(self, state):
        with self._lock:
            self.seed, self.offset = int(state["seed"]), int(state["offset"])


GLOBAL_STREAM = StreamState(seed=0)


def seed(s):
    """Reset the package-level stream (the analogue of np.random.seed for the device simulators)."""
    GLOBAL_STREAM.set_state({"seed": int(s), "offset": 0})


def _stream_position(seed, set_offset, stream_state, n_sets):
    """(seed, set_offset) of a call over n_sets parameter sets, as uint64.  Unless the caller gave both, the position is taken from
    the stream state -- once, and the stream moves on by n_sets even when one of the two was given."""
    if seed is None or set_offset is None:
        s_seed, s_off = (stream_state or GLOBAL_STREAM).take(n_sets)
        seed = s_seed if seed is None else seed
        set_offset = s_off if set_offset is None else set_offset
    return _u64(seed), _u64(set_offset)


def max_k_of(max_steps):
    """The reference loops `while ... n_steps < max_steps` with a float cap (basic_ddm_dc.py:87, 95): the largest
    step count reached is ceil(max_steps)."""
    return int(math.ceil(float(max_steps)))


def validate_params_host(model, params):
    """Host-side validation (only possible when parameters arrive on the host): the reference's error
    convention is ValueError (imputation_from_stahl_not_scaled.py:124-125)."""
    p = np.asarray(params)
    if not np.all(np.isfinite(p)):
        raise ValueError("parameters must be finite")
    for c in _POSITIVE_COLS[model]:
        if np.any(p[..., c] <= 0):
            raise ValueError(f"parameter column {c} (boundary / diffusion coefficient) must be > 0")
    if model in (SINGLE_TRIAL, SINGLE_TRIAL_ALT):
        lat = p[..., 1] if model == SINGLE_TRIAL else p[..., 5]
        if np.any(lat + 8.0 * np.abs(p[..., 4]) <= 0):
            raise ValueError("per-trial latent N(mean, std) > 0 is (numerically) never satisfied")


# the per-model entries that take (params, common arguments, trials, summary, stream) and nothing else
_PLAIN_ENTRY = {BASIC_DDM_DC: "nddm_basic_ddm_dc_simulate", SINGLE_TRIAL: "nddm_single_trial_simulate",
                SINGLE_TRIAL_ALT: "nddm_single_trial_alt_simulate"}


def simulate(model, params, n_trials, dt=0.01, max_steps=400.0, seed=None, set_offset=None, fast=None,
             bounds=None, ext_sigma=0.0, ext_mode=0, bridge=False, packed=False, want_trials=True, want_summary=True, want_ext=False,
             out_trials=None, out_summary=None, stream_state=None, device=None, set_offset_dev=None, want_codes=False,
             out_codes=None, state_f64=False):
    """Run one batched simulation on the current ROCm device.

    state_f64=True selects NDDM_STATE_F64 (include/nddm.h): the evidence is carried in float64 exactly as the reference's recurrence
    does (basic_ddm_dc.py:91-103) on the same normals -- basic_ddm_dc and single_trial only; with fast=False every trial's (step,
    choice) equals the float64 oracle's bit for bit.

    params: array-like or torch tensor [B, P] (or [P]) in the reference's parameter order.
    packed=True selects NDDM_GAUSS_PACKED (include/nddm.h): 8 normals per Philox block from 16 + 16 bit pairs, ~25 % faster,
    a different random stream; not with the bridge, max_steps < 2^14.

    set_offset_dev: optional device int64 tensor [1]; the global index of row 0 is then set_offset + its value WHEN THE
    LAUNCH RUNS (nddm_simulate_indirect) -- a launch captured into a hipGraph moves along the random stream by a captured
    `set_offset_dev += B` instead of new kernel arguments.

    want_codes / out_codes: also (or, with want_trials=False, only) write the trials in the 2-byte wire format, int16 [B, n_trials]
    holding uint16 (step index | code << 14) -- basic_ddm_dc and alpha_not_scaled without the bridge, max_steps < 2^14;
    decode_codes() gives the float pairs back (include/nddm.h: nddm_simulate_codes).  That entry point has no output for
    alpha_not_scaled's external datum: with want_ext it is written by a second, step-less launch (the same bits as any launch's).

    Returns a dict of torch tensors on the device: 'trials' f32 [B, n_trials, 2], 'summary' f32 [B, 10],
    'ext' f32 [B] (alpha_not_scaled only), plus 'seed' / 'set_offset' actually used.
    """
    torch = require_device()
    L = _lib.lib()
    dev = _device(device)
    rows = _SIM_ROWS[model]
    p_np = _host_rows(params, *rows)
    if p_np is not None:
        validate_params_host(model, p_np)
    p_dev = _device_rows(params, p_np, dev, *rows)
    B = int(p_dev.shape[0])
    n_trials = int(n_trials)
    if n_trials <= 0:
        raise ValueError("n_trials must be positive")
    if not (dt > 0 and math.isfinite(dt)):
        raise ValueError("dt must be finite and > 0")
    max_k = max_k_of(max_steps)
    if max_k < 0:
        raise ValueError("max_steps must be >= 0")

    b_dev = None
    if model == EXPLICIT_BOUNDARY:
        if bounds is None:
            raise ValueError("explicit-boundary model needs `bounds`")
        b_dev = _bounds_device(bounds, B, n_trials, dev)

    seed, set_offset = _stream_position(seed, set_offset, stream_state, B)
    fast = DEFAULT_FAST if fast is None else bool(fast)
    flags = (_lib.GAUSS_FAST if fast else _lib.GAUSS_EXACT) | (_lib.BRIDGE if bridge else 0) | (_lib.GAUSS_PACKED if packed else 0) \
        | (_lib.STATE_F64 if state_f64 else 0)
    if bridge and model != ALPHA_NOT_SCALED:
        raise ValueError("the Brownian-bridge correction is only available for the alpha_not_scaled model")

    with torch.cuda.device(dev):
        out_ext = torch.empty((B,), dtype=torch.float32, device=dev) if (want_ext and model == ALPHA_NOT_SCALED) else None
        if want_codes and out_codes is None:
            out_codes = torch.empty((B, n_trials), dtype=torch.int16, device=dev)
        if out_codes is not None and (tuple(out_codes.shape) != (B, n_trials) or out_codes.dtype != torch.int16
                                      or not out_codes.is_contiguous() or not out_codes.is_cuda):
            raise ValueError(f"out_codes must be a contiguous int16 device tensor of shape {(B, n_trials)}")
        out_trials = _out_buffer(want_trials, out_trials, (B, n_trials, 2), dev)
        out_summary = _out_buffer(want_summary, out_summary, (B, SUMMARY_K), dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        if B > 0:
            common = (B, n_trials, float(dt), max_k, seed, set_offset, flags)
            if set_offset_dev is not None and not (isinstance(set_offset_dev, torch.Tensor) and set_offset_dev.is_cuda
                                                   and set_offset_dev.dtype == torch.int64 and set_offset_dev.numel() >= 1):
                raise ValueError("set_offset_dev must be a device int64 tensor")
            if out_codes is not None:
                if out_ext is not None:
                    # nddm_simulate_codes has no output for the external datum.  The datum is a function of (seed, set, Alpha, ext_sigma,
                    # ext_mode) and the transform alone -- not of the trials -- so a launch of one step-less trial per set writes the
                    # bits any launch would (first: last_launch() then describes the launch that simulates)
                    _lib.check(L.nddm_simulate_indirect(model, _ptr(p_dev), None, B, 1, float(dt), 0, seed, set_offset, _ptr(set_offset_dev),
                                                        _lib.GAUSS_FAST if fast else _lib.GAUSS_EXACT, float(ext_sigma), int(ext_mode),
                                                        None, None, _ptr(out_ext), st))
                rc = L.nddm_simulate_codes(model, _ptr(p_dev), *common[:-1], _ptr(set_offset_dev), flags, _ptr(out_codes), _ptr(out_trials),
                                           _ptr(out_summary), st)
            elif set_offset_dev is not None:
                rc = L.nddm_simulate_indirect(model, _ptr(p_dev), _ptr(b_dev), *common[:-1], set_offset_dev.data_ptr(), flags,
                                              float(ext_sigma), int(ext_mode), _ptr(out_trials), _ptr(out_summary), _ptr(out_ext), st)
            elif model in _PLAIN_ENTRY:
                rc = getattr(L, _PLAIN_ENTRY[model])(_ptr(p_dev), *common, _ptr(out_trials), _ptr(out_summary), st)
            elif model == ALPHA_NOT_SCALED:
                rc = L.nddm_alpha_not_scaled_simulate(_ptr(p_dev), *common, float(ext_sigma), int(ext_mode),
                                                      _ptr(out_trials), _ptr(out_summary), _ptr(out_ext), st)
            elif model == EXPLICIT_BOUNDARY:
                rc = L.nddm_explicit_boundary_simulate(_ptr(p_dev), _ptr(b_dev), *common, _ptr(out_trials),
                                                       _ptr(out_summary), st)
            else:
                raise ValueError("unknown model")
            _lib.check(rc)
            # the kernel reads p_dev / b_dev asynchronously: tie their lifetime to the stream
            p_dev.record_stream(torch.cuda.current_stream(dev))
            if b_dev is not None:
                b_dev.record_stream(torch.cuda.current_stream(dev))
    res = {"seed": seed, "set_offset": set_offset, "params": p_dev}
    for k, v in (("trials", out_trials), ("summary", out_summary), ("ext", out_ext), ("codes", out_codes)):
        if v is not None:
            res[k] = v
    return res


def simulratcliff(params, n_trials, seed=None, set_offset=None, fast=None, ext_sigma=0.0, ext_mode=0, want_trials=True, want_summary=True,
                  want_ext=False, out_trials=None, out_summary=None, stream_state=None, device=None):
    """The EXACT first-passage sampler the reference generates alpha_not_scaled's data with -- simulratcliff, pyhddmjagsutils.py:47-176
    as called at alpha_not_scaled.py:95-108 -- batched on the device (include/nddm.h: nddm_simulratcliff): no step size.

    params: [B, 6] (or [6]) = Nu, Alpha, Beta, Tau, Eta, Varsigma.  Returns a dict of device tensors: 'trials' f32 [B, n_trials, 2] =
    (y, acc) with y = +-(Tau + decision time), 'summary' f32 [B, 10], 'ext' f32 [B], plus 'seed' / 'set_offset' / 'params'.
    fast=False: the reference's series term by term, bit-equal to the test suite's CPU restatement (its section D).  fast (the default,
    as for simulate()): hardware log / exp / reciprocal and the same acceptance function from three terms of its series or of the
    series' Jacobi-dual form -- on 6e6 trials no response differs from fast=False and no response time by more than 1e-6 s
    (profiles/r6_ratcliff_agreement.txt), at twice the rate.

    What cannot be sampled is flagged, in both modes.  (1) Invalid rows: host arrays are refused here (ValueError: a non-finite column,
    Alpha <= 0, Varsigma <= 0, Beta outside [0, 1], Eta < 0); a device tensor is not read on the host, and the kernel gives such a row
    no trial -- every (y, acc) NaN, n_upper = n_lower = 0, n_missing = n_trials, moments NaN, 'ext' by its formula.  (2) The domain: the
    rejection step cannot accept once G = r mu / (D pi) on a sphere passes about 7 (r = Alpha min(Beta, 1 - Beta), mu the trial's
    drift, D = Varsigma^2 / 2); a trial that runs into the sampler's loop caps there is (NaN, NaN) and counted in n_missing, never
    returned as a number.  G below about 6 -- the generator's box (alpha_not_scaled.py:66-72) but for the drift's far tail at its
    extreme corner -- is in range; check summary[:, 2] (or isnan(y)) on rows beyond it."""
    torch = require_device()
    L = _lib.lib()
    dev = _device(device)
    rows = (2, 6, "params must have shape [B, 6] (Nu, Alpha, Beta, Tau, Eta, Varsigma)")
    p_np = _host_rows(params, *rows)
    if p_np is not None:
        validate_params_host(ALPHA_NOT_SCALED, p_np)
        if np.any(p_np[:, 2] < 0) or np.any(p_np[:, 2] > 1) or np.any(p_np[:, 4] < 0):
            raise ValueError("Beta must lie in [0, 1] and Eta must be >= 0")
    p_dev = _device_rows(params, p_np, dev, *rows)
    B, n_trials = int(p_dev.shape[0]), int(n_trials)
    if n_trials <= 0:
        raise ValueError("n_trials must be positive")
    seed, set_offset = _stream_position(seed, set_offset, stream_state, B)
    fast = DEFAULT_FAST if fast is None else bool(fast)
    with torch.cuda.device(dev):
        out_ext = torch.empty((B,), dtype=torch.float32, device=dev) if want_ext else None
        out_trials = _out_buffer(want_trials, out_trials, (B, n_trials, 2), dev)
        out_summary = _out_buffer(want_summary, out_summary, (B, SUMMARY_K), dev)
        if B > 0:
            _lib.check(L.nddm_simulratcliff(_ptr(p_dev), B, n_trials, seed, set_offset, _lib.GAUSS_FAST if fast else _lib.GAUSS_EXACT,
                                            float(ext_sigma), int(ext_mode), _ptr(out_trials), _ptr(out_summary), _ptr(out_ext),
                                            torch.cuda.current_stream(dev).cuda_stream))
            p_dev.record_stream(torch.cuda.current_stream(dev))
    res = {"seed": seed, "set_offset": set_offset, "params": p_dev}
    for k, v in (("trials", out_trials), ("summary", out_summary), ("ext", out_ext)):
        if v is not None:
            res[k] = v
    return res


def _wiener_check_params(model, p_np):
    """Range checks of host-side likelihood parameters (ValueError, before any device work)."""
    if not np.all(np.isfinite(p_np)):
        raise ValueError("parameters must be finite")
    a, beta, tau = p_np[:, 1], p_np[:, 2], p_np[:, 3]
    s = p_np[:, 4] if model == BASIC_DDM_DC else p_np[:, 5]
    if np.any(a <= 0) or np.any(s <= 0):
        raise ValueError("boundary and diffusion coefficient must be > 0")
    if np.any(beta <= 0) or np.any(beta >= 1):
        raise ValueError("beta must lie in (0, 1)")
    if np.any(tau < 0) or (model == ALPHA_NOT_SCALED and np.any(p_np[:, 4] < 0)):
        raise ValueError("tau and Eta must be >= 0")


def _marginal_check_params(p_np):
    """Range checks of host-side SINGLE_TRIAL parameters for the marginal likelihood (ValueError, before any device work)."""
    if not np.all(np.isfinite(p_np)):
        raise ValueError("parameters must be finite")
    if np.any(p_np[:, 4] <= 0) or np.any(p_np[:, 6] <= 0) or np.any(p_np[:, 5] <= 0):
        raise ValueError("std_alpha, sigma1 and dc must be > 0")
    if np.any(p_np[:, 2] <= 0) or np.any(p_np[:, 2] >= 1):
        raise ValueError("beta must lie in (0, 1)")
    if np.any(p_np[:, 3] < 0):
        raise ValueError("ter must be >= 0")


def _wiener_host_checks(model, params, data, draws_per_dataset, what, outputs, requests=False, marginal=False, cols=None):
    """The front end wiener_log_likelihood, wiener_cdf, wiener_quantile and wiener_marginal_log_likelihood share: host inputs are refused
    here (ValueError), before any device work; a device tensor's shape is checked where it is cast, after the split.  -> (S, params' and
    data's row descriptions, the host arrays or None, R).  `what`: the quantity the model would have to have a closed form of; `outputs`:
    the caller's output switches by name; `requests`: `data` holds wiener_quantile's (p, boundary code) pairs instead of trials;
    `marginal`: the caller integrates SINGLE_TRIAL's latent boundary out -- that model and no other, its columns and (choicert, z1) data;
    `cols`: the columns params has instead of the model's own (the marginal's 7-column rows, gamma = 1)."""
    if marginal:
        if model != SINGLE_TRIAL:
            raise ValueError(f"model {model} has no {what} here (SINGLE_TRIAL only)")
    elif model not in (BASIC_DDM_DC, ALPHA_NOT_SCALED):
        raise ValueError(f"model {model} has no closed-form {what} here (BASIC_DDM_DC and ALPHA_NOT_SCALED only)")
    if not any(outputs.values()):
        raise ValueError("ask for " + " and/or ".join(outputs))
    S = int(draws_per_dataset)
    if S <= 0:
        raise ValueError("draws_per_dataset must be > 0")
    P = NPARAMS[model] if cols is None else cols
    p_rows = (2, P, f"params must have shape [R, {P}]")
    d_rows = (3, 2, "probs must have shape [D, n, 2]" if requests else "data must have shape [D, n_trials, 2]")
    p_np = _host_rows(params, *p_rows)
    if p_np is not None:
        _marginal_check_params(p_np) if marginal else _wiener_check_params(model, p_np)
    d_np = _host_rows(data, *d_rows)
    if d_np is not None and requests:
        if not np.all(np.isin(d_np[..., 1], (-1.0, 0.0, 1.0))):
            raise ValueError("probs are (p, boundary code) with code in {1, -1, 0}")
        if not np.all((d_np[..., 0] >= 0) & (d_np[..., 0] <= 1)):
            raise ValueError("p must lie in [0, 1]")
    elif d_np is not None and model == BASIC_DDM_DC and not np.all(np.isin(d_np[..., 1], (-1.0, 0.0, 1.0))):
        raise ValueError("basic_ddm_dc data are (rt, choice) with choice in {1, -1, 0}")
    R = p_np.shape[0] if p_np is not None else (1 if params.ndim == 1 else int(params.shape[0]))
    D = d_np.shape[0] if d_np is not None else (1 if data.ndim == 2 else int(data.shape[0]))
    if R != D * S:
        raise ValueError(f"params has {R} rows but {'probs' if requests else 'data'} holds {D} {'request' if requests else 'data'} sets x "
                         f"draws_per_dataset {S}")
    return S, p_rows, d_rows, p_np, d_np, R


def _wiener_device_call(checked, params, data, device, outputs, call):
    """The device half wiener_log_likelihood, wiener_marginal_log_likelihood[_grad], wiener_log_likelihood_grad, wiener_cdf and
    wiener_quantile share.  `checked`: what _wiener_host_checks returned; `outputs`: (result key, wanted?, shape with None for n_trials, torch dtype's name)
    in the result's order; `call(L, params pointer, data pointer, n_trials, {key: output pointer or None}, stream handle)` makes the one
    library call and checks its status -- it is not called for an empty batch.  -> {key: device tensor} of the wanted outputs."""
    S, p_rows, d_rows, p_np, d_np, R = checked
    torch = require_device()
    L = _lib.lib()
    dev = _device(device)
    with torch.cuda.device(dev):
        p_dev = _device_rows(params, p_np, dev, *p_rows)
        d_dev = _device_rows(data, d_np, dev, *d_rows)
        N = int(d_dev.shape[1])
        res = {key: torch.empty(tuple(N if n is None else n for n in shape), dtype=getattr(torch, dtype), device=dev)
               for key, wanted, shape, dtype in outputs if wanted}
        if R > 0:
            st = torch.cuda.current_stream(dev)
            call(L, _ptr(p_dev), _ptr(d_dev), N, {key: _ptr(res.get(key)) for key, _, _, _ in outputs}, st.cuda_stream)
            p_dev.record_stream(st)
            d_dev.record_stream(st)
    return res


def wiener_log_likelihood(model, params, data, draws_per_dataset=1, per_trial=False, want_sum=True, device=None):
    """Log-likelihood of observed trials under the Wiener first-passage density (include/nddm.h: nddm_wiener_log_likelihood), one
    kernel launch: the density JAGS dwiener / Stan wiener_lpdf evaluate in the reference's likelihood-based fits.

    model: BASIC_DDM_DC (params [R, 5], data (rt, choice); choice 0 = a timeout, scored as log P(T > rt - tau)) or ALPHA_NOT_SCALED
    (params [R, 6], drift ~ N(Nu, Eta) integrated out, Nu clipped to +-5; data (y, acc), y == 0 gives NaN).  data: [D, n_trials, 2]
    in the simulator's output format, R = D * draws_per_dataset, row r scored against data set r // draws_per_dataset.
    Returns a dict of device tensors: 'loglik' float64 [R] (want_sum) and 'trial_logp' float32 [R, n_trials] (per_trial).
    Host arrays are shape- and range-checked (ValueError); device tensors go to the kernel as they are, where an invalid row gives NaN."""
    checked = _wiener_host_checks(model, params, data, draws_per_dataset, "likelihood", {"per_trial": per_trial, "want_sum": want_sum})
    S, R = checked[0], checked[-1]
    return _wiener_device_call(
        checked, params, data, device, [("loglik", want_sum, (R,), "float64"), ("trial_logp", per_trial, (R, None), "float32")],
        lambda L, p, d, N, o, st: _lib.check(L.nddm_wiener_log_likelihood(int(model), p, R, S, d, N, 0, o["trial_logp"], o["loglik"], st)))


def _marginal_cols(params):
    """7 for a DEVICE tensor whose last dimension is 7 (rows without gamma, gamma = 1: the flow's draws, which the kernel reads as they
    are instead of an [R, 8] copy); else None, the model's own 8 -- a host array has its gamma column appended on the host for free
    (single_trial_alpha_not_scaled._with_gamma) and keeps the one documented shape, whose check names a wrong one."""
    return 7 if getattr(params, "is_cuda", False) and params.dim() >= 1 and int(params.shape[-1]) == 7 else None


def _host_counts(counts, D, N):
    """Host-side trial counts per data set -> int32 [D], each in [1, N] (ValueError otherwise, as InvariantNetwork._set_counts refuses
    them): no device work."""
    c = np.asarray(counts.cpu() if hasattr(counts, "cpu") else counts)
    if c.ndim != 1 or c.shape[0] != D or not np.issubdtype(c.dtype, np.integer):
        raise ValueError(f"counts must be integers [D = {D}], got {c.dtype} {c.shape}")
    if np.any(c < 1) or np.any(c > N):
        raise ValueError(f"counts must lie in [1, n_trials = {N}]")
    return c.astype(np.int32)


def wiener_marginal_log_likelihood(model, params, data, draws_per_dataset=1, t_censor=None, per_trial=False, want_sum=True, device=None, counts=None):
    """Marginal log-likelihood of observed trials under the single-trial model, the latent per-trial boundary integrated out (include/nddm.h:
    nddm_wiener_marginal_log_likelihood), one kernel launch.

    model: SINGLE_TRIAL (params [R, 8] = drift, mu_alpha, beta, ter, std_alpha, dc, sigma1, gamma; data (choicert, z1)).  data: [D, n_trials,
    2] in the simulator's output format, R = D * draws_per_dataset, row r scored against data set r // draws_per_dataset.  t_censor: the
    decision time a timeout (choicert == 0) is censored at, the simulator's max_steps * dt; None: timeouts give NaN.
    Returns a dict of device tensors: 'loglik' float64 [R] (want_sum) and 'trial_logp' float32 [R, n_trials] (per_trial).
    Host arrays are shape- and range-checked (ValueError); device tensors go to the kernel as they are, where an invalid row gives NaN.

    A device tensor params [R, 7] (no gamma column: gamma = 1, the bits of the 8-column row with 1.0f; host arrays are [R, 8]) and counts (None, or a trial count per data set,
    integers [D]: set d's rows score its first counts[d] trials only, the data beyond are never read, 'trial_logp' is 0 there, and
    'loglik' has the bits of a call on that set alone at n_trials = counts[d]) go through nddm_wiener_marginal_log_likelihood_ragged, the
    same kernel instantiated for them; without either the call is the one above.  Host-side counts outside [1, n_trials] are refused
    (ValueError); a device tensor passes through, and a count outside gives NaN in that set's rows."""
    cols = _marginal_cols(params)
    checked = _wiener_host_checks(model, params, data, draws_per_dataset, "marginal likelihood", {"per_trial": per_trial, "want_sum": want_sum},
                                  marginal=True, cols=cols)
    S, R = checked[0], checked[-1]
    tc = 0.0 if t_censor is None else float(t_censor)
    if math.isnan(tc) or tc < 0:
        raise ValueError("t_censor must be >= 0 (or None: timeouts then give NaN)")
    outputs = [("loglik", want_sum, (R,), "float64"), ("trial_logp", per_trial, (R, None), "float32")]
    if cols is None and counts is None:
        return _wiener_device_call(
            checked, params, data, device, outputs,
            lambda L, p, d, N, o, st: _lib.check(L.nddm_wiener_marginal_log_likelihood(int(model), p, R, S, d, N, tc, 0, o["trial_logp"], o["loglik"],
                                                                                       st)))
    c_dev = None
    if counts is not None:
        D, N = R // S, int((checked[4] if checked[4] is not None else data).shape[-2])
        on_device = bool(getattr(counts, "is_cuda", False))
        if on_device and (counts.dim() != 1 or counts.shape[0] != D or counts.is_floating_point()):
            raise ValueError(f"counts must be an integer tensor [D = {D}], got {counts.dtype} {tuple(counts.shape)}")
        c_host = None if on_device else _host_counts(counts, D, N)      # refused here, before any device work
        torch = require_device()
        dev = _device(device)
        c_dev = counts.to(dev, torch.int32).contiguous() if on_device else torch.as_tensor(c_host, device=dev)

    def call(L, p, d, N, o, st):
        _lib.check(L.nddm_wiener_marginal_log_likelihood_ragged(int(model), p, 8 if cols is None else cols, R, S, d, N, _ptr(c_dev), tc, 0,
                                                                o["trial_logp"], o["loglik"], st))
        if c_dev is not None:
            c_dev.record_stream(require_device().cuda.current_stream(c_dev.device))
    return _wiener_device_call(checked, params, data, device, outputs, call)


WHMC_STATE, WHMC_MAX_TRIALS, WHMC_MAX_ROUNDS = 12, 2048, 1 << 19


def wiener_hmc_max_iter(n_trials, n_leapfrog):
    """The most iterations one nddm_wiener_hmc launch may run: n_iter * n_leapfrog * ceil(n_trials / 64) <= 2^19."""
    return max(WHMC_MAX_ROUNDS // (int(n_leapfrog) * ((int(n_trials) + 63) // 64)), 0)


def _hmc_host_checks(model, data, sets, n_iter, n_adapt, n_leapfrog, thin, free_mask, chain_offset, iter_offset, max_iter_of, bound,
                     chains_per_dataset=None, censored=False):
    """The front end wiener_hmc and wiener_hmc_joint share, up to the launch bound: host inputs are refused here (ValueError), before any
    device work.  sets: the letter of data's first axis; max_iter_of / bound: the sampler's launch bound and its sentence ({m}: the bound,
    {N}, {L}); chains_per_dataset: wiener_hmc's; censored: timeouts (choice 0) are trials.  -> (the counts, mask and offsets as ints, data's row description, its host array or None,
    the number of data sets, n_trials)."""
    if model != BASIC_DDM_DC:
        raise ValueError(f"model {model} has no sampler here (BASIC_DDM_DC only)")
    if chains_per_dataset is not None and int(chains_per_dataset) <= 0:
        raise ValueError("chains_per_dataset must be > 0")
    n_iter, n_adapt, n_leapfrog, thin, free_mask = (int(x) for x in (n_iter, n_adapt, n_leapfrog, thin, free_mask))
    if n_iter <= 0 or n_leapfrog <= 0 or thin <= 0 or n_adapt < 0:
        raise ValueError("n_iter, n_leapfrog and thin must be > 0 and n_adapt >= 0")
    if not 0 <= free_mask < 32:
        raise ValueError("free_mask has five bits")
    chain_offset, iter_offset = int(chain_offset), int(iter_offset)
    if chain_offset < 0 or iter_offset < 0 or iter_offset + n_iter > 1 << 32:
        raise ValueError("chain_offset and iter_offset must be >= 0 and the iteration index < 2^32")
    d_rows = (3, 2, f"data must have shape [{sets}, n_trials, 2]")
    d_np = _host_rows(data, *d_rows)
    if d_np is not None:
        if not np.all(np.isfinite(d_np)):
            raise ValueError("data must be finite")
        if censored and not np.all(np.isin(d_np[..., 1], (-1.0, 0.0, 1.0))):
            raise ValueError("with censored=True the sampler takes (rt, choice) with choice in {1, -1, 0}")
        if not censored and not np.all(np.isin(d_np[..., 1], (-1.0, 1.0))):
            raise ValueError("the sampler takes (rt, choice) with choice in {1, -1}: a timeout (choice 0) has no gradient here")
        if np.any(d_np[..., 0] <= 0):
            raise ValueError("response times must be > 0")
    D, N = (int(d_np.shape[0]), int(d_np.shape[1])) if d_np is not None else \
        ((1, int(data.shape[0])) if data.ndim == 2 else (int(data.shape[0]), int(data.shape[1])))
    if N > WHMC_MAX_TRIALS:
        raise ValueError(f"n_trials must be <= {WHMC_MAX_TRIALS}")
    if n_iter > max_iter_of(N, n_leapfrog):
        raise ValueError(bound.format(m=max_iter_of(N, n_leapfrog), N=N, L=n_leapfrog))
    return (n_iter, n_adapt, n_leapfrog, thin, free_mask, chain_offset, iter_offset), d_rows, d_np, D, N


def _hmc_f64(x, shape, label, note=""):
    """A sampler's float64 input of a given shape: a device tensor is checked and left where it is (-> None), anything else -> its host
    array."""
    if getattr(x, "is_cuda", False):
        if tuple(x.shape) != shape or str(x.dtype) != "torch.float64" or not x.is_contiguous():
            raise ValueError(f"{label} must be a contiguous float64 {list(shape)}")
        return None
    a = np.ascontiguousarray(x, dtype=np.float64)
    if a.shape != shape:
        raise ValueError(f"{label} must have shape {list(shape)}{note}, got {a.shape}")
    return a


def _hmc_chain_checks(C, chain_offset, state, inv_mass, note="", own=lambda: {}):
    """The chain index, then the sampler's `own` inputs (-> {name: (value, host array or None)}), state [C, 12] and inv_mass [C, 5] or None
    -> the float64 inputs {name: (value, host array or None)}, the sampler's own first."""
    if chain_offset + C > 1 << 32:
        raise ValueError("the chain index must stay < 2^32")
    f64 = own()
    s_np = _hmc_f64(state, (C, WHMC_STATE), "state", note)
    if s_np is not None and not np.all(np.isfinite(s_np[:, :10])):
        raise ValueError("state must be finite")
    m_np = None if inv_mass is None else _hmc_f64(inv_mass, (C, 5), "inv_mass", note)
    if m_np is not None and not (np.all(np.isfinite(m_np)) and np.all(m_np > 0)):
        raise ValueError("inv_mass must be finite and > 0")
    return dict(f64, state=(state, s_np), inv_mass=(inv_mass, m_np))


def _hmc_device_call(data, d_rows, d_np, f64, C, K, want_draws, want_log_post, own, device, call, always=False):
    """The device half the two samplers share.  f64: _hmc_chain_checks' inputs; own: (key, shape, torch dtype's name) of the sampler's
    further buffers; call(L, data pointer, {name: input pointer}, {key: output pointer or None}, stream handle) makes the one library call and
    checks its status -- for no chain only if `always`.  -> ({key: device tensor} of the wanted outputs and `own`, {name: device tensor}
    of the inputs)."""
    torch = require_device()
    L = _lib.lib()
    dev = _device(device)
    with torch.cuda.device(dev):
        d_dev = _device_rows(data, d_np, dev, *d_rows)
        ins = {k: x if a is None else torch.as_tensor(a, dtype=torch.float64).to(dev) for k, (x, a) in f64.items()}
        res = {key: torch.empty(shape, dtype=getattr(torch, dtype), device=dev) if wanted else None for key, wanted, shape, dtype in
               [("draws", want_draws, (C, K, 5), "float32"), ("log_post", want_log_post, (C, K), "float32"), ("accept", True, (C,), "float32"),
                ("divergent", True, (C,), "int32"), ("flagged", True, (C,), "int32")] + [(key, True, shape, dtype) for key, shape, dtype in own]}
        if C > 0 or always:
            st = torch.cuda.current_stream(dev)
            call(L, _ptr(d_dev), {k: _ptr(v) for k, v in ins.items()}, {k: _ptr(v) for k, v in res.items()}, st.cuda_stream)
            for t in (d_dev, *ins.values(), *(res[key] for key, _, _ in own)):
                if t is not None:
                    t.record_stream(st)
    return {k: v for k, v in res.items() if v is not None}, ins


def wiener_hmc(model, data, state, chains_per_dataset=1, inv_mass=None, n_iter=1, n_adapt=0, n_leapfrog=16, thin=1, free_mask=31, seed=0,
               chain_offset=0, iter_offset=0, want_draws=True, want_log_post=True, device=None, censored=False):
    """Batched Hamiltonian Monte Carlo over the basic_ddm_dc Wiener posterior, one wave per chain, all n_iter iterations in ONE launch
    (include/nddm.h: nddm_wiener_hmc; the chain: csrc/nddm_wiener_hmc.h).

    model: BASIC_DDM_DC only.  data: [D, n_trials, 2] = (rt, choice), n_trials <= 2048.  state: float64 [C, 12], C = D *
    chains_per_dataset, chain c on data set c // chains_per_dataset (mcmc.make_state builds one; a device tensor is updated in place).
    inv_mass: float64 [C, 5] or None (ones).  One launch is bounded: n_iter <= wiener_hmc_max_iter(n_trials, n_leapfrog); mcmc.hmc_fit
    cuts a long run into such launches.  Returns a dict of device tensors: 'draws' float32 [C, K, 5] in the model's columns, 'log_post'
    float32 [C, K], 'accept' float32 [C], 'divergent' int32 [C], 'flagged' int32 [C] and 'state' float64 [C, 12]; K = (iter_offset +
    n_iter) // thin - iter_offset // thin.  Host inputs are shape- and range-checked (ValueError); a data set that cannot be sampled (a
    timeout, a non-finite value, an rt <= 0) that arrives on the device flags its chains instead.
    censored=True (NDDM_WIENER_CENSORED): timeouts (choice 0) are scored right-censored, log P(T > rt - tau), in the posterior and its
    gradient; tau's upper limit is min(1.5, the smallest rt of the RESPONSES).  With no timeout in the data the chains' bits are the default's."""
    (n_iter, n_adapt, n_leapfrog, thin, free_mask, chain_offset, iter_offset), d_rows, d_np, D, N = _hmc_host_checks(
        model, data, "D", n_iter, n_adapt, n_leapfrog, thin, free_mask, chain_offset, iter_offset, wiener_hmc_max_iter,
        "one launch runs at most {m} iterations at n_trials {N} and n_leapfrog {L} (n_iter * n_leapfrog * ceil(n_trials / 64) <= 2^19): cut the "
        "run (mcmc.hmc_fit does)", chains_per_dataset=chains_per_dataset, censored=censored)
    flags = _lib.WIENER_CENSORED if censored else 0
    S, K = int(chains_per_dataset), (iter_offset + n_iter) // thin - iter_offset // thin
    C = D * S
    f64 = _hmc_chain_checks(C, chain_offset, state, inv_mass, f" (D {D} x chains_per_dataset {S})")
    res, ins = _hmc_device_call(
        data, d_rows, d_np, f64, C, K, want_draws, want_log_post, [], device,
        lambda L, d, i, o, st: _lib.check(L.nddm_wiener_hmc(int(model), d, D, N, C, S, i["state"], i["inv_mass"], n_iter, n_adapt, n_leapfrog, thin,
                                                            free_mask, _u64(seed), chain_offset, iter_offset, flags, o["draws"], o["log_post"],
                                                            o["accept"], o["divergent"], o["flagged"], st)))
    res["state"] = ins["state"]
    return res


WHMCJ_MAX_ITER = 4096


def wiener_hmc_joint_max_iter(n_trials, n_leapfrog):
    """The most joint iterations one nddm_wiener_hmc_joint call may run: wiener_hmc_max_iter's bound and 4096 (two launches an iteration)."""
    return min(wiener_hmc_max_iter(n_trials, n_leapfrog), WHMCJ_MAX_ITER)


def wiener_hmc_joint(model, data, extdata, state, sigma, inv_mass=None, n_iter=1, n_adapt=0, n_leapfrog=16, thin=1, free_mask=31, seed=0,
                     chain_offset=0, iter_offset=0, sigma_fixed=False, want_draws=True, want_log_post=True, device=None, censored=False):
    """The alpha_not_scaled JAGS fit's sampler: wiener_hmc's chains coupled by one shared sigma, Metropolis within Gibbs (include/nddm.h:
    nddm_wiener_hmc_joint; csrc/nddm_wiener_hmc_joint.h).  Per joint iteration one participant launch and one sigma launch are enqueued on
    the current stream; nothing waits on the host.

    model: BASIC_DDM_DC only.  data: [P, n_trials, 2] = (rt, choice), one data set per participant.  extdata: float64 [P], ext_p ~
    N(boundary_p, sigma).  sigma: float64 [S], one per joint chain, in (0, 10) (any value > 0 with sigma_fixed).  state: float64 [P * S, 12],
    participant chain c = p * S + k; inv_mass: float64 [P * S, 5] or None.  Device tensors for state and sigma are updated in place.
    n_iter <= wiener_hmc_joint_max_iter(n_trials, n_leapfrog).  Returns wiener_hmc's dict -- 'log_post' is the participant's conditional
    log posterior given sigma, the ext term included -- plus 'sigma_draws' float32 [S, K], 'sigma_accept' float32 [S] (the share of the
    call's sigma proposals accepted; NaN with sigma_fixed) and 'sigma' float64 [S].  Host inputs are shape- and range-checked (ValueError);
    on the device a data set that cannot be sampled flags every chain, a bad state or sigma its joint chain.  censored=True: wiener_hmc's,
    passed through to the participants' chains."""
    (n_iter, n_adapt, n_leapfrog, thin, free_mask, chain_offset, iter_offset), d_rows, d_np, P, N = _hmc_host_checks(
        model, data, "P", n_iter, n_adapt, n_leapfrog, thin, free_mask, chain_offset, iter_offset, wiener_hmc_joint_max_iter,
        "one call runs at most {m} joint iterations at n_trials {N} and n_leapfrog {L} (n_iter <= 4096 and n_iter * n_leapfrog * ceil(n_trials / "
        "64) <= 2^19): cut the run (mcmc.hmc_fit_joint does)", censored=censored)
    flags = (_lib.HMC_SIGMA_FIXED if sigma_fixed else 0) | (_lib.WIENER_CENSORED if censored else 0)
    if not sigma_fixed and P < 2:
        raise ValueError("sampling sigma needs at least 2 participants")
    g_shape = tuple(sigma.shape) if hasattr(sigma, "shape") else np.shape(sigma)
    if len(g_shape) != 1 or g_shape[0] < 1:
        raise ValueError(f"sigma must have shape [S] with S >= 1 joint chains, got {g_shape}")
    S, K = int(g_shape[0]), (iter_offset + n_iter) // thin - iter_offset // thin
    C = P * S

    def own():
        g_np = _hmc_f64(sigma, (S,), "sigma")
        if g_np is not None and not (np.all(np.isfinite(g_np)) and np.all(g_np > 0) and (sigma_fixed or np.all(g_np < 10))):
            raise ValueError("sigma must be finite and > 0, and < 10 when it is sampled")
        e_np = _hmc_f64(extdata, (P,), "extdata")
        if e_np is not None and not np.all(np.isfinite(e_np)):
            raise ValueError("extdata must be finite")
        return {"extdata": (extdata, e_np), "sigma": (sigma, g_np)}
    f64 = _hmc_chain_checks(C, chain_offset, state, inv_mass, own=own)
    res, ins = _hmc_device_call(
        data, d_rows, d_np, f64, C, K, want_draws, want_log_post,
        [("sigma_draws", (S, K), "float32"), ("sigma_accept", (S,), "float32"), ("workspace", (C + S, 4), "float64")], device,
        lambda L, d, i, o, st: _lib.check(L.nddm_wiener_hmc_joint(
            int(model), d, P, N, C, S, i["extdata"], i["state"], i["inv_mass"], i["sigma"], o["workspace"], n_iter, n_adapt, n_leapfrog, thin,
            free_mask, _u64(seed), chain_offset, iter_offset, flags, o["draws"], o["log_post"], o["accept"],
            o["divergent"], o["flagged"], o["sigma_draws"], o["sigma_accept"], st)), always=True)
    del res["workspace"]
    res["state"], res["sigma"] = ins["state"], ins["sigma"]
    return res


# kernel launches wiener_log_likelihood_grad has made in this process (tests count them: one per forward plus backward)
_WIENER_GRAD_LAUNCHES = [0]


def wiener_grad_launches():
    """Developer aid: how many launches wiener_log_likelihood_grad has made in this process."""
    return _WIENER_GRAD_LAUNCHES[0]


def wiener_log_likelihood_grad(model, params, data, draws_per_dataset=1, device=None, censored=False):
    """Log-likelihood of observed trials under the Wiener first-passage density AND its gradient in the parameter columns, one kernel
    launch (include/nddm.h: nddm_wiener_log_likelihood_grad): what a gradient-based fit consumes per step.  The arguments of
    wiener_log_likelihood.  Returns {'loglik': float64 [R], 'grad': float64 [R, P]} on the device; 'loglik' has the bits of
    wiener_log_likelihood's.  alpha_not_scaled's Nu is clipped to +-5: where the clip is active d/dNu is 0.

    An invalid row gives NaN in both; a trial at or below tau (-inf in the value) or an alpha_not_scaled y == 0 gives a NaN gradient.
    basic_ddm_dc's censored timeouts (choice 0) are scored in 'loglik' exactly as wiener_log_likelihood scores them, either way.
    censored=False (the default, every bit as it was) -- NOT IMPLEMENTED there: such a row's gradient is NaN in every column, never a
    partial gradient.  censored=True (NDDM_WIENER_CENSORED, BASIC_DDM_DC only: ValueError otherwise): a timeout adds the gradient of
    log P(T > rt - tau) and the row's gradient is finite; a timeout with rt <= tau adds zero; a non-finite rt or a choice other than
    1, -1, 0 gives a NaN gradient.  With no timeout in the data the two give the same bits.
    Host arrays are shape- and range-checked (ValueError); device tensors go to the kernel as they are."""
    checked = _wiener_host_checks(model, params, data, draws_per_dataset, "likelihood", {"grad": True})
    if censored and model != BASIC_DDM_DC:
        raise ValueError("censored=True takes BASIC_DDM_DC only (alpha_not_scaled's y == 0 carries no time)")
    S, R = checked[0], checked[-1]
    flags = _lib.WIENER_CENSORED if censored else 0

    def call(L, p, d, N, o, st):
        _lib.check(L.nddm_wiener_log_likelihood_grad(int(model), p, R, S, d, N, flags, o["loglik"], o["grad"], st))
        _WIENER_GRAD_LAUNCHES[0] += 1

    return _wiener_device_call(checked, params, data, device,
                               [("loglik", True, (R,), "float64"), ("grad", True, (R, NPARAMS[model]), "float64")], call)


def wiener_marginal_log_likelihood_grad(model, params, data, draws_per_dataset=1, t_censor=None, device=None):
    """Marginal log-likelihood of observed trials under the single-trial model AND its gradient in the eight parameter columns, one kernel
    launch (include/nddm.h: nddm_wiener_marginal_log_likelihood_grad): what a gradient-based fit of this model consumes per step.  The
    arguments of wiener_marginal_log_likelihood.  Returns {'loglik': float64 [R], 'grad': float64 [R, 8]} on the device, the columns in
    params' order (drift, mu_alpha, beta, ter, std_alpha, dc, sigma1, gamma); 'loglik' has the bits of wiener_marginal_log_likelihood's.

    A timeout (choicert 0) with t_censor > 0 HAS a gradient: a valid row of valid trials, timeouts included, gets a finite one.  An invalid
    row gives NaN in both; |choicert| <= ter (-inf in the value), a timeout without t_censor, a non-finite z1 or a NaN choicert give NaN in
    every gradient column of their row.  Host arrays are shape- and range-checked (ValueError); device tensors go to the kernel as they are."""
    checked = _wiener_host_checks(model, params, data, draws_per_dataset, "marginal likelihood", {"grad": True}, marginal=True)
    S, R = checked[0], checked[-1]
    tc = 0.0 if t_censor is None else float(t_censor)
    if math.isnan(tc) or tc < 0:
        raise ValueError("t_censor must be >= 0 (or None: timeouts then give NaN)")

    def call(L, p, d, N, o, st):
        _lib.check(L.nddm_wiener_marginal_log_likelihood_grad(int(model), p, R, S, d, N, tc, 0, o["loglik"], o["grad"], st))
        _WIENER_MARGINAL_GRAD_LAUNCHES[0] += 1

    return _wiener_device_call(checked, params, data, device, [("loglik", True, (R,), "float64"), ("grad", True, (R, NPARAMS[model]), "float64")], call)


# kernel launches wiener_marginal_log_likelihood_grad has made in this process (tests count them: one per forward plus backward)
_WIENER_MARGINAL_GRAD_LAUNCHES = [0]


def wiener_marginal_grad_launches():
    """Developer aid: how many launches wiener_marginal_log_likelihood_grad has made in this process."""
    return _WIENER_MARGINAL_GRAD_LAUNCHES[0]


def wiener_cdf(model, params, data, draws_per_dataset=1, want_cdf=True, want_p_upper=True, device=None):
    """Distribution function of observed trials under the Wiener first-passage law and the choice probability (include/nddm.h:
    nddm_wiener_cdf), one kernel launch: RWiener / HDDM pwiener, the companion of wiener_log_likelihood, whose arguments these are.

    Returns a dict of float32 device tensors: 'cdf' [R, n_trials] (want_cdf) = P(T <= rt - tau, the boundary the trial ended on), the
    defective distribution function -- 0 for rt <= tau; a basic_ddm_dc timeout (choice 0) gives P(T <= rt - tau) over both boundaries,
    an alpha_not_scaled y == 0 NaN -- and 'p_upper' [R] (want_p_upper) = P(upper boundary), drift variability integrated out.
    Host arrays are shape- and range-checked (ValueError); device tensors go to the kernel as they are, where an invalid row gives NaN."""
    checked = _wiener_host_checks(model, params, data, draws_per_dataset, "distribution function",
                                  {"want_cdf": want_cdf, "want_p_upper": want_p_upper})
    S, R = checked[0], checked[-1]
    return _wiener_device_call(
        checked, params, data, device, [("cdf", want_cdf, (R, None), "float32"), ("p_upper", want_p_upper, (R,), "float32")],
        lambda L, p, d, N, o, st: _lib.check(L.nddm_wiener_cdf(int(model), p, R, S, d, N, 0, o["cdf"], o["p_upper"], st)))


def wiener_quantile(model, params, probs, draws_per_dataset=1, conditional=False, device=None):
    """Quantile function of the Wiener first-passage law (include/nddm.h: nddm_wiener_quantile), one kernel launch: RWiener / HDDM
    qwiener, the inverse of wiener_cdf, whose model, params and draws_per_dataset these are.

    probs: [D, n, 2] (or [n, 2]) = (p, boundary code) -- code 1 the upper boundary, -1 the lower one, 0 either boundary; R = D *
    draws_per_dataset, row r answers request set r // draws_per_dataset.  conditional=False: p is DEFECTIVE, the response time rt with
    P(T <= rt - tau, boundary) = p (NaN for a p beyond the boundary's probability, +inf at it); conditional=True: p is the share of that
    boundary's responses, P(T <= rt - tau, boundary) = p P(boundary) (+inf at p = 1).  p = 0 gives tau.
    Returns {'quantile': float32 [R, n]} on the device.  Host arrays are shape- and range-checked (ValueError: code in {1, -1, 0}, p in
    [0, 1]); device tensors go to the kernel as they are, where an invalid row, a NaN or a negative p give NaN."""
    checked = _wiener_host_checks(model, params, probs, draws_per_dataset, "distribution function", {"quantile": True}, requests=True)
    S, R = checked[0], checked[-1]
    flags = _lib.QUANTILE_CONDITIONAL if conditional else 0
    return _wiener_device_call(
        checked, params, probs, device, [("quantile", True, (R, None), "float32")],
        lambda L, p, d, N, o, st: _lib.check(L.nddm_wiener_quantile(int(model), p, R, S, d, N, flags, o["quantile"], st)))


def decode_codes(model, codes, params, dt, out_trials=None):
    """The 2-byte wire format back to the float pairs the simulator writes: codes int16 [B, n_trials] (uint16 content), params
    f32 [B, P] (tau is read from them), -> f32 [B, n_trials, 2], bit-identical to simulate()'s 'trials' (nddm_decode_codes)."""
    torch = require_device()
    B, n_trials = int(codes.shape[0]), int(codes.shape[1])
    if out_trials is None:
        out_trials = torch.empty((B, n_trials, 2), dtype=torch.float32, device=codes.device)
    p = params.to(dtype=torch.float32).contiguous()
    with torch.cuda.device(codes.device):
        _lib.check(_lib.lib().nddm_decode_codes(model, codes.contiguous().data_ptr(), p.data_ptr(), B, n_trials, float(dt),
                                                out_trials.data_ptr(), torch.cuda.current_stream(codes.device).cuda_stream))
    return out_trials


def draw_prior_device(model, batch_size, seed=0, set_offset=0, gamma=1.0, device=None, set_offset_dev=None, out=None):
    """On-device batched draw_prior (basic_ddm_dc.py:62-80 / single_trial_alpha_not_scaled.py:78-102): f32 [B, P].
    set_offset_dev: as in simulate() (nddm_draw_prior_indirect)."""
    torch = require_device()
    L = _lib.lib()
    dev = _device(device)
    P = NPARAMS[model]
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty((int(batch_size), P), dtype=torch.float32, device=dev)
        position = (model, int(batch_size), _u64(seed), _u64(set_offset))
        rest = (float(gamma), out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        if set_offset_dev is not None:
            _lib.check(L.nddm_draw_prior_indirect(*position, set_offset_dev.data_ptr(), *rest))
        else:
            _lib.check(L.nddm_draw_prior(*position, *rest))
    return out


PINNED_FROM_BYTES = 1 << 20
# NDDM_PINNED_RESULTS=0 (or engine.PINNED_RESULTS = False): results come back in ordinary pageable memory (`.cpu()`), for callers
# that KEEP many large results -- see to_host()
PINNED_RESULTS = os.environ.get("NDDM_PINNED_RESULTS", "1") not in ("0", "false", "no")


def _pinned(pinned):
    return PINNED_RESULTS if pinned is None else bool(pinned)


def release_pinned_cache():
    """Hand the pinned host blocks of results that were dropped back to the OS (PyTorch caches them for reuse otherwise)."""
    torch = _torch()
    fn = getattr(torch._C, "_host_emptyCache", None)
    if fn is not None:
        fn()
        return True
    return False


def to_host(t, pinned=None):
    """Device tensor -> NumPy array (what the adapters' `as_numpy` forms return).  A result of a megabyte or more goes through
    PINNED host memory: the copy then runs at the link's rate (53 GB/s measured on the MI355X box against 6.4 GB/s into pageable
    memory -- 2.4 GB of trials in 45 ms instead of 380, `profiles/r4_pcie_rate.txt`).  The array owns its block (it returns to
    PyTorch's pinned-memory cache when the array is dropped).

    What that costs: PyTorch's pinned allocator rounds a block up to a power of two (the 2.4 GB headline result pins 4 GB) and
    keeps dropped blocks cached, so a caller that holds on to MANY large results (imputation loops, generate_data) can run out of
    lockable memory where `.cpu()` would not.  `pinned=False` / NDDM_PINNED_RESULTS=0 selects the pageable path;
    release_pinned_cache() returns the cached blocks of dropped results to the OS."""
    torch = _torch()
    if not isinstance(t, torch.Tensor):
        return np.asarray(t)
    if not t.is_cuda:
        return t.numpy()
    if t.numel() * t.element_size() < PINNED_FROM_BYTES or not _pinned(pinned):
        return t.cpu().numpy()
    h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    h.copy_(t)
    return h.numpy()


HOST_CHUNK_BYTES = 128 << 20


def simulate_to_host(model, params, n_trials, seed=None, set_offset=None, stream_state=None, bounds=None, want_trials=True,
                     want_summary=True, want_ext=False, device=None, chunk_bytes=None, pinned=None, **kw):
    """simulate() for a caller who wants NumPy arrays back (the adapters' `as_numpy` forms): {'trials', 'summary', 'ext'} as
    float32 arrays in pinned host memory (pinned=False / NDDM_PINNED_RESULTS=0: pageable memory, see to_host), plus 'seed' /
    'set_offset'.

    A small batch is one launch and one copy.  A large one (more than `chunk_bytes` of trials, default 128 MB) is simulated in
    CHUNKS of parameter sets, and every chunk's results travel to the host on a second stream while the next chunk is simulated:
    the sets' random streams are keyed by their global index (set_offset + row), so the chunks reproduce the one launch bit for
    bit, the device holds two chunks instead of the whole result, and the 2.4 GB of the 1M x 300 workload are on the host
    47 ms after the call instead of 77 (one launch, then the copy) or 400 (`.cpu()`): profiles/r4_pcie_rate.txt."""
    torch = require_device()
    dev = _device(device)
    rows = _SIM_ROWS[model]
    p_np = _host_rows(params, *rows)
    if p_np is not None:
        validate_params_host(model, p_np)
    params = _device_rows(params, p_np, dev, *rows)
    B, n_trials = int(params.shape[0]), int(n_trials)
    seed, set_offset = _stream_position(seed, set_offset, stream_state, B)
    # a missing `bounds` is left to simulate(), which refuses it in its own order of checks
    if model == EXPLICIT_BOUNDARY and bounds is not None:
        bounds = _bounds_device(bounds, B, n_trials, dev)
    want_ext = bool(want_ext and model == ALPHA_NOT_SCALED)
    row_bytes = n_trials * 8 if want_trials else 4 * SUMMARY_K
    chunk_bytes = HOST_CHUNK_BYTES if chunk_bytes is None else int(chunk_bytes)
    rows = B if B * row_bytes <= chunk_bytes or not want_trials else max(1, chunk_bytes // row_bytes)
    common = dict(seed=seed, want_trials=want_trials, want_summary=want_summary, want_ext=want_ext, device=dev, **kw)
    res = {"seed": seed, "set_offset": set_offset}
    if rows >= B:                                            # one launch, one copy per output
        r = simulate(model, params, n_trials, set_offset=set_offset, bounds=bounds, **common)
        for k in ("trials", "summary", "ext"):
            if k in r:
                res[k] = to_host(r[k], pinned)
        return res
    with torch.cuda.device(dev):
        pin = lambda *shape: torch.empty(shape, dtype=torch.float32, pin_memory=_pinned(pinned))
        host = {"trials": pin(B, n_trials, 2) if want_trials else None, "summary": pin(B, SUMMARY_K) if want_summary else None,
                "ext": pin(B) if want_ext else None}
        cur, side = torch.cuda.current_stream(dev), torch.cuda.Stream(device=dev)
        bufs, copied = [None, None], [None, None]
        for c, lo in enumerate(range(0, B, rows)):
            hi, b = min(B, lo + rows), c & 1
            if copied[b] is not None:
                cur.wait_event(copied[b])                   # this buffer set's previous chunk is on the host
            if bufs[b] is None:
                bufs[b] = {"trials": torch.empty((rows, n_trials, 2), dtype=torch.float32, device=dev) if want_trials else None,
                           "summary": torch.empty((rows, SUMMARY_K), dtype=torch.float32, device=dev) if want_summary else None}
            n = hi - lo
            tr = bufs[b]["trials"][:n] if want_trials else None
            sm = bufs[b]["summary"][:n] if want_summary else None
            r = simulate(model, params[lo:hi], n_trials, set_offset=_u64(set_offset + lo),
                         bounds=None if bounds is None else bounds[lo:hi], out_trials=tr, out_summary=sm, **common)
            ev = torch.cuda.Event()
            ev.record(cur)
            side.wait_event(ev)
            with torch.cuda.stream(side):
                for k in ("trials", "summary", "ext"):
                    if host[k] is not None:
                        host[k][lo:hi].copy_(r[k], non_blocking=True)
                        r[k].record_stream(side)
                copied[b] = torch.cuda.Event()
                copied[b].record(side)
        side.synchronize()
    for k, h in host.items():
        if h is not None:
            res[k] = h.numpy()
    return res


def debug_normals(counters, k0, k1, fast=False, raw=False, form=None):
    """4 normals per Philox counter row (tests compare these with the oracle's).
    raw=True: the transform's own factors instead (include/nddm.h: NDDM_DEBUG_RAW) -- [n, 6] = r0, cos0, sin0, r1, cos1, sin1 with the
    radius in noise units, in the form the auxiliary stream evaluates (form=None or "aux"), the step loop's (form="hot"), or [n, 12]
    for the four pairs of the packed layout (form="packed").
    counters: anything np.asarray takes, or an int32 device tensor [n, 4] holding the words' bits."""
    torch = require_device()
    if form not in (None, "aux", "hot", "packed"):
        raise ValueError(f"debug_normals: form={form!r} (None, 'aux', 'hot' or 'packed')")
    if form is not None and not raw:
        raise ValueError("debug_normals: form= selects a form of the raw dump (raw=True)")
    if isinstance(counters, torch.Tensor):
        if counters.dtype != torch.int32 or counters.dim() != 2 or counters.shape[1] != 4:
            raise ValueError("debug_normals: a counter tensor is int32 [n, 4]")
        c = counters.cuda().contiguous()
    else:
        c = torch.as_tensor(np.asarray(counters, dtype=np.uint32).view(np.int32)).cuda().contiguous()
    n = c.shape[0]
    flags = 1 if fast else 0
    width = 4
    if raw:
        flags |= _lib.DEBUG_RAW | {"hot": _lib.DEBUG_HOT, "packed": _lib.DEBUG_PACKED}.get(form, 0)
        width = 12 if form == "packed" else 6
    out = torch.empty((n, width), dtype=torch.float32, device=c.device)
    rc = _lib.lib().nddm_debug_normals(c.data_ptr(), n, int(k0), int(k1), flags, out.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream)
    _lib.check(rc)
    return out.cpu().numpy()


class debug_trace:
    """Developer aid (profiling): `with debug_trace() as t: simulate(...)`, then `t.read()`.  While active, every wave of
    the simulator kernels stores one record {step-loop blocks, refill phases, s_memtime cycles, lifetime / start / queue
    found empty / end in 100 MHz ticks} and, with chunks > 0, the tick at which each chunk was pulled from the work queue
    (include/nddm.h: nddm_set_debug_trace; plain stores, so the traced launch runs like any other)."""

    def __init__(self, waves=16384, chunks=0, device=None):
        torch = require_device()
        self.waves, self.chunks = int(waves), int(chunks)
        dev = _device(device)
        self.buf = torch.zeros(8 * self.waves + self.chunks, dtype=torch.int64, device=dev)

    def __enter__(self):
        _lib.check(_lib.lib().nddm_set_debug_trace(self.buf.data_ptr(), self.waves, self.chunks))
        return self

    def __exit__(self, *exc):
        require_device().cuda.synchronize()
        _lib.lib().nddm_set_debug_trace(None, 0, 0)
        return False

    def read(self):
        """dict: totals over the waves that ran (blocks, refills, cycles, ticks, waves), the per-wave records [n, 8] and
        the chunks' pull ticks."""
        d = self.buf.cpu().numpy()
        rec = d[:8 * self.waves].reshape(self.waves, 8)
        rec = rec[rec[:, 7] == 1]
        pulls = d[8 * self.waves:]
        return {"blocks": float(rec[:, 0].sum()), "refills": float(rec[:, 1].sum()), "cycles": float(rec[:, 2].sum()),
                "ticks": float(rec[:, 3].sum()), "waves": int(rec.shape[0]), "records": rec, "pulls": pulls[pulls > 0]}


def release_graph_memory():
    """Free the OWNERLESS memory behind captured launches on the current device: what launches captured with no graph
    arena bound were given (include/nddm.h: nddm_release_graph_memory).  Memory charged to a GraphArena is never touched."""
    _lib.check(_lib.lib().nddm_release_graph_memory())


class GraphArena:
    """Owner of the library memory behind captured launches (include/nddm.h: nddm_graph_arena_*).  Every launch captured
    into a hipGraph pins an allocation of its own (queue words + scratch); launches captured inside `with arena.bound():`
    are charged to this arena, and `release()` frees exactly those -- another owner's graphs keep replaying.  The holder
    destroys its graphs first, then releases."""

    def __init__(self):
        import ctypes
        h = ctypes.c_uint64(0)
        _lib.check(_lib.lib().nddm_graph_arena_create(ctypes.byref(h)))
        self.handle = int(h.value)

    def bound(self):
        """Context manager: captured launches of THIS thread are charged to the arena inside the block."""
        return _ArenaBinding(self)

    def info(self):
        import ctypes
        b, n = ctypes.c_uint64(0), ctypes.c_int32(0)
        _lib.check(_lib.lib().nddm_graph_arena_info(self.handle, ctypes.byref(b), ctypes.byref(n)))
        return {"bytes": int(b.value), "allocations": int(n.value)}

    @property
    def released(self):
        return self.handle == 0

    def release(self):
        """Free the arena's memory (idempotent).  Call after its graphs have been destroyed and the device is idle with
        respect to them."""
        if self.handle:
            h, self.handle = self.handle, 0
            _lib.check(_lib.lib().nddm_graph_arena_release(h))


class _ArenaBinding:
    def __init__(self, arena):
        self.arena, self.prev = arena, None

    def __enter__(self):
        import ctypes
        if self.arena.released:
            raise RuntimeError("this GraphArena has been released")
        prev = ctypes.c_uint64(0)
        _lib.check(_lib.lib().nddm_graph_arena_bind(self.arena.handle, ctypes.byref(prev)))
        self.prev = int(prev.value)
        return self.arena

    def __exit__(self, *exc):
        L = _lib.lib()
        if L.nddm_graph_arena_bind(self.prev, None) != 0:      # the outer owner was released meanwhile: no owner
            L.nddm_graph_arena_bind(0, None)
        return False


class graph_memory:
    """`with engine.graph_memory(): ...capture, replay, delete the graphs...`: an arena of its own is bound for the block
    and released on exit -- only what was captured INSIDE the block is freed (a GraphTrainer alive beside it, or an outer
    graph_memory block, keeps its memory).  A loop that re-captures -- one graph per n_trials bucket, say -- grows
    without an owner."""

    def __enter__(self):
        self.arena = GraphArena()
        self._binding = self.arena.bound()
        self._binding.__enter__()
        return self.arena

    def __exit__(self, *exc):
        self._binding.__exit__(*exc)
        require_device().cuda.synchronize()
        self.arena.release()
        return False


def last_launch():
    """Developer aid: geometry of this thread's last simulator launch (include/nddm.h: nddm_debug_last_launch)."""
    import ctypes
    out = (ctypes.c_int32 * 8)()
    _lib.check(_lib.lib().nddm_debug_last_launch(out))
    keys = ("grid_waves", "vgpr_keys", "ring", "tile_trials", "tiles_per_set", "sets_per_chunk", "refill_thresh", "lds_bytes")
    return dict(zip(keys, (int(v) for v in out)))
