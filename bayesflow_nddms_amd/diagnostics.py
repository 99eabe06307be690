"""Host-side distribution diagnostics: histograms on the integer Euler-Maruyama step grid and the
Kolmogorov-Smirnov distance of signed response times (sign = choice, 0 = missing response).

Comparing on the integer step index avoids float32-vs-float64 tie artefacts: rt = k*dt + tau, so the
signed RT is a monotone function of choice*k and the KS distance of signed RTs is the KS distance of choice*k.
"""
import numpy as np


def step_hist_from_trials(trials, tau, dt, max_k, signed=False):
    """trials [..., 2] -> int64 hist [3, max_k+1] (rows: upper, lower, timeout) over the step index k.

    signed=False: columns (rt, choice) as basic_ddm_dc.py:124; signed=True: column 0 is choicert = +-(ter + rt) or 0
    (single_trial_alpha_not_scaled.py:136-141)."""
    t = np.asarray(trials, dtype=np.float64)
    if np.ndim(tau) > 0:                      # one non-decision time per set: trials is [B, N, 2]
        tau = np.broadcast_to(np.asarray(tau, dtype=np.float64).reshape(-1, 1), t.shape[:2]).reshape(-1)
    else:
        tau = float(tau)
    t = t.reshape(-1, 2)
    if signed:
        choice = np.sign(t[:, 0])
        k = np.where(choice == 0, max_k, np.rint((np.abs(t[:, 0]) - tau) / dt)).astype(np.int64)
    else:
        choice = t[:, 1]
        k = np.rint((t[:, 0] - tau) / dt).astype(np.int64)
    k = np.clip(k, 0, max_k)
    hist = np.zeros((3, max_k + 1), dtype=np.int64)
    for row, c in ((0, 1), (1, -1), (2, 0)):
        hist[row] = np.bincount(k[choice == c], minlength=max_k + 1)
    return hist


def signed_cdf(hist):
    """CDF over positions -K..K of choice*k (timeouts at 0)."""
    h = np.asarray(hist, dtype=np.float64)
    K = h.shape[1] - 1
    pmf = np.zeros(2 * K + 1)
    pmf[:K + 1] += h[1][::-1]          # lower boundary: position -k
    pmf[K] += h[2].sum()               # missing responses: position 0
    pmf[K:] += h[0]                    # upper boundary: position +k
    return np.cumsum(pmf) / pmf.sum()


def ks_signed(hist_a, hist_b):
    """Two-sample KS distance of the signed step index (== of the signed RT)."""
    return float(np.max(np.abs(signed_cdf(hist_a) - signed_cdf(hist_b))))


def ks_conditional(hist_a, hist_b, row):
    """KS of the step index given the choice (row 0 upper, 1 lower)."""
    a, b = np.asarray(hist_a[row], float), np.asarray(hist_b[row], float)
    if a.sum() == 0 or b.sum() == 0:
        return 0.0
    return float(np.max(np.abs(np.cumsum(a) / a.sum() - np.cumsum(b) / b.sum())))


def choice_probs(hist):
    h = np.asarray(hist, dtype=np.float64)
    return h.sum(axis=1) / h.sum()


def ks_quantile_table(sample, q_table):
    """KS distance between an empirical sample and a reference given as a dense quantile table
    (q_table[i] = quantile i/(len-1)).  Used for continuous outputs (z1, simulratcliff RTs)."""
    s = np.sort(np.asarray(sample, dtype=np.float64))
    q = np.asarray(q_table, dtype=np.float64)
    n, m = len(s), len(q) - 1
    # reference CDF evaluated at the sample points by inverting the quantile table
    f_ref = np.interp(s, q, np.linspace(0.0, 1.0, m + 1), left=0.0, right=1.0)
    f_emp_hi = np.arange(1, n + 1) / n
    f_emp_lo = np.arange(0, n) / n
    return float(max(np.max(np.abs(f_emp_hi - f_ref)), np.max(np.abs(f_emp_lo - f_ref))))


# ------------------------------------------------------------------------------------------------------------------
# The numbers the reference's recovery plots print (the consumer of amortizer.sample on the other side of the path)
def recovery_statistics(theta_true, theta_est):
    """Per parameter, what `recovery_scatter` writes into its panels (pyhddmjagsutils.py:609-623): R^2 = sklearn's r2_score(true,
    estimate) -- 1 - SS_res / SS_tot about the mean of the TRUE values, negative when the estimates are worse than that mean -- and
    Pearson's rho.  theta_true, theta_est: [n_datasets, P] (the reference passes posterior MEANS: basic_ddm_dc.py:236-250).
    -> {'r2': [P], 'rho': [P]}."""
    t, e = np.asarray(theta_true, dtype=np.float64), np.asarray(theta_est, dtype=np.float64)
    if t.shape != e.shape or t.ndim != 2:
        raise ValueError(f"theta_true and theta_est must both be [n_datasets, P]; got {t.shape} and {e.shape}")
    ss_res = ((t - e) ** 2).sum(axis=0)
    ss_tot = ((t - t.mean(axis=0)) ** 2).sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r2 = np.where(ss_tot > 0, 1.0 - ss_res / ss_tot, np.where(ss_res == 0, 1.0, 0.0))      # (r2_score's convention for a constant target)
        tc, ec = t - t.mean(axis=0), e - e.mean(axis=0)
        rho = (tc * ec).sum(axis=0) / np.sqrt((tc ** 2).sum(axis=0) * (ec ** 2).sum(axis=0))
    return {"r2": r2, "rho": rho}


def converged_fits(param_means, index=3, low=0.0, high=1.0):
    """The reference's "clearly good" filter (basic_ddm_dc.py:239-241, single_trial_alpha_not_scaled.py:326-328): model fits whose
    posterior MEAN of the non-decision time (parameter 3 in both models) lies inside (0, 1) -> boolean [n_datasets]."""
    m = np.asarray(param_means, dtype=np.float64)
    return (m[:, index] > low) & (m[:, index] < high)


def rhat_neff(samples):
    """Convergence diagnostics of MCMC output in the reference's JAGS-sample layout: a dict of arrays [..., iterations, chains] (keys that
    begin with '_' are skipped), or one such array -> per key (or for the array) {'rhat', 'neff', 'mean', 'std'}, each of the leading
    shape.  What the reference's `diagnostic` reports (pyhddmjagsutils.py:180-331), from the formulas of Gelman et al., Bayesian Data
    Analysis, 3rd ed., section 11.4-11.5, with that function's conventions: population variances (divisor n) within a chain;
        rhat   split chains: each chain's halves as 2m chains of n/2, sqrt(((1 - 2/n) W + (2/n) B) / W)
        neff   m n / (1 + 2 sum rho_t) with rho_t = 1 - V_t / (2 var+), var+ of the UNSPLIT chains, V_t the variogram at lag t averaged over
               the chains; lags 1, 2, ... are added in pairs (t, t + 1), t odd, while the last pair's sum is not negative (that pair is
               still counted) and the pair's even lag stays below n - 2; rounded to an integer."""
    if isinstance(samples, dict):
        return {k: rhat_neff(v) for k, v in samples.items() if not k.startswith("_")}
    x = np.asarray(samples, dtype=np.float64)
    if x.ndim < 2 or x.shape[-2] < 4 or x.shape[-1] < 2:
        raise ValueError(f"samples must be [..., iterations >= 4, chains >= 2], got {x.shape}")
    lead, n, m = x.shape[:-2], x.shape[-2], x.shape[-1]
    x = x.reshape((-1, n, m))

    def var_plus(y):                                                    # y [V, n, m] -> (var+, W)
        k = y.shape[1]
        cm = y.mean(axis=1)
        B = k * ((cm - cm.mean(axis=1, keepdims=True)) ** 2).sum(axis=1) / (y.shape[2] - 1.0)
        W = y.var(axis=1).mean(axis=1)
        return (1.0 - 1.0 / k) * W + B / k, W
    h = n // 2
    split = np.concatenate([x[:, :h, :], x[:, h:2 * h, :]] if n % 2 == 0 else [x[:, :h, :], x[:, n - h:, :]], axis=2)
    with np.errstate(divide="ignore", invalid="ignore"):
        vs, Ws = var_plus(split)
        rhat = np.sqrt(vs / Ws)
        vp, _ = var_plus(x)
        neff = np.empty(x.shape[0])
        for v in range(x.shape[0]):
            tot, pair, t = 0.0, 0.0, 2
            while t < n - 2 and pair >= 0.0:
                odd = 1.0 - np.mean((x[v, t - 1:] - x[v, :n - t + 1]) ** 2) / (2.0 * vp[v])
                even = 1.0 - np.mean((x[v, t:] - x[v, :n - t]) ** 2) / (2.0 * vp[v])
                pair = odd + even
                tot += pair
                t += 2
            neff[v] = np.round(m * n / (1.0 + 2.0 * tot))
    return {"rhat": rhat.reshape(lead), "neff": neff.reshape(lead), "mean": x.mean(axis=(1, 2)).reshape(lead),
            "std": x.reshape(x.shape[0], -1).std(axis=1).reshape(lead)}


def summary(insamples):
    """The reference's `summary` (pyhddmjagsutils.py:334-388) for MCMC output in its JAGS-sample layout -- what mcmc.hmc_fit /
    hmc_fit_joint return and rhat_neff accepts: a dict of arrays [..., iterations, chains] (keys that begin with '_' are skipped) -> per
    key {'mean', 'std', 'median', '95lower', '95upper', '99lower', '99upper'}, each float64 of the leading shape, over the key's
    iterations x chains samples.  mean and std (ddof 0) are NumPy's in float64.  The quantiles are exact order statistics,
    interpolated as np.quantile's default does, of the samples as float32 (the fits' samples are float32 values) through
    amortizer.draw_quantiles as [variables, iterations x chains, 1]: one kernel launch per key on the device when there is one,
    the PyTorch evaluation of the same definition otherwise.  A non-finite sample is left out of its variable's quantiles."""
    import torch
    from .amortizer import draw_quantiles
    dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    names = (("median", .5), ("95lower", .025), ("95upper", .975), ("99lower", .005), ("99upper", .995))
    result = {}
    for key, v in insamples.items():
        if key.startswith("_"):
            continue
        x = np.asarray(v.cpu() if hasattr(v, "is_cuda") else v, dtype=np.float64)
        if x.ndim < 2 or x.shape[-1] * x.shape[-2] == 0:
            raise ValueError(f"samples of '{key}' must be [..., iterations >= 1, chains >= 1], got {x.shape}")
        lead = x.shape[:-2]
        allsamps = x.reshape(lead + (x.shape[-2] * x.shape[-1],))
        res = {"mean": np.mean(allsamps, axis=-1), "std": np.std(allsamps, axis=-1)}
        if allsamps.size:
            th = torch.as_tensor(allsamps.reshape(-1, allsamps.shape[-1]).astype(np.float32), device=dev)[:, :, None]
            q = draw_quantiles(th, [p for _, p in names])["quantiles"][:, :, 0].cpu().numpy()
        else:
            q = np.empty((0, len(names)))
        for k, (name, _) in enumerate(names):
            res[name] = q[:, k].reshape(lead)
        result[key] = res
    return result


def posterior_log_likelihood(samples, data, model):
    """Score posterior draws by the exact likelihood: samples [D, S, P] (what amortizer.sample returns for a batch of D data sets;
    [S, P] for one), data [D, n_trials, 2] in the simulator's format (model = engine.BASIC_DDM_DC or engine.ALPHA_NOT_SCALED) ->
    float64 [D, S] = log p(data[d] | samples[d, s]), in one launch of the broadcast layout (each data set staged once per 16 draws).
    The numbers importance weights (amortizer.importance_weights, AmortizedPosterior.posterior_importance), posterior predictive log
    scores and LOO / WAIC start from."""
    from . import engine
    single = samples.ndim == 2
    s = samples[None] if single else samples
    d = data[None] if data.ndim == 2 else data
    D, S, P = (int(x) for x in s.shape)
    if int(d.shape[0]) != D:
        raise ValueError(f"samples hold {D} data sets but data holds {int(d.shape[0])}")
    flat = s.reshape(D * S, P) if hasattr(s, "is_cuda") else np.asarray(s, dtype=np.float64).reshape(D * S, P)
    ll = engine.wiener_log_likelihood(model, flat, d, draws_per_dataset=S)["loglik"].reshape(D, S)
    return ll[0] if single else ll


def signed_cdf_analytic(trials, params, model):
    """The exact law's distribution function of the SIGNED response time, G(y) = P(signed RT <= y), at every trial of every set:
    trials [B, N, 2] in the simulator's format (model = engine.BASIC_DDM_DC: (rt, choice); engine.ALPHA_NOT_SCALED: (y, acc)), params
    [B, P] -> float32 [B, N] on the device, one launch (engine.wiener_cdf):
        G = P_lo - F_lo(rt - tau) on the lower boundary,   G = P_lo + F_up(rt - tau) on the upper one.
    A timeout (choice 0 / y == 0) has no signed time: NaN."""
    from . import engine
    torch = engine.require_device()
    r = engine.wiener_cdf(model, params, trials, draws_per_dataset=1)
    t = trials if hasattr(trials, "is_cuda") else torch.as_tensor(np.asarray(trials, dtype=np.float32), device=r["cdf"].device)
    t = t[None] if t.ndim == 2 else t
    side = t[..., 1] if model == engine.BASIC_DDM_DC else t[..., 0]
    p_lo = (1.0 - r["p_upper"])[:, None]
    g = torch.where(side > 0, p_lo + r["cdf"], p_lo - r["cdf"])
    return torch.where(side == 0, torch.full_like(g, float("nan")), g)


def ks_analytic(trials, params, model):
    """One-sample Kolmogorov-Smirnov distance of each set's signed response times from the exact law's G (signed_cdf_analytic):
    sup_y |ECDF(y) - G(y)| = max_i max(|i/n - G(y_(i))|, |(i-1)/n - G(y_(i))|) over the sorted sample -> float64 [B] on the device,
    no host synchronisation (a sort along the trial axis, one kernel launch, a max).  A set that holds a timeout (choice 0 / y == 0)
    gives NaN for that set: a timeout has no place on the signed axis."""
    from . import engine
    torch = engine.require_device()
    g = signed_cdf_analytic(trials, params, model).double()
    n = g.shape[1]
    t = trials if hasattr(trials, "is_cuda") else torch.as_tensor(np.asarray(trials, dtype=np.float32), device=g.device)
    t = t[None] if t.ndim == 2 else t
    y = t[..., 0] * t[..., 1] if model == engine.BASIC_DDM_DC else t[..., 0]
    gs = torch.gather(g, 1, torch.sort(y, dim=1).indices)
    i = torch.arange(1, n + 1, dtype=torch.float64, device=g.device)[None, :]
    dist = torch.maximum((i / n - gs).abs(), ((i - 1.0) / n - gs).abs())
    ks = dist.max(dim=1).values
    return torch.where(torch.isnan(g).any(dim=1), torch.full_like(ks, float("nan")), ks)


def quantile_probability(sim_data, params, model, probs=(.1, .3, .5, .7, .9)):
    """The numbers of a quantile-probability plot, on the device: sim_data [D, N, 2] in the simulator's format (model =
    engine.BASIC_DDM_DC: (rt, choice); engine.ALPHA_NOT_SCALED: (y, acc)), params [D, S, P] (S parameter rows per data set, posterior draws
    for instance) -> a dict of device tensors
        'observed'          float32 [D, 2, Q]     empirical response-time quantiles (linear interpolation of the order statistics) of the
                                                  lower ([:, 0]) and upper ([:, 1]) boundary's responses; NaN for a boundary with fewer than Q
        'predicted'         float32 [D, S, 2, Q]  the exact law's quantiles of each boundary's own responses (engine.wiener_quantile, one launch)
        'p_upper_observed'  float32 [D]           the share of upper-boundary responses among the responses (timeouts left out)
        'p_upper_predicted' float32 [D, S]        P(upper boundary) (engine.wiener_cdf)
    No host synchronisation: a sort along the trial axis and two kernel launches."""
    from . import engine
    torch = engine.require_device()
    D, S, P = (int(x) for x in params.shape)
    flat = params.reshape(D * S, P) if hasattr(params, "is_cuda") else np.asarray(params, dtype=np.float64).reshape(D * S, P)
    pr = np.asarray(probs, dtype=np.float64).reshape(-1)
    Q = pr.shape[0]
    req = np.stack([np.concatenate([pr, pr]), np.concatenate([-np.ones(Q), np.ones(Q)])], -1)[None]
    pred = engine.wiener_quantile(model, flat, req, draws_per_dataset=D * S, conditional=True)["quantile"].reshape(D, S, 2, Q)
    dev = pred.device
    t = sim_data if hasattr(sim_data, "is_cuda") else torch.as_tensor(np.asarray(sim_data, dtype=np.float32), device=dev)
    if int(t.shape[0]) != D:
        raise ValueError(f"params hold {D} data sets but sim_data holds {int(t.shape[0])}")
    p_up = engine.wiener_cdf(model, flat, t, draws_per_dataset=S, want_cdf=False)["p_upper"].reshape(D, S)
    rt = t[..., 0] if model == engine.BASIC_DDM_DC else t[..., 0].abs()
    side = t[..., 1] if model == engine.BASIC_DDM_DC else t[..., 0]
    pq = torch.as_tensor(pr, dtype=torch.float64, device=dev)[None, :]
    obs, counts = [], []
    for mask in (side < 0, side > 0):
        n = mask.sum(dim=1)
        srt = torch.sort(torch.where(mask, rt, torch.full_like(rt, float("inf"))), dim=1).values.double()
        pos = pq * (n.clamp(min=1) - 1)[:, None].double()
        lo = pos.floor().long()
        hi = torch.minimum(lo + 1, (n.clamp(min=1) - 1)[:, None])
        a, b = torch.gather(srt, 1, lo), torch.gather(srt, 1, hi)
        val = a + (b - a) * (pos - lo.double())
        obs.append(torch.where((n >= Q)[:, None], val, torch.full_like(val, float("nan"))).float())
        counts.append(n)
    n_lo, n_up = counts
    return {"observed": torch.stack(obs, 1), "predicted": pred, "p_upper_observed": (n_up.double() / (n_lo + n_up).double()).float(),
            "p_upper_predicted": p_up}
