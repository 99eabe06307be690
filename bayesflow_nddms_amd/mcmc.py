"""The reference's likelihood-based fit of basic_ddm_dc (basic_ddm_dc_pyjags.py: JAGS over dwiener, 6 chains per participant) as batched
Hamiltonian Monte Carlo on the device: engine.wiener_hmc runs every chain of every participant in one launch per block of iterations
(csrc/nddm_wiener_hmc.h); this module holds the host side -- the coordinates, the initial values, the warm-up schedule and the
reference's sample layout.  DESIGN.md section 17.

Columns (drift, boundary, beta, tau, dc); the posterior, its supports and its documented deviations from the JAGS model (the dc floor, tau
below the smallest response time) are the header's."""
import numpy as np

from . import engine

PARAM_NAMES = ("drift", "boundary", "beta", "tau", "dc")
JAGS_NAMES = {"drift": "delta", "boundary": "alpha", "beta": "beta", "tau": "ndt", "dc": "varsigma"}     # basic_ddm_dc_pyjags.py:170
DC_MIN = 0.05
ALL_FREE = 31


def free_mask(free=PARAM_NAMES):
    """Column names (or a mask) -> the five-bit mask of the sampled columns."""
    if isinstance(free, (int, np.integer)):
        if not 0 <= int(free) < 32:
            raise ValueError("free_mask has five bits")
        return int(free)
    unknown = [f for f in free if f not in PARAM_NAMES]
    if unknown:
        raise ValueError(f"unknown columns {unknown}: the columns are {PARAM_NAMES}")
    return sum(1 << PARAM_NAMES.index(f) for f in set(free))


def _tau_limit(d, censored=False):
    """d [C, N, 2] -> T [C] = min(1.5, the smallest rt of the data set); censored: of its RESPONSES (choice != 0), 1.5 where it has none --
    a timeout's rt bounds nothing (csrc/nddm_wiener_hmc.h: whmc_stage)."""
    rt = d[..., 0]
    if censored:
        rt = np.where(d[..., 1] == 0, np.asarray(np.inf, dtype=rt.dtype), rt)
    return np.minimum(1.5, rt.min(axis=1).astype(np.float64))


def _support(data, censored=False):
    """data [C, N, 2] (one data set per row of theta / q) -> (lo [C, 5], width [C, 5]) of the bounded columns (column 0 unused).
    censored: tau's upper limit comes from the responses only."""
    d = np.asarray(data, dtype=np.float32)
    if d.ndim == 2:
        d = d[None]
    if d.ndim != 3 or d.shape[-1] != 2 or d.shape[1] == 0:
        raise ValueError(f"data must have shape [C, n_trials, 2], got {d.shape}")
    T = _tau_limit(d, censored)
    if not (np.all(T > 0) and np.all(d[..., 0] > 0)):
        raise ValueError("response times must be > 0")
    C = d.shape[0]
    lo = np.zeros((C, 5))
    lo[:, 4] = DC_MIN
    wd = np.stack([np.ones(C), np.full(C, 10.0), np.ones(C), T, np.full(C, 10.0 - DC_MIN)], 1)
    return lo, wd


def theta_to_q(theta, data, free=ALL_FREE, censored=False):
    """theta [C, 5] (or [5]) in the model's columns -> the sampler's coordinates q, float64: drift unchanged, a bounded column
    logit((theta - lo) / (hi - lo)) with tau's upper limit T = min(1.5, the smallest rt of the row's data set) -- hence `data` [C, N, 2]
    (or [N, 2]).  A column that is not `free` keeps theta, as the sampler's state does.  censored (here and below): the data may hold
    timeouts (choice 0), and T is the smallest rt of the responses."""
    t = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    lo, wd = _support(data, censored)
    if t.shape != lo.shape:
        raise ValueError(f"theta must have shape [{lo.shape[0]}, 5] (one row per data set), got {t.shape}")
    mask = free_mask(free)
    x = (t - lo) / wd
    if any((mask >> j & 1) and np.any(~((x[:, j] > 0) & (x[:, j] < 1))) for j in range(1, 5)):
        raise ValueError("theta lies outside the sampler's support: boundary (0, 10), beta (0, 1), tau (0, min(1.5, min rt)), dc (0.05, 10)")
    q = t.copy()
    for j in range(1, 5):
        if mask >> j & 1:
            q[:, j] = np.log(x[:, j]) - np.log1p(-x[:, j])
    return q if np.ndim(theta) == 2 else q[0]


def q_to_theta(q, data, free=ALL_FREE, censored=False):
    """The inverse of theta_to_q."""
    x = np.atleast_2d(np.asarray(q, dtype=np.float64))
    lo, wd = _support(data, censored)
    if x.shape != lo.shape:
        raise ValueError(f"q must have shape [{lo.shape[0]}, 5] (one row per data set), got {x.shape}")
    mask = free_mask(free)
    t = x.copy()
    for j in range(1, 5):
        if mask >> j & 1:
            e = np.exp(-np.abs(x[:, j]))
            t[:, j] = lo[:, j] + wd[:, j] * np.where(x[:, j] >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    return t if np.ndim(q) == 2 else t[0]


def make_state(theta, data, eps0=0.05, free=ALL_FREE, censored=False):
    """The state [C, 12] a chain starts from at theta [C, 5] (data [C, N, 2]: each chain's data set): q, log eps = log eps0, log eps-bar =
    0, H-bar = 0, mu = log(10 eps0), no adapting iteration done (Hoffman & Gelman 2014, algorithm 5's initial values)."""
    q = np.atleast_2d(theta_to_q(theta, data, free, censored))
    st = np.zeros((q.shape[0], engine.WHMC_STATE))
    st[:, :5] = q
    st[:, 5] = np.log(eps0)
    st[:, 8] = np.log(10.0 * eps0)
    return st


def restart_adaptation(state, eps0=None):
    """A state whose step-size adaptation begins again: at the step size it has (or eps0), H-bar = 0, no adapting iteration done."""
    st = np.array(state, dtype=np.float64)
    if eps0 is not None:
        st[:, 5] = np.log(eps0)
    st[:, 6] = 0.0
    st[:, 7] = 0.0
    st[:, 8] = np.log(10.0) + st[:, 5]
    st[:, 9] = 0.0
    return st


def hmc_init(data, chains, seed, censored=False):
    """The reference's initial values (basic_ddm_dc_pyjags.py:188-196) for `chains` chains per data set: uniform on (.5, 2) for boundary and
    dc, (.2, .8) for beta, (-4, 4) for drift, (0, min rt / 2) for the non-decision time -> float64 [D, chains, 5] in this project's
    columns.  censored: min rt is the responses' (1.5 for a data set of timeouts alone)."""
    d = np.asarray(data, dtype=np.float64)
    if d.ndim == 2:
        d = d[None]
    rng = np.random.default_rng(seed)
    D = d.shape[0]
    th = np.empty((D, int(chains), 5))
    th[..., 0] = rng.uniform(-4.0, 4.0, (D, chains))
    th[..., 1] = rng.uniform(0.5, 2.0, (D, chains))
    th[..., 2] = rng.uniform(0.2, 0.8, (D, chains))
    th[..., 3] = rng.uniform(0.0, 1.0, (D, chains)) * (_tau_limit(d, censored)[:, None] / 2.0)
    th[..., 4] = rng.uniform(0.5, 2.0, (D, chains))
    return th


def _host(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def _trials(data, sets):
    """The data of a fit as float32 [sets, n_trials, 2] on the host (`sets`: the first axis' letter in the refusal)."""
    d = np.asarray(_host(data), dtype=np.float32)
    if d.ndim == 2:
        d = d[None]
    if d.ndim != 3 or d.shape[-1] != 2:
        raise ValueError(f"data must have shape [{sets}, n_trials, 2], got {d.shape}")
    return d


def _run(call, lead, carried, inv_mass, n_iter, n_adapt, iter_offset, max_iter, thin, **kw):
    """n_iter iterations from iter_offset as bounded launches -> (the launches' results, what the sampler carries from launch to launch).
    lead: the sampler's inputs before the carried ones; carried: {result key: value} in the call's order -- the state, and sigma when the
    sampler has one -- each taken from the launch's result for the next."""
    out, done = [], 0
    while done < n_iter:
        n = min(max_iter, n_iter - done)
        r = call(engine.BASIC_DDM_DC, *lead, *carried.values(), inv_mass=inv_mass, n_iter=n, n_adapt=n_adapt, thin=thin,
                 iter_offset=iter_offset + done, **kw)
        carried = {k: r[k] for k in carried}
        out.append(r)
        done += n
    return out, carried


def _fit(call, d, lead, own_fixed, init, max_iter_of, unit, chains, warmup, samples, thin, n_leapfrog, free, fixed, seed, eps0, censored=False,
         **kw):
    """What hmc_fit and hmc_fit_joint share: the checks, the mask and `fixed`, the initial state, the warm-up's two stages with the mass
    estimate between them, the sampling phase cut into bounded launches, and the JAGS layout.  d: _trials' data; lead: the sampler's inputs
    before the state; own_fixed(fixed) takes the sampler's own entries out of `fixed` -> (what else `fixed` may name, in the refusal's
    words, the sampler's own keywords); init(d, chains, seed) -> (theta [D, chains, 5], what the sampler carries besides the state);
    max_iter_of: the sampler's launch bound, `unit` its name for a launch; censored: every engine call gets censored=True (and none the
    keyword otherwise), and the support and the initial values come from the responses.
    -> (the layout, the sampling launches' results, mean(key): their n_iter-weighted mean of a per-launch output)."""
    chains, warmup, samples, thin = int(chains), int(warmup), int(samples), int(thin)
    if chains < 1 or warmup < 4 or samples < 1 or thin < 1 or samples % thin:
        raise ValueError("chains >= 1, warmup >= 4, samples >= 1 and thin dividing samples are required")
    mask = free_mask(free)
    fixed = {} if fixed is None else dict(fixed)
    also, own_kw = own_fixed(fixed)
    for k in fixed:
        if k not in PARAM_NAMES:
            raise ValueError(f"unknown fixed column {k!r}: the columns are {PARAM_NAMES}{also}")
        mask &= ~(1 << PARAM_NAMES.index(k))                             # (a fixed column is not sampled, whatever `free` says)
    D, N = d.shape[0], d.shape[1]
    theta, carried = init(d, chains, seed, censored) if censored else init(d, chains, seed)
    for k, v in fixed.items():
        theta[..., PARAM_NAMES.index(k)] = float(v)
    per_chain = np.repeat(d, chains, 0)
    carried = {"state": make_state(theta.reshape(-1, 5), per_chain, eps0=eps0, free=mask, censored=censored), **carried}
    max_iter = max_iter_of(N, n_leapfrog)
    if max_iter < 1:
        raise ValueError(f"n_leapfrog is too large for one bounded {unit}")
    kw = dict(kw, n_leapfrog=n_leapfrog, free_mask=mask, seed=seed, **own_kw, **({"censored": True} if censored else {}))
    quiet = dict(kw, want_draws=False, want_log_post=False)
    # stage 1: unit mass; its second half kept (every iteration) for the mass
    w1 = warmup // 2
    h1 = w1 // 2
    _, carried = _run(call, lead, carried, None, h1, w1, 0, max_iter, 1, **quiet)
    res, carried = _run(call, lead, carried, None, w1 - h1, w1, h1, max_iter, 1, want_log_post=False, **kw)
    th = np.concatenate([_host(r["draws"]) for r in res], 1).astype(np.float64)                   # [C, w1 - h1, 5], float32 theta
    lo, wd = _support(per_chain, censored)
    x = np.clip((th - lo[:, None, :]) / wd[:, None, :], 1e-7, 1.0 - 1e-7)
    qs = np.where(np.array([False] + [bool(mask >> j & 1) for j in range(1, 5)]), np.log(x) - np.log1p(-x), th)
    var = np.var(qs, axis=1) if qs.shape[1] > 1 else np.ones((D * chains, 5))
    inv_mass = np.where(np.isfinite(var), np.maximum(var, 1e-3), 1.0)
    # stage 2: that mass, the step size adapted again
    carried["state"] = restart_adaptation(_host(carried["state"]))
    w2 = warmup - w1
    _, carried = _run(call, lead, carried, inv_mass, w2, w2, w1, max_iter, 1, **quiet)
    res, carried = _run(call, lead, carried, inv_mass, samples, w2, warmup, max_iter, thin, **kw)
    # (iteration g is kept when (g + 1) % thin == 0: with warmup a multiple of thin every launch's draws line up)
    draws = np.concatenate([_host(r["draws"]) for r in res], 1).astype(np.float64)
    lp = np.concatenate([_host(r["log_post"]) for r in res], 1).astype(np.float64)
    K = draws.shape[1]
    n_samp = np.array([min(max_iter, samples - i * max_iter) for i in range(len(res))], dtype=np.float64)

    def mean(key):
        return sum(_host(r[key]).astype(np.float64) * n for r, n in zip(res, n_samp)) / n_samp.sum()
    out = {JAGS_NAMES[name]: draws[:, :, j].reshape(D, chains, K).transpose(0, 2, 1) for j, name in enumerate(PARAM_NAMES)}
    out["log_post"] = lp.reshape(D, chains, K).transpose(0, 2, 1)
    out["accept_rate"] = mean("accept").reshape(D, chains)
    out["n_divergent"] = sum(_host(r["divergent"]).astype(np.int64) for r in res).reshape(D, chains)
    out["flagged"] = _host(res[0]["flagged"]).astype(np.int64).reshape(D, chains)
    return out, res, mean


def hmc_fit(data, chains=6, warmup=2000, samples=10000, thin=10, n_leapfrog=16, free=PARAM_NAMES, fixed=None, seed=0, eps0=0.05,
            device=None, _call=None, censored=False):
    """Fit basic_ddm_dc to every data set of data [D, n_trials, 2] = (rt, choice in {1, -1}) by `chains` HMC chains each, all D * chains
    chains side by side on the device (engine.wiener_hmc), the defaults the reference's: 6 chains, 2000 + 10 000 iterations, thin 10.

    free: the sampled columns; fixed: {column: value}, columns held at a value and taken out of `free` (fixed={"dc": 1.0} is the standard DDM
    fit: the likelihood identifies only boundary / dc and drift / dc, so with dc free the priors alone hold that direction); a column
    neither free nor fixed keeps its initial value.  Warm-up has two stages: the first half adapts
    the step size under unit mass, and its second half's q give inv_mass, their per-chain variance floored at 1e-3; the second half adapts
    the step size again under that mass.  Sampling follows, cut into the bounded launches the entry point accepts.
    censored=True: the data may hold the simulator's timeouts (choice 0), scored right-censored (engine.wiener_hmc's censored); tau's upper
    limit and the initial values come from the responses.  Without it a data set with a timeout is refused (a host array) or flagged.

    Returns the reference's JAGS-sample layout: 'alpha', 'ndt', 'beta', 'delta', 'varsigma', each float64 [D, samples // thin, chains], plus
    'log_post' of the same shape, 'accept_rate' [D, chains] (the sampling iterations' mean acceptance probability), 'n_divergent'
    [D, chains] and 'flagged' [D, chains]."""
    call = _call or (lambda *a, **k: engine.wiener_hmc(*a, device=device, **k))
    d = _trials(data, "D")
    return _fit(call, d, (d,), lambda fixed: ("", {}), lambda *a: (hmc_init(*a), {}), engine.wiener_hmc_max_iter, "launch", chains, warmup,
                samples, thin, n_leapfrog, free, fixed, seed, eps0, censored=bool(censored), chains_per_dataset=int(chains))[0]


def hmc_init_joint(data, chains, seed, censored=False):
    """The reference's initial values of the alpha_not_scaled fit (alpha_not_scaled.py:233-244): hmc_init's for the participants (alpha and
    varsigma U(.5, 2), beta U(.2, .8), delta U(-4, 4), ndt U(0, min rt / 2)) and sigma U(.01, 5) per joint chain -> (theta float64 [P, chains,
    5], sigma float64 [chains])."""
    theta = hmc_init(data, chains, seed, censored)
    sigma = np.random.default_rng([int(seed), 0x516]).uniform(0.01, 5.0, int(chains))
    return theta, sigma


def hmc_fit_joint(data, extdata, chains=6, warmup=2000, samples=10000, thin=10, n_leapfrog=16, free=PARAM_NAMES, fixed=None, seed=0,
                  eps0=0.05, device=None, _call=None, censored=False):
    """Fit the alpha_not_scaled JAGS model (alpha_not_scaled.py:138-259): every participant of data [P, n_trials, 2] = (rt, choice in {1,
    -1}) has basic_ddm_dc's five parameters, extdata [P] ~ N(alpha_p, sigma) measures the boundary, and one sigma ~ N(3, 1) T(0, 10) is
    shared -- `chains` JOINT chains of P participant chains and a sigma each, side by side on the device (engine.wiener_hmc_joint), the
    defaults the reference's: 6 chains, 2000 + 10 000 iterations, thin 10.

    free / fixed / censored: hmc_fit's; `fixed` may also name "sigma" (held at that value, never sampled).  The warm-up is hmc_fit's two stages.
    Returns hmc_fit's dictionary (each variable float64 [P, samples // thin, chains]; 'log_post' is the participant's conditional log
    posterior given sigma) plus 'sigma' float64 [1, samples // thin, chains] -- the shape pyjags gives a scalar node, so
    diagnostics.rhat_neff(fit) takes it as it stands -- and 'sigma_accept' [chains], the share of the sampling iterations' sigma proposals
    accepted (NaN when sigma is fixed)."""
    call = _call or (lambda *a, **k: engine.wiener_hmc_joint(*a, device=device, **k))
    d = _trials(data, "P")
    P = d.shape[0]
    ext = np.asarray(_host(extdata), dtype=np.float64).reshape(-1)
    if ext.shape != (P,) or not np.all(np.isfinite(ext)):
        raise ValueError(f"extdata must hold one finite value per participant ({P}), got shape {ext.shape}")
    held = []                                                            # the fixed sigma, if there is one

    def own_fixed(fixed):
        if "sigma" in fixed:
            held.append(float(fixed.pop("sigma")))
            if not (np.isfinite(held[0]) and held[0] > 0):
                raise ValueError("a fixed sigma must be finite and > 0")
        elif P < 2:
            raise ValueError("sampling sigma needs at least 2 participants: fix it (fixed={'sigma': value}) or bring more")
        return " and 'sigma'", dict(sigma_fixed=bool(held))

    def init(d, chains, seed, censored=False):
        theta, sigma = hmc_init_joint(d, chains, seed, censored)
        return theta, {"sigma": np.full(chains, held[0]) if held else sigma}
    out, res, mean = _fit(call, d, (d, ext), own_fixed, init, engine.wiener_hmc_joint_max_iter, "call", chains, warmup, samples, thin, n_leapfrog,
                          free, fixed, seed, eps0, censored=bool(censored))
    out["sigma"] = np.concatenate([_host(r["sigma_draws"]) for r in res], 1).astype(np.float64).T[None]      # [chains, K] -> [1, K, chains]
    out["sigma_accept"] = mean("sigma_accept")
    return out
