"""Prior and context samplers.

Host versions restate the reference's draw order call for call (basic_ddm_dc.py:50-80,
single_trial_alpha_not_scaled.py:66-102, :889-913, :1205-1232): `RNG` is a module-level default_rng(2023) (PCG64)
used for drift / beta / sigma1 / gamma, the truncated normals go through scipy.stats.truncnorm.rvs on NumPy's
GLOBAL legacy stream, and prior_N uses np.random.randint -- so with the same seeds they return the reference's
numbers bit for bit (tests/golden/priors.npz).

DevicePrior is the batched on-device sampler (SURVEY f-1): the per-set SciPy calls cost ~0.5 ms per draw, i.e.
minutes per million sets, which would dwarf the simulate time; the device version fills [B, P] in one launch and is
checked per marginal by KS against the reference draws.
"""
import numpy as np
from scipy.stats import truncnorm

from . import engine


def prior_N(n_min=60, n_max=300):
    """A prior for the random number of observations (basic_ddm_dc.py:50-52); global NumPy stream."""
    return np.random.randint(n_min, n_max + 1)


def truncnorm_better(mean=0, sd=1, low=-10, upp=10, size=1):
    """basic_ddm_dc.py:55-57."""
    return truncnorm.rvs((low - mean) / sd, (upp - mean) / sd, loc=mean, scale=sd, size=size)


RNG = np.random.default_rng(2023)   # basic_ddm_dc.py:60 / single_trial_alpha_not_scaled.py:76


def reset_host_rng(seed=2023):
    """Re-create the module-level generator (what re-importing the reference script does)."""
    global RNG
    RNG = np.random.default_rng(seed)


def draw_prior_basic():
    """basic_ddm_dc.py:62-80 -> [drift, alpha, beta, ter, dc]."""
    drift = RNG.normal(0.0, 2.0)
    alpha = truncnorm_better(mean=1.0, sd=0.5, low=0.0, upp=10)[0]
    beta = RNG.beta(2.0, 2.0)
    ter = truncnorm_better(mean=0.5, sd=0.25, low=0.0, upp=1.5)[0]
    dc = truncnorm_better(mean=1.0, sd=0.5, low=0.0, upp=10)[0]
    return np.hstack((drift, alpha, beta, ter, dc))


def draw_prior_single():
    """single_trial_alpha_not_scaled.py:78-102 -> [drift, mu_alpha, beta, ter, std_alpha, dc, sigma1]
    (draw_prior_alt :889-913 has the same marginals with std_dc / mu_dc at indices 4 / 5)."""
    drift = RNG.normal(0.0, 2.0)
    mu_alpha = truncnorm_better(mean=1.0, sd=0.5, low=0.0, upp=10)[0]
    beta = RNG.beta(2.0, 2.0)
    ter = truncnorm_better(mean=0.5, sd=0.25, low=0.0, upp=1.5)[0]
    std_alpha = truncnorm_better(mean=1.0, sd=0.5, low=0.0, upp=3)[0]
    dc = truncnorm_better(mean=1.0, sd=0.5, low=0.0, upp=10)[0]
    sigma1 = RNG.uniform(0.0, 5.0)
    return np.hstack((drift, mu_alpha, beta, ter, std_alpha, dc, sigma1))


def draw_prior_scale():
    """single_trial_alpha_not_scaled.py:1205-1232: the 7 parameters above + gamma ~ U(0, 2)."""
    p = draw_prior_single()
    gamma = RNG.uniform(0.0, 2.0)
    return np.hstack((p, gamma))


# the supports of the priors above (drift ~ N(0, 2): +- 5 sd), per parameter in the reference's order
PRIOR_SUPPORT = {"basic": ([-10.0, 0.0, 0.0, 0.0, 0.0], [10.0, 10.0, 1.0, 1.5, 10.0]),
                 "single": ([-10.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [10.0, 10.0, 1.0, 1.5, 3.0, 10.0, 5.0])}


def prior_box(model="basic", widen=1.0):
    """(low, high): the prior's support widened by `widen` times its own width on each side -- the generous box
    `AmortizedPosterior.sample(..., reject_outside=prior_box(model))` redraws outside of.  A posterior draw beyond it is not a
    parameter value the model could have produced the data with; the reference itself counts "model fits in the prior range"
    before plotting (basic_ddm_dc.py:239-241)."""
    lo, hi = (np.asarray(v, dtype=np.float64) for v in PRIOR_SUPPORT[model])
    return lo - widen * (hi - lo), hi + widen * (hi - lo)


# The priors above as densities, ONE description per column from which both the host's log density (log_prior_density) and the
# table the importance kernel reads (prior_table, csrc/train_importance.hip) are built:
#   ("normal", mean, sd) | ("truncnormal", mean, sd, low, high) | ("beta", a, b) on [0, 1] | ("uniform", low, high) | ("fixed", value)
_BASIC_DENSITY = (("normal", 0.0, 2.0), ("truncnormal", 1.0, 0.5, 0.0, 10.0), ("beta", 2.0, 2.0), ("truncnormal", 0.5, 0.25, 0.0, 1.5),
                  ("truncnormal", 1.0, 0.5, 0.0, 10.0))
_SINGLE_DENSITY = _BASIC_DENSITY[:4] + (("truncnormal", 1.0, 0.5, 0.0, 3.0), ("truncnormal", 1.0, 0.5, 0.0, 10.0), ("uniform", 0.0, 5.0))
PRIOR_DENSITY = {"basic": _BASIC_DENSITY, "single": _SINGLE_DENSITY, "scale": _SINGLE_DENSITY + (("uniform", 0.0, 2.0),)}
PRIOR_KINDS = {"normal": 0, "truncnormal": 1, "beta": 2, "uniform": 3, "fixed": 4}


def prior_table(model="basic"):
    """float64 [P, 6], one row per column: kind (PRIOR_KINDS), two shape parameters, low, high, and the log normaliser -- what is
    subtracted from the kernel of the log density inside [low, high]; outside (or at a non-finite value) the log density is -inf.
        normal       mean, sd;  -inf, inf;  log(sd) + log(2 pi) / 2
        truncnormal  mean, sd;  low, high;  the same + log(Phi((high - mean) / sd) - Phi((low - mean) / sd))
        beta         a, b;      0, 1;       log B(a, b)      (a term whose exponent is 0 is 0, also at the edge: scipy's xlogy)
        uniform      0, 0;      low, high;  log(high - low)
        fixed        value, 0;  value, value;  0             (a column that is no random variable: 0 at its value, -inf elsewhere)
    model: a name of PRIOR_DENSITY or such a description itself (a sequence of tuples)."""
    from scipy.special import betaln, ndtr
    rows = []
    for col in (PRIOR_DENSITY[model] if isinstance(model, str) else model):
        kind, a = col[0], [float(v) for v in col[1:]]
        if kind == "normal":
            row = [a[0], a[1], -np.inf, np.inf, np.log(a[1]) + 0.5 * np.log(2.0 * np.pi)]
        elif kind == "truncnormal":
            mass = ndtr((a[3] - a[0]) / a[1]) - ndtr((a[2] - a[0]) / a[1])
            row = [a[0], a[1], a[2], a[3], np.log(a[1]) + 0.5 * np.log(2.0 * np.pi) + np.log(mass)]
        elif kind == "beta":
            row = [a[0], a[1], 0.0, 1.0, float(betaln(a[0], a[1]))]
        elif kind == "uniform":
            row = [0.0, 0.0, a[0], a[1], np.log(a[1] - a[0])]
        elif kind == "fixed":
            row = [a[0], 0.0, a[0], a[0], 0.0]
        else:
            raise ValueError(f"unknown prior kind {kind!r}")
        rows.append([float(PRIOR_KINDS[kind])] + row)
    return np.asarray(rows, dtype=np.float64)


# The rows the marginal likelihood's accuracy is stated on (tests/wiener_marginal_ref.py: _prior_pool, DEVICE_BAR): lower bounds by column
# name.  An importance sampler sends the likelihood its proposal's tail draws, so its target is the posterior under the prior restricted
# to these rows (restricted_density), and says so.
MARGINAL_DOMAIN = {"std_alpha": 0.02, "dc": 0.05, "sigma1": 0.02}
_SINGLE_COLUMNS = ("drift", "mu_alpha", "beta", "ter", "std_alpha", "dc", "sigma1", "gamma")


def restricted_density(model, lows=MARGINAL_DOMAIN):
    """PRIOR_DENSITY[model] ("single": 7 columns; "scale": 8, gamma ~ U(0, 2)) with the lower end of the named columns RAISED to lows[name]
    (never lowered): a description prior_table and log_prior_density accept, which renormalise the truncated normals and the uniform
    themselves -- the prior conditioned on the rows inside, a proper density.  lows: {column name: lower bound} over std_alpha, dc, sigma1."""
    if model not in ("single", "scale"):
        raise ValueError(f"restricted_density covers the single-trial models 'single' and 'scale', not {model!r}")
    unknown = set(lows) - set(_SINGLE_COLUMNS[4:7])
    if unknown:
        raise ValueError(f"lower bounds may be given for std_alpha, dc and sigma1, not {sorted(unknown)}")
    out = []
    for name, col in zip(_SINGLE_COLUMNS, PRIOR_DENSITY[model]):
        if name in lows:
            low = max(float(lows[name]), float(col[-2]))
            if not low < float(col[-1]):
                raise ValueError(f"the lower bound of {name} must lie below its upper end {col[-1]}")
            col = col[:-2] + (low, col[-1])
        out.append(col)
    return tuple(out)


def log_prior_density(model, theta):
    """log p(theta) under the model's prior, float64: theta [..., P] -> [...], the sum over the columns of prior_table(model)'s
    densities; -inf where a component is outside its support or not finite.  The host definition of what the importance kernel
    evaluates (amortizer.importance_weights)."""
    table = prior_table(model)
    th = np.asarray(theta, dtype=np.float64)
    if th.shape[-1] != table.shape[0]:
        raise ValueError(f"theta must have {table.shape[0]} columns, got {th.shape}")
    out = np.zeros(th.shape[:-1])
    with np.errstate(all="ignore"):
        for d, (kind, p1, p2, lo, hi, ln) in enumerate(table):
            x = th[..., d]
            if kind in (0.0, 1.0):
                u = (x - p1) / p2
                lp = -0.5 * u * u - ln
            elif kind == 2.0:
                ta = 0.0 if p1 == 1.0 else (p1 - 1.0) * np.log(x)
                tb = 0.0 if p2 == 1.0 else (p2 - 1.0) * np.log1p(-x)
                lp = ta + tb - ln
            else:
                lp = np.full(x.shape, -ln)
            out = out + np.where(np.isfinite(x) & (x >= lo) & (x <= hi), lp, -np.inf)
    return out


class DevicePrior:
    """Batched on-device draw_prior: `DevicePrior('basic')(B)` -> torch float32 [B, P] on the GPU.

    model: 'basic' (P=5) | 'single' (P=7) | 'scale' (P=8, gamma ~ U(0,2)).  Counter-based: row i of call c depends
    only on (seed, global row index), so shards of a batch drawn on different GPUs are consistent."""

    _NCOLS = {"basic": 5, "single": 7, "scale": 8}

    def __init__(self, model="basic", seed=2023, stream_state=None):
        if model not in self._NCOLS:
            raise ValueError(f"unknown prior model {model!r}")
        self.model = model
        self.state = stream_state or engine.StreamState(seed=seed)

    def __call__(self, batch_size, set_offset=None):
        seed, off = self.state.take(batch_size) if set_offset is None else (self.state.seed, set_offset)
        if self.model == "basic":
            return engine.draw_prior_device(engine.BASIC_DDM_DC, batch_size, seed=seed, set_offset=off)
        gamma = -1.0 if self.model == "scale" else 1.0
        out = engine.draw_prior_device(engine.SINGLE_TRIAL, batch_size, seed=seed, set_offset=off, gamma=gamma)
        return out[:, :self._NCOLS[self.model]].contiguous()


# ---------------------------------------------------------------------------------------------------------------
# Vectorised host draws of the same marginals (one SciPy call per column instead of three per parameter set):
# synthetic parameter matrices for benchmarks, tests and bulk simulation.  Same distributions as draw_prior_*,
# but a different (seeded, default_rng) stream -- use the call-for-call functions above for reference-identical draws.
def _tn_vec(rng, mean, sd, low, upp, size):
    return truncnorm.rvs((low - mean) / sd, (upp - mean) / sd, loc=mean, scale=sd, size=size, random_state=rng)


def basic_prior_matrix(B, seed=2023):
    """float32 [B, 5]: drift, boundary, beta, tau, dc  (basic_ddm_dc.py:62-80)."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.normal(0.0, 2.0, B), _tn_vec(rng, 1.0, .5, 0.0, 10.0, B), rng.beta(2.0, 2.0, B),
                     _tn_vec(rng, .5, .25, 0.0, 1.5, B), _tn_vec(rng, 1.0, .5, 0.0, 10.0, B)], axis=1).astype(np.float32)


def single_prior_matrix(B, seed=2023, gamma=1.0):
    """float32 [B, 8]: drift, mu_alpha, beta, ter, std_alpha, dc, sigma1, gamma  (single_trial_alpha_not_scaled.py:78-102)."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.normal(0.0, 2.0, B), _tn_vec(rng, 1.0, .5, 0.0, 10.0, B), rng.beta(2.0, 2.0, B),
                     _tn_vec(rng, .5, .25, 0.0, 1.5, B), _tn_vec(rng, 1.0, .5, 0.0, 3.0, B),
                     _tn_vec(rng, 1.0, .5, 0.0, 10.0, B), rng.uniform(0.0, 5.0, B), np.full(B, gamma)],
                    axis=1).astype(np.float32)


def alpha_ns_prior_matrix(B, seed=2021):
    """float32 [B, 6]: Nu, Alpha, Beta, Tau, Eta, Varsigma  (alpha_not_scaled.py:66-72)."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-4, 4, B), rng.uniform(.8, 1.4, B), rng.uniform(.3, .7, B), rng.uniform(.15, .6, B),
                     rng.uniform(0, 2, B), rng.uniform(.8, 1.4, B)], axis=1).astype(np.float32)
