"""The call schedule of mcmc.hmc_fit and mcmc.hmc_fit_joint, without a compiler or a GPU: a recording fake in the engine call's place
(`_call`) whose draws encode their own position.  The launches the two fits make -- the two-stage warm-up, the cut of the sampling phase
into bounded launches -- are asserted literally, and every number of the returned JAGS layout must decode to the chain, the kept index and
the column it stands for."""
import numpy as np

from bayesflow_nddms_amd import engine, mcmc

CHAINS, WARMUP, SAMPLES, THIN, LEAPFROG, SEED = 3, 2000, 20000, 10, 16, 4
K_ALL = SAMPLES // THIN

WARMUP_CALLS = [(500, 1000, 0, 1, True, False, False), (500, 1000, 500, 1, True, True, False), (1000, 1000, 1000, 1, False, False, False)]
SAMPLING = [(16384, 2000), (3616, 18384)]                                                            # 2^19 / (16 x ceil(100 / 64))
SAMPLING_JOINT = [(4096, 2000), (4096, 6096), (4096, 10192), (4096, 14288), (3616, 18384)]        # min(16384, 4096)


def _data():
    rng = np.random.default_rng(3)
    return np.stack([rng.uniform(0.4, 1.2, (2, 100)), rng.choice([-1.0, 1.0], (2, 100))], -1).astype(np.float32)


class Fake:
    """The engine call's stand-in: records every call; a sampling launch's draws are c * 10000 + 5 * (kept index over the whole sampling
    phase) + j, its log_post -(c * 10000 + kept index), its sigma draws 100 * k + kept index; a warm-up launch's draws are a fixed pattern
    inside the support (they feed the mass estimate)."""

    def __init__(self, joint):
        self.joint, self.calls = joint, []

    def __call__(self, model, data, *rest, inv_mass=None, n_iter=1, n_adapt=0, thin=1, iter_offset=0, want_draws=True, want_log_post=True, **kw):
        ext, state, sigma = rest if self.joint else (None, rest[0], None)
        assert model == engine.BASIC_DDM_DC and data.shape == (2, 100, 2)
        i = len(self.calls)
        self.calls.append(dict(key=(n_iter, n_adapt, iter_offset, thin, inv_mass is None, want_draws, want_log_post), state=state, sigma=sigma,
                               ext=ext, inv_mass=inv_mass, kw=kw))
        C = state.shape[0]
        K = (iter_offset + n_iter) // thin - iter_offset // thin
        c, k, j = np.arange(C)[:, None, None], np.arange(K)[None, :, None], np.arange(5)[None, None, :]
        if iter_offset >= WARMUP:
            first = iter_offset // thin - WARMUP // thin
            draws = c * 10000 + 5 * (first + k) + j
            lp = -(c * 10000 + first + k)[:, :, 0]
        else:
            first = 0
            draws = np.array([0.5, 1.0, 0.5, 0.1, 1.0]) + 0.01 * ((c + k * (j + 1)) % 7)
            lp = np.zeros((C, K))
        r = {"accept": np.full(C, 0.5 + 0.01 * i, np.float32), "divergent": np.ones(C, np.int32), "flagged": np.zeros(C, np.int32), "state": state}
        if want_draws:
            r["draws"] = draws.astype(np.float32)
        if want_log_post:
            r["log_post"] = lp.astype(np.float32)
        if self.joint:
            S = len(sigma)
            r.update(sigma_draws=(100 * np.arange(S)[:, None] + first + np.arange(K)[None, :]).astype(np.float32),
                     sigma_accept=np.full(S, 0.2 + 0.01 * i, np.float32), sigma=sigma)
        return r


def _fit(joint):
    fake, d = Fake(joint), _data()
    kw = dict(chains=CHAINS, warmup=WARMUP, samples=SAMPLES, thin=THIN, n_leapfrog=LEAPFROG, seed=SEED, _call=fake)
    out = mcmc.hmc_fit_joint(d, np.array([1.0, 1.5]), **kw) if joint else mcmc.hmc_fit(d, **kw)
    return fake, d, out


def _weighted(plan, const):
    """The n_iter-weighted mean of a per-launch constant over the sampling launches (calls 3, 4, ...: after the warm-up's three)."""
    n = np.array([p[0] for p in plan], np.float64)
    return sum(np.float64(np.float32(const(i + 3))) * w for i, w in enumerate(n)) / n.sum()


def _check_common(fake, d, out, plan):
    assert [c["key"] for c in fake.calls] == WARMUP_CALLS + [(n, 1000, off, THIN, False, True, True) for n, off in plan]
    # the first state is hmc_init's draws, in its order; every call carries the options
    theta = mcmc.hmc_init(d, CHAINS, SEED).reshape(-1, 5)
    assert np.array_equal(fake.calls[0]["state"][:, :5], mcmc.theta_to_q(theta, np.repeat(d, CHAINS, 0)))
    assert fake.calls[0]["state"].shape == (6, engine.WHMC_STATE)
    for c in fake.calls:
        assert c["kw"]["n_leapfrog"] == LEAPFROG and c["kw"]["free_mask"] == 31 and c["kw"]["seed"] == SEED
    assert np.array_equal(fake.calls[2]["inv_mass"], fake.calls[-1]["inv_mass"]) and fake.calls[2]["inv_mass"].shape == (6, 5)
    dd, kk, cc = np.meshgrid(np.arange(2), np.arange(K_ALL), np.arange(CHAINS), indexing="ij")
    for j, name in enumerate(mcmc.PARAM_NAMES):
        v = out[mcmc.JAGS_NAMES[name]]
        assert v.shape == (2, K_ALL, CHAINS) and v.dtype == np.float64
        assert np.array_equal(v, (dd * CHAINS + cc) * 10000 + 5 * kk + j), name
    assert out["log_post"].dtype == np.float64 and np.array_equal(out["log_post"], -((dd * CHAINS + cc) * 10000 + kk))
    assert out["accept_rate"].shape == (2, CHAINS)
    np.testing.assert_allclose(out["accept_rate"], _weighted(plan, lambda i: 0.5 + 0.01 * i), rtol=1e-13)
    assert out["n_divergent"].shape == (2, CHAINS) and out["n_divergent"].dtype == np.int64 and np.all(out["n_divergent"] == len(plan))
    assert out["flagged"].shape == (2, CHAINS) and not out["flagged"].any()


def test_hmc_fit_makes_the_launches_of_its_schedule_and_lays_the_draws_out():
    fake, d, out = _fit(False)
    _check_common(fake, d, out, SAMPLING)
    assert all(c["kw"]["chains_per_dataset"] == CHAINS and "sigma_fixed" not in c["kw"] for c in fake.calls)
    assert set(out) == {"alpha", "ndt", "beta", "delta", "varsigma", "log_post", "accept_rate", "n_divergent", "flagged"}


def test_hmc_fit_joint_makes_the_launches_of_its_schedule_and_lays_the_draws_out():
    fake, d, out = _fit(True)
    _check_common(fake, d, out, SAMPLING_JOINT)
    sigma0 = mcmc.hmc_init_joint(d, CHAINS, SEED)[1]
    for c in fake.calls:
        assert c["kw"]["sigma_fixed"] is False and "chains_per_dataset" not in c["kw"]
        assert np.array_equal(c["sigma"], sigma0) and np.array_equal(c["ext"], [1.0, 1.5]) and c["ext"].dtype == np.float64
    assert out["sigma"].shape == (1, K_ALL, CHAINS) and out["sigma"].dtype == np.float64
    assert np.array_equal(out["sigma"][0], 100 * np.arange(CHAINS)[None, :] + np.arange(K_ALL)[:, None])
    assert out["sigma_accept"].shape == (CHAINS,)
    np.testing.assert_allclose(out["sigma_accept"], _weighted(SAMPLING_JOINT, lambda i: 0.2 + 0.01 * i), rtol=1e-13)
    assert set(out) == {"alpha", "ndt", "beta", "delta", "varsigma", "log_post", "accept_rate", "n_divergent", "flagged", "sigma", "sigma_accept"}


def test_both_fits_hand_the_sampler_the_same_mass_for_the_same_stage_two_draws():
    a, b = _fit(False)[0], _fit(True)[0]
    assert a.calls[2]["inv_mass"] is not None and np.array_equal(a.calls[2]["inv_mass"], b.calls[2]["inv_mass"])
    assert np.all(a.calls[2]["inv_mass"] >= 1e-3) and np.ptp(a.calls[2]["inv_mass"]) > 0
