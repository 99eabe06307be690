"""GPU tests of the single-trial model's marginal log-likelihood (include/nddm.h: nddm_wiener_marginal_log_likelihood;
csrc/nddm_wiener_marginal.h): accuracy against the float64 yardstick (tests/wiener_marginal_ref.py) at the shapes where the kernel's paths
change, the row sums' order, layout and capture independence of their bits, the special values from device tensors and host arrays, and
the two adapters.  The bars (wiener_marginal_ref.DEVICE_BAR) are 4 x the header's largest float32 error on the host, per row set."""
import numpy as np
import pytest

import wiener_marginal_ref as M

pytestmark = pytest.mark.gpu

# (D, S, N): paired layouts (S = 1) with N < 64, a partial last wave and workgroup, more than one LDS tile's worth of trials; broadcast
# layouts (S >= 16) with a partial last workgroup per data set and N no multiple of 64; (2, 17, 1025): S = 17 is the smallest S the plan
# stages (S >= 16) with S % 4 == 1, so each data set's last workgroup has one row and three waves that only stage, across two tiles
SHAPES = [(1, 1, 1), (5, 1, 65), (3, 1, 1025), (2, 16, 1), (2, 17, 130), (2, 17, 1025)]
K_TRIALS = 6              # distinct trials per data set; a data set of N trials cycles through them
GOOD = [0.8, 1.2, 0.45, 0.2, 0.5, 1.1, 0.7, 1.0]


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _case(name, D, S, N, want_ref=True):
    """Rows and data sets of one shape from the set `name`: data set d belongs to a row of the set that has a censored trial of its own
    (d = 0) or to the set's d-th row, and holds that row's own trial and K_TRIALS - 1 more drawn as the set draws them, cycled to N trials;
    its S rows are the set's row and S - 1 copies with drift, mu_alpha, std_alpha, dc and sigma1 moved by up to 3 % (draws around one
    posterior).  -> (float32 params [D * S, 8], float32 data [D, N, 2], t_censor, float64 yardstick [D * S, N])."""
    p32, y32, z32, tc = M.SETS[name](300)
    base = [int(np.flatnonzero(y32 == 0)[0])] + list(range(D - 1))
    pb = p32[base]
    ym, zm = M.more_trials(name, pb, K_TRIALS - 1, seed=23 + D + S + N)
    yk, zk = np.concatenate([y32[base, None], ym], 1), np.concatenate([z32[base, None], zm], 1)
    if N == 1 and D > 1:                                                # (one trial per data set: the first censored, the others responses)
        resp = np.argmax(yk[1:] != 0, 1)
        yk[1:, 0], zk[1:, 0] = yk[1:][np.arange(D - 1), resp], zk[1:][np.arange(D - 1), resp]
    rng = np.random.default_rng(D + S + N)
    rows = np.repeat(pb, S, 0).astype(np.float64)
    jit = 1.0 + 0.03 * rng.uniform(-1, 1, (D * S, 5))
    jit[::S] = 1.0
    rows[:, [0, 1, 4, 5, 6]] *= jit
    rows = rows.astype(np.float32)
    k = min(N, K_TRIALS)
    ref = np.zeros((D * S, k)) if not want_ref else M.pairs_log_lik(rows, np.repeat(yk[:, :k], S, 0), np.repeat(zk[:, :k], S, 0), tc)       # [D * S, k]
    idx = np.arange(N) % K_TRIALS
    data = np.stack([yk[:, idx], zk[:, idx]], -1).astype(np.float32)
    return rows, data, tc, ref[:, idx]


@pytest.mark.parametrize("name", ["prior_rows", "box"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(x) for x in s))
def test_accuracy_against_the_float64_yardstick(name, shape):
    torch = _torch()
    from bayesflow_nddms_amd import engine
    D, S, N = shape
    rows, data, tc, ref = _case(name, D, S, N)
    assert np.any(data[..., 0] == 0) and np.all(np.isfinite(ref))       # censored trials in every shape; the yardstick scores every pair
    r = engine.wiener_marginal_log_likelihood(engine.SINGLE_TRIAL, torch.as_tensor(rows).cuda(), torch.as_tensor(data).cuda(), draws_per_dataset=S,
                                              t_censor=tc, per_trial=True)
    assert r["loglik"].shape == (D * S,) and r["loglik"].dtype == torch.float64 and r["trial_logp"].shape == (D * S, N)
    got = r["trial_logp"].cpu().numpy().astype(np.float64)
    err = np.abs(got - ref)
    print(f"{name} {shape}: max |trial_logp - yardstick| = {err.max():.3g} (bar {M.DEVICE_BAR[name]:g}), log L in [{ref.min():.1f}, {ref.max():.1f}]")
    assert np.all(np.isfinite(got)) and err.max() <= M.DEVICE_BAR[name]
    # the row's sum is the trials' sum in the kernel's order: lane j adds trials j, j + 64, ... in float64, then a butterfly over the lanes
    part = np.zeros((D * S, 64))
    for i in range(N):
        part[:, i % 64] += got[:, i]
    lanes = np.arange(64)
    for m in (1, 2, 4, 8, 16, 32):
        part = part + part[:, lanes ^ m]
    assert np.array_equal(part[:, 0], r["loglik"].cpu().numpy())


def test_loglik_bits_do_not_depend_on_the_layout_or_on_a_capture():
    torch = _torch()
    from bayesflow_nddms_amd import engine
    D, S, N = 2, 32, 130
    rows, data, tc, _ = _case("prior_rows", D, S, N, want_ref=False)
    p, d = torch.as_tensor(rows).cuda(), torch.as_tensor(data).cuda()
    wl = lambda s, dd: engine.wiener_marginal_log_likelihood(engine.SINGLE_TRIAL, p, dd, draws_per_dataset=s, t_censor=tc)["loglik"]
    ref = wl(S, d)                                                       # broadcast layout, 2 x 32
    assert torch.isfinite(ref).all()
    for s in (16, 8, 1):                                                 # broadcast 4 x 16; paired 8 x 8 and 64 x 1 (repeated data sets)
        assert torch.equal(wl(s, d.repeat_interleave(S // s, 0)), ref), s
    # an eager call and one captured graph replayed twice (one stream, one kernel node)
    torch.cuda.synchronize()
    with engine.graph_memory():
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side), torch.cuda.graph(g, stream=side):
            out = wl(S, d)
        torch.cuda.synchronize()
        for _ in range(2):
            out.fill_(0.0)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, ref)
        del g


@pytest.mark.parametrize("on_device", [True, False], ids=["device_tensors", "host_arrays"])
def test_special_values(on_device):
    torch = _torch()
    from bayesflow_nddms_amd import engine
    give = (lambda x: torch.as_tensor(np.asarray(x, np.float32)).cuda()) if on_device else (lambda x: np.asarray(x, np.float64))
    tr = [[0.6, 1.0], [-0.9, 1.4], [0.0, 1.1], [0.15, 1.0], [0.2, 1.0], [0.7, float("nan")], [0.7, float("inf")]]
    call = lambda P, tc: engine.wiener_marginal_log_likelihood(engine.SINGLE_TRIAL, give(P), give([tr] * len(P)), t_censor=tc, per_trial=True)
    v = call([GOOD] * 3, 2.0)
    t, s = v["trial_logp"].cpu().numpy(), v["loglik"].cpu().numpy()
    assert np.all(np.isfinite(t[:, :3])) and np.all(t[:, 2] < 0)        # two responses and a timeout with t_censor
    assert np.all(t[:, 3] == -np.inf) and np.all(t[:, 4] == -np.inf)    # |y| < ter and |y| == ter
    assert np.all(np.isnan(t[:, 5:])) and np.all(np.isnan(s))           # a non-finite z1: that trial, and the sum it joins
    ref = M.pairs_log_lik(np.float32([GOOD]), np.float32([[0.6, -0.9, 0.0]]), np.float32([[1.0, 1.4, 1.1]]), 2.0)[0]
    assert np.all(np.abs(t[0, :3] - ref) <= M.DEVICE_BAR["prior_rows"])
    for tc in (None, 0.0):                                              # a timeout without a censoring time: NaN, the other trials unchanged
        o = call([GOOD], tc)["trial_logp"].cpu().numpy()[0]
        assert np.isnan(o[2]) and np.array_equal(o[:2], t[0, :2])
    if on_device:                                                       # (host arrays with such rows are refused before the launch: the CPU tests)
        bad = [list(GOOD) for _ in range(5)]
        bad[1][4] = 0.0
        bad[3][2] = 1.0
        o = call(bad, 2.0)
        ot, os_ = o["trial_logp"].cpu().numpy(), o["loglik"].cpu().numpy()
        assert np.all(np.isnan(ot[[1, 3]])) and np.all(np.isnan(os_))   # (every sum holds the NaN z1 trial)
        assert np.array_equal(ot[[0, 2, 4]], t, equal_nan=True)         # the neighbours unaffected
        fin = engine.wiener_marginal_log_likelihood(engine.SINGLE_TRIAL, give(bad), give([tr[:3]] * 5), t_censor=2.0)["loglik"].cpu().numpy()
        assert np.all(np.isnan(fin[[1, 3]])) and np.all(np.isfinite(fin[[0, 2, 4]])) and fin[0] == fin[2] == fin[4]


def test_single_trial_logpdf_broadcasts_in_one_call():
    torch = _torch()
    from bayesflow_nddms_amd import engine, likelihood
    y = np.array([0.6, -0.9, 0.0, 1.3], np.float32)
    z = np.array([1.0, 1.4, 1.1, 0.9], np.float32)
    mu = np.array([[1.0], [1.2], [1.5]], np.float32)                   # [3, 1] against [4]: one row per mu, four trials each
    out = likelihood.single_trial_logpdf(y, z, GOOD[0], mu, GOOD[2], GOOD[3], GOOD[4], GOOD[5], GOOD[6], t_censor=2.0)
    assert out.shape == (3, 4) and out.dtype == torch.float32 and torch.isfinite(out).all()
    rows = np.tile(np.float32(GOOD), (3, 1))
    rows[:, 1] = mu[:, 0]
    direct = engine.wiener_marginal_log_likelihood(engine.SINGLE_TRIAL, rows, np.tile(np.stack([y, z], -1), (3, 1, 1)), t_censor=2.0,
                                                   per_trial=True, want_sum=False)["trial_logp"]
    assert torch.equal(out, direct)
    # parameters that vary along the last axis: one row per element, the same values
    per = likelihood.single_trial_logpdf(y, z, GOOD[0], 1.2, GOOD[2], GOOD[3], np.full(4, GOOD[4], np.float32), GOOD[5], GOOD[6], gamma=1.0, t_censor=2.0)
    assert per.shape == (4,) and torch.equal(per, out[1])
    assert likelihood.single_trial_logpdf(0.6, 1.0, *GOOD[:7]).shape == ()
    assert torch.isnan(likelihood.single_trial_logpdf(0.0, 1.0, *GOOD[:7]))      # a timeout and no t_censor


def test_model_adapter_scores_its_own_simulators_output():
    torch = _torch()
    from bayesflow_nddms_amd import engine, single_trial_alpha_not_scaled as st
    params = np.array([[0.3, 1.6, 0.5, 0.3, 0.3, 0.7, 0.5], [1.5, 1.0, 0.4, 0.2, 0.2, 1.0, 1.0]])
    sim = st.batch_simulate_trials(params, 200, dt=.01, max_steps=100., seed=5, set_offset=0, as_numpy=False, with_summary=False)["sim_data"]
    assert (sim[0, :, 0] == 0).any()                                     # the slow row times out at the 1 s cap now and then
    ll = st.log_likelihood(params, sim, dt=.01, max_steps=100.)
    assert ll.shape == (2,) and ll.dtype == torch.float64 and torch.isfinite(ll).all()
    direct = engine.wiener_marginal_log_likelihood(engine.SINGLE_TRIAL, np.concatenate([params, np.ones((2, 1))], 1), sim, t_censor=1.0)["loglik"]
    assert torch.equal(ll, direct)
    # the data are likelier under the parameters that made them than under the other row's
    swapped = st.log_likelihood(params[::-1].copy(), sim, dt=.01, max_steps=100.)
    assert (ll > swapped).all()
    # one parameter set and its [n_trials, 2] data, as simulate_trials returns them
    one = st.log_likelihood(params[1], sim[1].cpu().numpy(), dt=.01, max_steps=100.)
    assert one.shape == (1,) and one[0] == ll[1]
