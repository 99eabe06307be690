"""GPU tests of the gradient of the single-trial model's marginal log-likelihood (include/nddm.h: nddm_wiener_marginal_log_likelihood_grad;
csrc/nddm_wiener_marginal_grad.h): the value's bits against the forward kernel's, the gradient against the float64 yardstick
(tests/wiener_marginal_grad_ref.py) at the shapes where the kernel's paths change -- censored trials in every one -- layout and capture
independence of its bits, the special values, and the autograd binding.  The bars (wiener_marginal_grad_ref.DEVICE_BAR) are 4 x the header's
largest float32 error over scale_j on the host, per row set."""
import functools

import numpy as np
import pytest

import wiener_marginal_grad_ref as MG
from test_gpu_wiener_marginal import GOOD, SHAPES, _case

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@functools.lru_cache(maxsize=None)
def _grad_case(name, D, S, N):
    """test_gpu_wiener_marginal's rows and data sets of one shape, and the yardstick: -> (rows, data, t_censor, the rows' gradients
    [D * S, 8], their scales [D * S, 8] = the sum over the row's trials of |per-trial gradient|)."""
    rows, data, tc, _ = _case(name, D, S, N, want_ref=False)
    k = min(N, data.shape[1], 6)                                        # the data set cycles through its first 6 trials
    # (the rule with the finer panels alone: that the coarser one agrees with it is the CPU tests' business, on the sets' own rows)
    per = MG.pairs_grad(rows, np.repeat(data[:, :k, 0], S, 0), np.repeat(data[:, :k, 1], S, 0), tc, check=False)      # [D * S, k, 8]
    count = np.bincount(np.arange(N) % 6, minlength=k)[:k].astype(np.float64)
    return rows, data, tc, np.einsum("k,rkj->rj", count, per), np.einsum("k,rkj->rj", count, np.abs(per))


@pytest.mark.parametrize("name", ["prior_rows", "box"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(x) for x in s))
def test_value_bits_and_gradient_accuracy(name, shape):
    torch = _torch()
    from bayesflow_nddms_amd import engine
    D, S, N = shape
    rows, data, tc, ref, scale = _grad_case(name, D, S, N)
    assert np.any(data[..., 0] == 0) and np.all(np.isfinite(ref))       # censored trials in every shape; the yardstick scores every pair
    p, d = torch.as_tensor(rows).cuda(), torch.as_tensor(data).cuda()
    r = engine.wiener_marginal_log_likelihood_grad(engine.SINGLE_TRIAL, p, d, draws_per_dataset=S, t_censor=tc)
    assert r["loglik"].shape == (D * S,) and r["loglik"].dtype == torch.float64 and r["grad"].shape == (D * S, 8) and r["grad"].dtype == torch.float64
    fwd = engine.wiener_marginal_log_likelihood(engine.SINGLE_TRIAL, p, d, draws_per_dataset=S, t_censor=tc)["loglik"]
    assert torch.isfinite(fwd).all() and torch.equal(r["loglik"], fwd)   # bit for bit
    got = r["grad"].cpu().numpy()
    assert np.all(np.isfinite(got))
    with np.errstate(all="ignore"):                                     # (a scale of 0 -- ter's, where every trial is a timeout: the two must be equal)
        rel = np.where(scale > 0, np.abs(got - ref) / scale, np.where(got == ref, 0.0, np.inf))
    print(f"{name} {shape}: max |grad - yardstick| / scale per column = {np.array2string(rel.max(0), precision=2)} (bar {MG.DEVICE_BAR[name]:g}), "
          f"|d| up to {np.abs(ref).max():.3g}")
    assert rel.max() <= MG.DEVICE_BAR[name]


def test_gradient_bits_do_not_depend_on_the_layout_or_on_a_capture():
    torch = _torch()
    from bayesflow_nddms_amd import engine
    D, S, N = 2, 32, 130
    rows, data, tc, _ = _case("prior_rows", D, S, N, want_ref=False)
    p, d = torch.as_tensor(rows).cuda(), torch.as_tensor(data).cuda()
    wl = lambda s, dd: engine.wiener_marginal_log_likelihood_grad(engine.SINGLE_TRIAL, p, dd, draws_per_dataset=s, t_censor=tc)
    ref = wl(S, d)                                                       # broadcast layout, 2 x 32
    assert torch.isfinite(ref["grad"]).all() and torch.isfinite(ref["loglik"]).all()
    for s in (16, 8, 1):                                                 # broadcast 4 x 16; paired 8 x 8 and 64 x 1 (repeated data sets)
        o = wl(s, d.repeat_interleave(S // s, 0))
        assert torch.equal(o["grad"], ref["grad"]) and torch.equal(o["loglik"], ref["loglik"]), s
    # an eager call and one captured graph replayed twice (one stream, one kernel node)
    torch.cuda.synchronize()
    with engine.graph_memory():
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side), torch.cuda.graph(g, stream=side):
            out = wl(S, d)
        torch.cuda.synchronize()
        for _ in range(2):
            out["grad"].fill_(0.0)
            out["loglik"].fill_(0.0)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out["grad"], ref["grad"]) and torch.equal(out["loglik"], ref["loglik"])
        del g


def test_special_values():
    torch = _torch()
    from bayesflow_nddms_amd import engine
    give = lambda x: torch.as_tensor(np.asarray(x, np.float32)).cuda()
    tr = [[0.6, 1.0], [-0.9, 1.4], [1.3, 0.9]]
    odd = [tr[0], [0.0, 1.1], tr[2]]                                    # its only oddity: a timeout

    def call(P, D, tc=2.0):
        r = engine.wiener_marginal_log_likelihood_grad(engine.SINGLE_TRIAL, give(P), give(D), t_censor=tc)
        return r["loglik"].cpu().numpy(), r["grad"].cpu().numpy()
    bad = [list(GOOD) for _ in range(7)]
    bad[1][4] = 0.0
    bad[3][2] = 1.0
    bad[5][0] = float("nan")
    ll, g = call(bad, [odd] * 7)
    assert np.all(np.isnan(ll[[1, 3, 5]])) and np.all(np.isnan(g[[1, 3, 5]]))           # invalid rows: NaN in the value and in every column
    ok = [0, 2, 4, 6]
    assert np.all(np.isfinite(ll[ok])) and np.all(np.isfinite(g[ok]))                    # a timeout gets a FINITE gradient
    assert np.array_equal(ll[ok], np.repeat(ll[0], 4)) and np.array_equal(g[ok], np.tile(g[0], (4, 1)))      # the neighbours unaffected
    p32, d32 = np.float32([GOOD]), np.float32([odd])
    ref = MG.pairs_grad(p32, d32[..., 0], d32[..., 1], 2.0)[0]
    assert np.all(np.abs(g[0] - ref.sum(0)) <= MG.DEVICE_BAR["prior_rows"] * np.abs(ref).sum(0))
    plain = call([GOOD], [tr])
    assert np.all(np.isfinite(plain[1])) and np.any(np.abs(plain[1] - g[0]) > 1e-3)       # (the timeout moved it)
    # one odd trial among valid ones, rows 1.. ; row 0 is the plain one and stays as it is
    cases = [([0.15, 1.0], -np.inf), ([0.2, 1.0], -np.inf),             # |y| < ter, |y| == ter: -inf and a NaN row gradient
             ([0.7, float("nan")], np.nan), ([0.7, float("inf")], np.nan), ([float("nan"), 1.0], np.nan)]
    ll, g = call([GOOD] * (1 + len(cases)), [tr] + [[tr[0], c, tr[2]] for c, _ in cases])
    assert ll[0] == plain[0][0] and np.array_equal(g[0], plain[1][0])
    for i, (_, want) in enumerate(cases, 1):
        assert (np.isnan(ll[i]) if want != want else ll[i] == want) and np.all(np.isnan(g[i])), i
    for tc in (None, 0.0):                                              # a timeout without a censoring time: NaN in both; a row without one: unchanged
        ll, g = call([GOOD, GOOD], [odd, tr], tc)
        assert np.isnan(ll[0]) and np.all(np.isnan(g[0])) and ll[1] == plain[0][0] and np.array_equal(g[1], plain[1][0])
    # every node at -inf (z1 so far out that the Gaussian factor underflows at every boundary): -inf and NaN
    ll, g = call([GOOD], [[[0.6, 1e30]]])
    assert ll[0] == -np.inf and np.all(np.isnan(g))


def test_autograd_makes_one_launch_and_returns_thetas_dtype():
    torch = _torch()
    from bayesflow_nddms_amd import engine, likelihood, single_trial_alpha_not_scaled as st
    rows, data, tc, ref, scale = _grad_case("prior_rows", 5, 1, 65)
    d = torch.as_tensor(data).cuda()
    direct = engine.wiener_marginal_log_likelihood_grad(engine.SINGLE_TRIAL, torch.as_tensor(rows).cuda(), d, t_censor=tc)
    for dtype in (torch.float32, torch.float64):
        theta = torch.as_tensor(rows).to(dtype).cuda().requires_grad_(True)
        n0 = engine.wiener_marginal_grad_launches()
        ll = likelihood.single_trial_loglik(theta, d, t_censor=tc)
        (-ll.sum()).backward()
        assert engine.wiener_marginal_grad_launches() == n0 + 1          # the forward's one launch; the backward makes none
        assert theta.grad.dtype == dtype and theta.grad.shape == theta.shape and theta.grad.is_cuda
        assert torch.equal(ll.detach(), direct["loglik"]) and torch.equal(theta.grad, (-direct["grad"]).to(dtype))
    # a host tensor: the gradient comes back to the host in its dtype; nothing requiring grad: the same values
    th = torch.as_tensor(rows, dtype=torch.float64).requires_grad_(True)
    (-likelihood.single_trial_loglik(th, d, t_censor=tc).sum()).backward()
    assert not th.grad.is_cuda and th.grad.dtype == torch.float64 and torch.equal(th.grad, -direct["grad"].cpu())
    assert torch.equal(likelihood.single_trial_loglik(torch.as_tensor(rows).cuda(), d, t_censor=tc), direct["loglik"])
    # the model's adapter: its own simulator's output, timeouts included; gamma's column dropped
    params = np.array([[0.3, 1.6, 0.5, 0.3, 0.3, 0.7, 0.5], [1.5, 1.0, 0.4, 0.2, 0.2, 1.0, 1.0]])
    sim = st.batch_simulate_trials(params, 200, dt=.01, max_steps=100., seed=5, set_offset=0, as_numpy=False, with_summary=False)["sim_data"]
    assert (sim[0, :, 0] == 0).any()
    ll, g = st.log_likelihood_and_grad(params, sim, dt=.01, max_steps=100.)
    assert g.shape == (2, 7) and g.dtype == torch.float64 and torch.isfinite(g).all()
    assert torch.equal(ll, st.log_likelihood(params, sim, dt=.01, max_steps=100.))
