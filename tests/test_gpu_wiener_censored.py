"""GPU tests of NDDM_WIENER_CENSORED in the Wiener log-likelihood's gradient (engine.wiener_log_likelihood_grad(..., censored=True) ->
nddm_wiener_log_likelihood_grad's flag 4 -> wiener_grad_kernel<basic, layout, censored>; csrc/nddm_wiener_grad.h): rows with 10 % timeouts
against the float64 yardstick (tests/wiener_censored_ref.py) at the shapes where the kernel's paths change, the value's bits against
nddm_wiener_log_likelihood, the flag's neutrality where nothing is censored, layout independence, the special values, and autograd.
The bar (wiener_censored_ref.BAR, in units of the per-column condition scale) is the host test's."""
import numpy as np
import pytest

import wiener_censored_ref as R

pytestmark = pytest.mark.gpu

PAIRED = [(1, 1), (15, 65), (17, 1025), (33, 63)]                      # (R, N): N < 64, a partial last wave / workgroup, two LDS tiles' worth
STAGED = [(2, 16, 1), (3, 17, 1025), (2, 31, 2049)]                    # (D, S, N): a partial last workgroup per data set, three tiles
TAU = (0.20, 0.22)
SURV_U = 0.06                                                           # WIENER_SURV_U


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _rows(n, rng):
    """Distinct rows with a' in [1.09, 2.0] (the crossover of log S at t in [0.071, 0.24]), |v'| <= 1.12 and tau in [0.20, 0.22]."""
    return np.stack([rng.uniform(-1, 1, n), rng.uniform(1.2, 1.8, n), rng.uniform(0.2, 0.8, n), rng.uniform(*TAU, n),
                     rng.uniform(0.9, 1.1, n)], 1).astype(np.float32)


def _trials(D, N, rng, censored=True):
    """[D, N, 2] = (rt, choice): responses at rt in [0.35, 2.0] above every row's tau; with `censored` every tenth trial (and the only one
    of data set 0 when N == 1) is a timeout, in turn at rt 0.235 / 0.26 (t <= 0.06: below every row's crossover) and in [0.5, 1.1]
    (t >= 0.28: above it), and trial 13 of data set 0 is a timeout at rt = 0.1 <= tau."""
    rt = rng.uniform(0.35, 2.0, (D, N))
    ch = np.where(rng.random((D, N)) < 0.5, 1.0, -1.0)
    if censored:
        idx = np.arange(3, N, 10) if N > 3 else np.arange(0)
        small = np.where(np.arange(idx.size) % 4 == 0, 0.235, 0.26)
        for d in range(D):
            rt[d, idx] = np.where(np.arange(idx.size) % 2 == 0, small, rng.uniform(0.5, 1.1, idx.size))
            ch[d, idx] = 0.0
        if N == 1:
            rt[0, 0], ch[0, 0] = 0.8, 0.0
        if N > 13:
            rt[0, 13], ch[0, 13] = 0.1, 0.0
    return np.stack([rt, ch], -1).astype(np.float32)


def _yardstick(p32, d32, S):
    """float64 (gradient, scale) of rows p32 against data sets d32 (row r scores set r // S), at the kernel's float32 t = rt - tau; every
    timeout with t > 0 has the yardstick's `ok`, and a row with two of them or more has them on both sides of the crossover."""
    d = np.repeat(d32, S, 0)
    t = (d[..., 0] - p32[:, 3:4]).astype(np.float32).astype(np.float64)
    code = d[..., 1].astype(np.float64)
    p = p32.astype(np.float64)
    cens = (code == 0) & (t > 0)
    _, ok = R.log_survival(p[:, None, :], np.where(cens, t, 1e-3))
    assert np.all(ok)
    u = t / (p[:, 1:2] / p[:, 4:5]) ** 2
    many = cens.sum(1) >= 2
    assert np.all(np.any(cens & (u < SURV_U), 1)[many]) and np.all(np.any(cens & (u >= SURV_U), 1)[many])
    return R.row_grad(p, t, code)


def _check(name, got, ref, scale):
    err = np.abs(got - ref) / scale
    print(f"{name}: max |gradient - yardstick| / scale per column {np.array2string(err.max(0), precision=2)}")
    assert np.all(np.isfinite(got)) and np.all(err <= R.BAR), (name, err.max(0))


@pytest.mark.parametrize("shape", PAIRED + STAGED, ids=lambda s: "x".join(str(x) for x in s))
def test_gradient_with_timeouts_against_float64_and_the_values_bits(shape):
    """Fails without the feature: flags = 4 is NDDM_ERR_PARAM there (and censored= is no keyword of the engine call)."""
    torch = _torch()
    from bayesflow_nddms_amd import engine
    rng = np.random.default_rng(sum(shape))
    (D, S, N) = shape if len(shape) == 3 else (shape[0], 1, shape[1])
    p32, d32 = _rows(D * S, rng), _trials(D, N, rng)
    assert np.any(d32[..., 1] == 0)
    if N > 13:
        assert abs(np.mean(d32[..., 1] == 0) - 0.1) < 0.02 and d32[0, 13, 0] < TAU[0]
    p, d = torch.as_tensor(p32).cuda(), torch.as_tensor(d32).cuda()
    r = engine.wiener_log_likelihood_grad(engine.BASIC_DDM_DC, p, d, draws_per_dataset=S, censored=True)
    assert r["loglik"].shape == (D * S,) and r["grad"].shape == (D * S, 5) and r["grad"].dtype == torch.float64
    ref, scale = _yardstick(p32, d32, S)
    _check(f"{shape}", r["grad"].cpu().numpy(), ref, scale)
    # the value: bit for bit the forward kernel's sum, and the unflagged gradient kernel's
    fwd = engine.wiener_log_likelihood(engine.BASIC_DDM_DC, p, d, draws_per_dataset=S)["loglik"]
    assert torch.equal(r["loglik"], fwd) and torch.isfinite(fwd).all()
    r0 = engine.wiener_log_likelihood_grad(engine.BASIC_DDM_DC, p, d, draws_per_dataset=S)
    has = torch.as_tensor(np.repeat((d32[..., 1] == 0).any(1), S)).cuda()
    assert torch.equal(r0["loglik"], fwd) and torch.isnan(r0["grad"][has]).all() and torch.equal(r0["grad"][~has], r["grad"][~has])


def test_one_timeout_alone_is_its_own_partials():
    """(1, 1) with its one trial censored, at three decision times: the row's gradient is the timeout's, to 1e-4 of each partial's size
    (scale_j is |partial| itself here), with d/dtau = (f_lower + f_upper) / S > 0."""
    torch = _torch()
    from bayesflow_nddms_amd import engine
    p32 = np.array([[0.6, 1.4, 0.4, 0.2, 1.0]], np.float32)
    for rt in (0.25, 0.5, 1.0):
        d32 = np.array([[[rt, 0.0]]], np.float32)
        g = engine.wiener_log_likelihood_grad(engine.BASIC_DDM_DC, torch.as_tensor(p32).cuda(), torch.as_tensor(d32).cuda(), censored=True)["grad"]
        own = R.timeout_grad(p32[0].astype(np.float64), float(np.float32(rt) - np.float32(0.2)))
        err = np.abs(g.cpu().numpy()[0] - own) / np.abs(own)
        print(f"rt {rt}: partials {np.array2string(own, precision=4)}, relative error {np.array2string(err, precision=2)}")
        assert np.all(err <= 1e-4) and own[3] > 0


@pytest.mark.parametrize("shape", [(33, 1, 63), (3, 17, 1025)], ids=["paired", "broadcast"])
def test_the_flag_changes_no_bit_where_nothing_is_censored(shape):
    torch = _torch()
    from bayesflow_nddms_amd import engine
    rng = np.random.default_rng(5)
    D, S, N = shape
    p = torch.as_tensor(_rows(D * S, rng)).cuda()
    d = torch.as_tensor(_trials(D, N, rng, censored=False)).cuda()
    a = engine.wiener_log_likelihood_grad(engine.BASIC_DDM_DC, p, d, draws_per_dataset=S, censored=True)
    b = engine.wiener_log_likelihood_grad(engine.BASIC_DDM_DC, p, d, draws_per_dataset=S)
    assert torch.equal(a["loglik"], b["loglik"]) and torch.equal(a["grad"], b["grad"]) and torch.isfinite(a["grad"]).all()


def test_gradient_bits_with_timeouts_do_not_depend_on_the_layout():
    torch = _torch()
    from bayesflow_nddms_amd import engine
    rng = np.random.default_rng(9)
    D, S, N = 2, 32, 1100                                                # N > one LDS tile
    p = torch.as_tensor(_rows(D * S, rng)).cuda()
    d = torch.as_tensor(_trials(D, N, rng)).cuda()
    wl = lambda s, data: engine.wiener_log_likelihood_grad(engine.BASIC_DDM_DC, p, data, draws_per_dataset=s, censored=True)
    ref = wl(S, d)                                                       # broadcast layout, 2 x 32
    assert torch.isfinite(ref["grad"]).all() and (d[..., 1] == 0).sum() >= 200
    for s in (16, 8, 4, 1):                                              # broadcast 4 x 16; paired 8 x 8, 16 x 4 and 64 x 1 (repeated data sets)
        r = wl(s, d.repeat_interleave(S // s, 0))
        assert torch.equal(r["grad"], ref["grad"]) and torch.equal(r["loglik"], ref["loglik"]), s
    # the same row repeated 16 times on one data set (broadcast) against the row alone (paired)
    kw = dict(censored=True)
    one = engine.wiener_log_likelihood_grad(engine.BASIC_DDM_DC, p[:3], d[:1].repeat_interleave(3, 0), **kw)
    rep = engine.wiener_log_likelihood_grad(engine.BASIC_DDM_DC, p[:3].repeat_interleave(16, 0), d[:1].repeat_interleave(3, 0), draws_per_dataset=16, **kw)
    assert torch.equal(rep["grad"], one["grad"].repeat_interleave(16, 0)) and torch.equal(one["grad"], ref["grad"][:3])


def test_special_values_on_the_device():
    torch = _torch()
    from bayesflow_nddms_amd import _lib, engine
    rng = np.random.default_rng(4)
    P = _rows(9, rng)
    data = torch.as_tensor(_trials(9, 70, rng)).cuda()
    wl = lambda p, d: engine.wiener_log_likelihood_grad(engine.BASIC_DDM_DC, torch.as_tensor(p).cuda(), d, censored=True)
    good = wl(P, data)
    assert torch.isfinite(good["grad"]).all() and torch.isfinite(good["loglik"]).all()
    # invalid rows between valid ones: NaN there only
    bad = P.copy()
    bad[1, 0] = np.nan; bad[3, 1] = 0.0; bad[5, 2] = 1.0; bad[6, 4] = -1.0
    r = wl(bad, data)
    for i in range(9):
        if i in (1, 3, 5, 6):
            assert torch.isnan(r["loglik"][i]) and torch.isnan(r["grad"][i]).all(), i
        else:
            assert torch.equal(r["loglik"][i], good["loglik"][i]) and torch.equal(r["grad"][i], good["grad"][i]), i
    # a NaN rt on a timeout, a choice of 2 and a NaN choice: NaN in that row's gradient only
    for (row, trial), (rt, ch) in (((2, 23), (np.nan, 0.0)), ((4, 5), (0.9, 2.0)), ((7, 68), (0.9, np.nan)), ((0, 3), (np.inf, 0.0))):
        d2 = data.clone()
        d2[row, trial, 0], d2[row, trial, 1] = rt, ch
        r2 = wl(P, d2)
        assert torch.isnan(r2["grad"][row]).all(), (row, trial)
        keep = [i for i in range(9) if i != row]
        assert torch.equal(r2["grad"][keep], good["grad"][keep]) and torch.equal(r2["loglik"][keep], good["loglik"][keep])
        fwd = engine.wiener_log_likelihood(engine.BASIC_DDM_DC, torch.as_tensor(P).cuda(), d2)["loglik"]
        same = lambda a, b: torch.equal(torch.nan_to_num(a, nan=1.0e300), torch.nan_to_num(b, nan=1.0e300))
        assert same(r2["loglik"], fwd)                                   # (NaN where the forward kernel's is)
    # a response at rt <= tau is still -inf in the value and NaN in the gradient; a timeout there adds nothing (data set 0's trial 13)
    d3 = data.clone()
    d3[4, 5, 0], d3[4, 5, 1] = 0.05, 1.0
    r3 = wl(P, d3)
    assert r3["loglik"][4] == -float("inf") and torch.isnan(r3["grad"][4]).all() and torch.equal(r3["grad"][:4], good["grad"][:4])
    assert data[0, 13, 1] == 0 and data[0, 13, 0] < P[0, 3]
    d4 = data.clone()
    d4[0, 13, 0] = -3.0
    r4 = wl(P, d4)
    assert torch.equal(r4["grad"], good["grad"]) and torch.equal(r4["loglik"], good["loglik"])
    # alpha_not_scaled with the flag: ValueError from the adapter, NDDM_ERR_PARAM from the entry point
    pa = torch.tensor([[1.0, 1.0, 0.5, 0.2, 0.5, 1.3]]).cuda()
    da = torch.tensor([[[0.5, 1.0], [-0.7, 0.0]]]).cuda()
    with pytest.raises(ValueError, match="BASIC_DDM_DC only"):
        engine.wiener_log_likelihood_grad(engine.ALPHA_NOT_SCALED, pa, da, censored=True)
    out = torch.zeros(1, 6, dtype=torch.float64).cuda()
    L = _lib.lib()
    rc = L.nddm_wiener_log_likelihood_grad(engine.ALPHA_NOT_SCALED, engine._ptr(pa), 1, 1, engine._ptr(da), 2, _lib.WIENER_CENSORED, None,
                                           engine._ptr(out), None)
    assert rc == _lib.NDDM_ERR_PARAM and b"NDDM_WIENER_CENSORED takes NDDM_BASIC_DDM_DC only" in L.nddm_last_error()
    torch.cuda.synchronize()
    assert (out == 0).all()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_autograd_through_timeouts_is_the_kernels_gradient_in_one_launch(dtype):
    torch = _torch()
    from bayesflow_nddms_amd import basic_ddm_dc, engine, likelihood
    dt = getattr(torch, dtype)
    rng = np.random.default_rng(12)
    D, S, N = 2, 5, 90
    base = torch.as_tensor(_rows(D * S, rng).astype(np.float64), dtype=dt).cuda()
    raw = torch.zeros(D * S, 5, dtype=dt).cuda().requires_grad_(True)
    data = torch.as_tensor(_trials(D, N, rng)).cuda().requires_grad_(True)
    go = torch.as_tensor(rng.normal(size=D * S)).cuda()
    n0 = engine.wiener_grad_launches()
    params = base * torch.exp(0.1 * raw)
    ll = likelihood.wiener_loglik(engine.BASIC_DDM_DC, params, data, draws_per_dataset=S, censored=True)
    assert ll.dtype == torch.float64 and ll.shape == (D * S,) and ll.requires_grad
    ll.backward(go)
    assert engine.wiener_grad_launches() == n0 + 1                      # one launch per forward plus backward
    assert data.grad is None and raw.grad is not None and raw.grad.dtype == dt and torch.isfinite(raw.grad).all()
    raw2 = raw.detach().clone().requires_grad_(True)
    params2 = base * torch.exp(0.1 * raw2)
    r = engine.wiener_log_likelihood_grad(engine.BASIC_DDM_DC, params2.detach(), data.detach(), draws_per_dataset=S, censored=True)
    params2.backward((go[:, None] * r["grad"]).to(dt))
    assert torch.equal(ll.detach(), r["loglik"]) and torch.equal(raw.grad, raw2.grad) and raw.grad.abs().max() > 0
    # without the keyword the same rows have no gradient
    raw3 = raw.detach().clone().requires_grad_(True)
    likelihood.wiener_loglik(engine.BASIC_DDM_DC, base * torch.exp(0.1 * raw3), data.detach(), draws_per_dataset=S).backward(go)
    assert torch.isnan(raw3.grad).all()
    # the model adapter is the engine call
    v, g = basic_ddm_dc.log_likelihood_and_grad(params.detach(), data.detach(), censored=True)
    assert torch.equal(v, r["loglik"]) and torch.equal(g, r["grad"])


def test_gradient_ascent_on_simulated_data_with_timeouts_raises_the_log_likelihood():
    torch = _torch()
    from bayesflow_nddms_amd import basic_ddm_dc, engine, likelihood
    truth = np.array([0.3, 1.6, 0.5, 0.3, 1.0])                          # a slow process: a share of the trials runs into the 1 s horizon
    y = basic_ddm_dc.batch_simulate_trials(truth[None].astype(np.float32), 600, dt=.01, max_steps=100., seed=21, set_offset=0, as_numpy=False,
                                           with_summary=False)["sim_data"]
    n_timeouts = int((y[..., 1] == 0).sum())
    assert 20 <= n_timeouts <= 400, n_timeouts
    start = truth * np.array([1.5, 0.8, 1.2, 0.8, 1.2])
    theta = torch.as_tensor(start[None]).cuda().requires_grad_(True)
    opt = torch.optim.Adam([theta], lr=0.002)                            # 20 steps move a parameter by 0.04 at the most
    first = None
    for _ in range(20):
        opt.zero_grad()
        ll = likelihood.wiener_loglik(engine.BASIC_DDM_DC, theta, y, censored=True)
        first = float(ll.detach()) if first is None else first
        (-ll.sum()).backward()
        assert torch.isfinite(theta.grad).all()
        opt.step()
    last = float(likelihood.wiener_loglik(engine.BASIC_DDM_DC, theta.detach(), y, censored=True))
    print(f"{n_timeouts} timeouts of 600 trials: log-likelihood {first:.3f} -> {last:.3f} after 20 Adam steps")
    assert np.isfinite(first) and last > first
