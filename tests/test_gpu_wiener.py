"""GPU tests of the Wiener first-passage log-likelihood (include/nddm.h: nddm_wiener_log_likelihood; csrc/nddm_wiener.h): pointwise
accuracy against the float64 yardstick (tests/wiener_ref.py), normalisation of the device density, agreement with the product's exact
sampler, the censored timeouts, layout / launch / stream / capture independence of the bits, the special rows, a recovery scan, and
the posterior helper."""
import os
import threading

import numpy as np
import pytest

import wiener_ref as W
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _simpson_log_grid(x0, x1, n):
    """Nodes and Simpson weights of int_x0^x1 f(x) dx on a grid uniform in log x (n odd)."""
    s = np.linspace(np.log(x0), np.log(x1), n)
    h = s[1] - s[0]
    w = np.ones(n)
    w[1:-1:2], w[2:-1:2] = 4.0, 2.0
    x = np.exp(s)
    return x, w * h / 3.0 * x


def test_pointwise_accuracy_against_the_float64_yardstick():
    torch = _torch()
    from bayesflow_nddms_amd import engine
    rng = np.random.default_rng(11)
    n = 200_000
    u = np.concatenate([np.exp(rng.uniform(np.log(1e-3), np.log(50.0), n - n // 4)), rng.uniform(0.3, 0.5, n // 4)])
    nu = rng.uniform(-5, 5, n)
    a = rng.uniform(0.5, 2.5, n)
    beta = rng.uniform(0.02, 0.98, n)
    tau = rng.uniform(0.0, 0.5, n)
    eta = np.where(rng.random(n) < 0.3, 0.0, rng.uniform(0, 3, n))
    up = rng.random(n) < 0.5
    p32 = np.stack([nu, a, beta, tau, eta, np.ones(n)], 1).astype(np.float32)
    rt32 = (p32[:, 3].astype(np.float64) + u * p32[:, 1].astype(np.float64) ** 2).astype(np.float32)
    y32 = np.where(up, rt32, -rt32).astype(np.float32)
    data = np.stack([y32, (np.sign(y32) + 1) / 2], 1).astype(np.float32)[:, None, :]
    got = engine.wiener_log_likelihood(engine.ALPHA_NOT_SCALED, torch.as_tensor(p32).cuda(), torch.as_tensor(data).cuda(),
                                       per_trial=True)["trial_logp"][:, 0].double().cpu().numpy()
    t32 = (rt32 - p32[:, 3]).astype(np.float32).astype(np.float64)           # the kernel's t = rt - tau, in float32
    p = p32.astype(np.float64)
    ref = W.log_f(t32, up, p[:, 1], p[:, 0], p[:, 2], 1.0, p[:, 4])
    err = np.abs(got - ref)
    inner = np.abs(ref) <= 20
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(ref))
    print(f"pointwise: max |d log f| {err[inner].max():.3g} (p99 {np.percentile(err[inner], 99):.3g}) where |log f| <= 20; "
          f"max rel {np.max(err[~inner] / np.abs(ref[~inner])):.3g} beyond")
    assert err[inner].max() <= 1e-4
    assert np.all(err[~inner] <= 1e-5 * np.abs(ref[~inner]))


def _both_sides(torch, engine, model, params, x):
    """per-trial log f of the rows `params` at decision times x on the upper and the lower boundary: [R, 2, len(x)]"""
    R, M = params.shape[0], x.size
    tau = params[:, 3].astype(np.float64)
    rt = (tau[:, None] + x[None, :])
    if model == engine.BASIC_DDM_DC:
        d = np.concatenate([np.stack([rt, np.ones_like(rt)], -1), np.stack([rt, -np.ones_like(rt)], -1)], 1)
    else:
        d = np.concatenate([np.stack([rt, np.ones_like(rt)], -1), np.stack([-rt, np.zeros_like(rt)], -1)], 1)
    out = engine.wiener_log_likelihood(model, torch.as_tensor(params, dtype=torch.float32).cuda(),
                                       torch.as_tensor(d, dtype=torch.float32).cuda(), per_trial=True, want_sum=False)["trial_logp"]
    # the kernel's t is rt - tau in float32: integrate over that t
    t = (d[..., 0].astype(np.float32).__abs__() - params[:, 3:4].astype(np.float32)).astype(np.float64)
    return out.double().cpu().numpy().reshape(R, 2, M), t.reshape(R, 2, M)


def test_device_density_normalises():
    torch = _torch()
    from bayesflow_nddms_amd import engine
    rng = np.random.default_rng(5)
    basic = np.stack([rng.uniform(-3, 3, 12), rng.uniform(0.6, 2.0, 12), rng.uniform(0.2, 0.8, 12), rng.uniform(0.1, 0.5, 12),
                      rng.uniform(0.8, 1.3, 12)], 1)
    ans = np.stack([rng.uniform(-3, 3, 12), rng.uniform(0.6, 1.6, 12), rng.uniform(0.2, 0.8, 12), rng.uniform(0.1, 0.5, 12),
                    np.r_[np.zeros(6), rng.uniform(0.3, 2.0, 6)], rng.uniform(0.9, 1.3, 12)], 1)
    x, wts = _simpson_log_grid(1e-5, 60.0, 30001)
    for model, P in ((engine.BASIC_DDM_DC, basic), (engine.ALPHA_NOT_SCALED, ans)):
        lf, t = _both_sides(torch, engine, model, P.astype(np.float32), x)
        # Simpson in log t on the float32 nodes the kernel saw: the weights of the float64 grid times dt/dx ~ 1
        mass = np.sum(np.exp(lf) * wts[None, None, :] * (t / x[None, None, :]), axis=-1)
        for i in range(P.shape[0]):
            assert abs(mass[i].sum() - 1.0) < 2e-5, (model, i, mass[i])
            eta0 = model == engine.BASIC_DDM_DC or P[i, 4] == 0
            if eta0:
                p32 = P[i].astype(np.float32).astype(np.float64)
                s = p32[4] if model == engine.BASIC_DDM_DC else p32[5]
                assert abs(mass[i, 0] - W.p_upper(p32[1], p32[0], p32[2], s)) < 2e-5, (model, i)


def test_density_matches_the_exact_sampler():
    torch = _torch()
    from bayesflow_nddms_amd import engine
    g = np.load(os.path.join(GOLDEN, "ratcliff.npz"))
    sets = g["sets"].astype(np.float32)                                      # Nu, Alpha, Beta, Tau, Eta, Varsigma
    n = 200_000
    sim = engine.simulratcliff(sets, n, seed=77, set_offset=0, fast=False, want_summary=False)["trials"][..., 0].double().cpu().numpy()
    x, wts = _simpson_log_grid(1e-6, 80.0, 40001)
    lf, t = _both_sides(torch, engine, engine.ALPHA_NOT_SCALED, sets, x)
    for i in range(sets.shape[0]):
        f = np.exp(lf[i]) * (t[i] / x)[...] * wts                           # mass of each node
        cu, cl = np.cumsum(f[0]), np.cumsum(f[1])
        p_lo = cl[-1]
        y = np.sort(sim[i])
        tau = float(sets[i, 3])
        F = np.where(y < 0, p_lo - np.interp(-y - tau, x, cl, left=0.0, right=p_lo), p_lo + np.interp(y - tau, x, cu, left=0.0, right=cu[-1]))
        ecdf_hi = np.arange(1, n + 1) / n
        ks = max(np.max(np.abs(ecdf_hi - F)), np.max(np.abs(ecdf_hi - 1.0 / n - F)))
        print(f"set {i}: KS {ks:.4f}, mass {cu[-1] + p_lo:.6f}")
        assert ks < 0.005, (i, ks)


def test_timeouts_are_right_censored():
    torch = _torch()
    from bayesflow_nddms_amd import engine
    P = np.array([[0.0, 3.0, 0.5, 0.3, 0.5], [0.3, 2.5, 0.4, 0.2, 0.6], [-0.2, 3.5, 0.6, 0.4, 0.7]], np.float32)
    sim = engine.simulate(engine.BASIC_DDM_DC, P, 2000, dt=0.01, max_steps=400, seed=3, set_offset=0, want_summary=False)["trials"]
    lp = engine.wiener_log_likelihood(engine.BASIC_DDM_DC, torch.as_tensor(P).cuda(), sim, per_trial=True)["trial_logp"].double().cpu().numpy()
    d = sim.cpu().numpy()
    n_cens = 0
    for i in range(P.shape[0]):
        cens = d[i, :, 1] == 0
        n_cens += cens.sum()
        t = (d[i, cens, 0] - P[i, 3]).astype(np.float32).astype(np.float64)
        p = P[i].astype(np.float64)
        ref = np.array([W.log_survival(tt, p[1], p[0], p[2], p[4]) for tt in t])
        assert np.all(np.abs(lp[i, cens] - ref) <= 2e-5 + 1e-5 * np.abs(ref)), i
        assert np.all(np.isfinite(lp[i]))
    assert n_cens > 500


def _rows(n, rng):
    return np.stack([rng.uniform(-2, 2, n), rng.uniform(0.6, 1.8, n), rng.uniform(0.2, 0.8, n), rng.uniform(0.1, 0.3, n),
                     rng.uniform(0, 1.5, n), rng.uniform(0.8, 1.2, n)], 1).astype(np.float32)


def test_layout_launch_stream_and_capture_give_the_same_bits():
    torch = _torch()
    from bayesflow_nddms_amd import engine
    rng = np.random.default_rng(9)
    D, S, N = 6, 40, 2500                                                    # N > one LDS tile
    p = torch.as_tensor(_rows(D * S, rng)).cuda()
    sim = engine.simulratcliff(_rows(D, rng), N, seed=1, set_offset=0, want_summary=False)["trials"]
    wl = lambda s, d: engine.wiener_log_likelihood(engine.ALPHA_NOT_SCALED, p, d, draws_per_dataset=s, per_trial=True)
    ref = wl(S, sim)
    for s in (20, 8, 4, 1):                                                  # staged (>= 16 draws per data set) and direct layouts
        r = wl(s, sim.repeat_interleave(S // s, 0))
        assert torch.equal(r["loglik"], ref["loglik"]) and torch.equal(r["trial_logp"], ref["trial_logp"]), s
    for _ in range(3):
        r = wl(S, sim)
        assert torch.equal(r["loglik"], ref["loglik"]) and torch.equal(r["trial_logp"], ref["trial_logp"])
    # the row sum is the float64 sum of the per-trial values (in its own fixed order)
    f64 = ref["trial_logp"].double().sum(1)
    assert torch.allclose(ref["loglik"], f64, rtol=1e-12, atol=0)
    # two threads, two streams
    res = [None, None]

    def run(k):
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            res[k] = wl(S, sim)
        st.synchronize()
    th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    for r in res:
        assert torch.equal(r["loglik"], ref["loglik"]) and torch.equal(r["trial_logp"], ref["trial_logp"])
    # captured under a graph arena, replayed twice
    torch.cuda.synchronize()
    with engine.graph_memory():
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side), torch.cuda.graph(g, stream=side):
            out = wl(S, sim)
        torch.cuda.synchronize()
        for _ in range(2):
            out["loglik"].fill_(0.0)
            out["trial_logp"].fill_(0.0)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out["loglik"], ref["loglik"]) and torch.equal(out["trial_logp"], ref["trial_logp"])
        del g
        torch.cuda.synchronize()


def test_edge_rows():
    torch = _torch()
    from bayesflow_nddms_amd import engine
    from bayesflow_nddms_amd.likelihood import diffusion_lpdf, dwiener_logpdf
    rng = np.random.default_rng(4)
    P = np.tile(np.array([[1.0, 1.2, 0.5, 0.3, 1.0]], np.float32), (8, 1))
    P[:, 0] = rng.uniform(-1, 1, 8)
    data = torch.as_tensor(np.stack([rng.uniform(0.4, 2.0, (8, 50)), rng.choice([-1.0, 1.0], (8, 50))], -1), dtype=torch.float32).cuda()
    good = engine.wiener_log_likelihood(engine.BASIC_DDM_DC, torch.as_tensor(P).cuda(), data, per_trial=True)
    bad = P.copy()
    bad[1, 0] = np.nan; bad[3, 1] = 0.0; bad[5, 2] = 1.0; bad[6, 4] = -1.0
    r = engine.wiener_log_likelihood(engine.BASIC_DDM_DC, torch.as_tensor(bad).cuda(), data, per_trial=True)
    for i in range(8):
        if i in (1, 3, 5, 6):
            assert torch.isnan(r["loglik"][i]) and torch.isnan(r["trial_logp"][i]).all(), i
        else:
            assert torch.equal(r["loglik"][i], good["loglik"][i]) and torch.equal(r["trial_logp"][i], good["trial_logp"][i]), i
    # rt <= tau: -inf
    d2 = data.clone()
    d2[0, 0, 0] = 0.3
    d2[0, 1, 0] = 0.1
    r2 = engine.wiener_log_likelihood(engine.BASIC_DDM_DC, torch.as_tensor(P).cuda(), d2, per_trial=True)
    assert r2["trial_logp"][0, 0] == -float("inf") and r2["trial_logp"][0, 1] == -float("inf") and r2["loglik"][0] == -float("inf")
    # alpha_not_scaled: y == 0 is NaN; |Nu| > 5 scores as clipped
    pa = torch.tensor([[7.0, 1.0, 0.5, 0.2, 0.5, 1.0], [5.0, 1.0, 0.5, 0.2, 0.5, 1.0], [-9.0, 1.0, 0.5, 0.2, 0.5, 1.0],
                       [-5.0, 1.0, 0.5, 0.2, 0.5, 1.0]]).cuda()
    y = torch.tensor([[0.5, -0.7, 0.0, 1.1]]).cuda()
    d3 = torch.stack([y, (torch.sign(y) + 1) / 2], -1)
    r3 = engine.wiener_log_likelihood(engine.ALPHA_NOT_SCALED, pa, d3, draws_per_dataset=4, per_trial=True)["trial_logp"]
    assert torch.isnan(r3[:, 2]).all()
    keep = [0, 1, 3]
    assert torch.equal(r3[0, keep], r3[1, keep]) and torch.equal(r3[2, keep], r3[3, keep])
    # Stan's substitution: |Y| < ter -> wiener_lpdf(ter + 0.0001) at the upper boundary
    Y = torch.tensor([0.1, -0.2, 0.6, -0.9]).cuda()
    fl = diffusion_lpdf(Y, 1.3, 0.35, 0.45, 0.8, 1.1, stan_floor=True)
    plain = diffusion_lpdf(Y, 1.3, 0.35, 0.45, 0.8, 1.1)
    at = diffusion_lpdf(torch.tensor([0.35]).cuda() + torch.tensor(0.0001).cuda(), 1.3, 0.35, 0.45, 0.8, 1.1)
    assert torch.equal(fl[:2], at.expand(2)) and torch.equal(fl[2:], plain[2:])
    assert (plain[:2] == -float("inf")).all()
    # JAGS dwiener(alpha, tau, beta, delta) = Stan diffusion_lpdf with dc = 1; broadcasting
    j = dwiener_logpdf(Y[2:], 1.3, 0.35, 0.45, 0.8)
    assert torch.equal(j, diffusion_lpdf(Y[2:], 1.3, 0.35, 0.45, 0.8, 1.0))
    grid = dwiener_logpdf(torch.tensor([[0.6], [-0.9]]).cuda(), torch.tensor([1.0, 1.5, 2.0]).cuda(), 0.3, 0.5, 1.0)
    assert grid.shape == (2, 3)
    ref = W.log_f(np.float64(np.float32(0.6) - np.float32(0.3)), True, np.float32(1.5), 1.0, 0.5)
    assert abs(float(grid[0, 1]) - float(ref)) < 1e-5


def test_recovery_scan():
    torch = _torch()
    from bayesflow_nddms_amd import engine
    th0 = np.array([1.0, 1.2, 0.45, 0.35, 0.5, 1.0], np.float32)
    y = engine.simulratcliff(th0[None], 20_000, seed=21, set_offset=0, want_summary=False)["trials"]
    half = np.array([0.3, 0.08, 0.04, 0.004, 0.4, 0.08])
    rows = []
    for j in range(6):
        g = np.tile(th0, (201, 1)).astype(np.float64)
        g[:, j] = th0[j] + np.linspace(-half[j], half[j], 201)
        rows.append(g)
    P = torch.as_tensor(np.concatenate(rows), dtype=torch.float32).cuda()
    ll = engine.wiener_log_likelihood(engine.ALPHA_NOT_SCALED, P, y, draws_per_dataset=P.shape[0])["loglik"].cpu().numpy().reshape(6, 201)
    for j in range(6):
        x = np.concatenate(rows)[j * 201:(j + 1) * 201, j]
        x = x.astype(np.float32).astype(np.float64)
        i = int(np.argmax(ll[j]))
        assert 0 < i < 200, (j, i)
        h = x[i + 1] - x[i]
        curv = -(ll[j, i + 1] - 2 * ll[j, i] + ll[j, i - 1]) / h ** 2
        se = 1.0 / np.sqrt(curv)
        print(f"param {j}: argmax {x[i]:.4f} (truth {th0[j]:.4f}), SE {se:.4f}")
        assert abs(x[i] - th0[j]) <= 4 * se + h, (j, x[i], th0[j], se)


def test_posterior_helper_is_the_engine_call():
    torch = _torch()
    from bayesflow_nddms_amd import basic_ddm_dc, diagnostics, engine
    rng = np.random.default_rng(8)
    D, S, N = 3, 50, 120
    th = np.stack([rng.uniform(-1, 1, D), rng.uniform(0.8, 1.5, D), rng.uniform(0.4, 0.6, D), rng.uniform(0.2, 0.4, D),
                   rng.uniform(0.8, 1.2, D)], 1).astype(np.float32)
    sim = engine.simulate(engine.BASIC_DDM_DC, th, N, dt=0.001, max_steps=4000, seed=2, set_offset=0, want_summary=False)["trials"]
    samples = (th[:, None, :] + rng.normal(0, 0.02, (D, S, 5))).astype(np.float32)
    sd = torch.as_tensor(samples).cuda()
    got = diagnostics.posterior_log_likelihood(sd, sim, engine.BASIC_DDM_DC)
    want = engine.wiener_log_likelihood(engine.BASIC_DDM_DC, sd.reshape(D * S, 5), sim, draws_per_dataset=S)["loglik"].reshape(D, S)
    assert got.shape == (D, S) and torch.equal(got, want)
    assert torch.equal(basic_ddm_dc.log_likelihood(sd.reshape(D * S, 5), sim), want.reshape(-1))
    one = diagnostics.posterior_log_likelihood(samples[1], sim[1].cpu().numpy(), engine.BASIC_DDM_DC)
    assert torch.equal(one, want[1])
