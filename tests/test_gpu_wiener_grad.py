"""GPU tests of the Wiener log-likelihood's gradient (include/nddm.h: nddm_wiener_log_likelihood_grad; csrc/nddm_wiener_grad.h) and its
autograd binding (likelihood.wiener_loglik): the gradient against the float64 yardstick (tests/wiener_grad_ref.py) at the shapes where the
kernel's paths change, the value's bits against nddm_wiener_log_likelihood, layout independence of the gradient's bits, the priors' rows,
the special values, autograd, a gradient ascent, and capture / replay.  The bar B (wiener_grad_ref.BAR_B, in units of the per-column
condition scale) is the host test's."""
import os
import sys

import numpy as np
import pytest

import wiener_cdf_ref as C
import wiener_grad_ref as G
from conftest import ROOT

pytestmark = pytest.mark.gpu

PAIRED = [(1, 1), (15, 65), (17, 1025), (33, 63)]                      # (R, N): N < 64, a partial last wave / workgroup, two LDS tiles' worth
STAGED = [(2, 16, 1), (3, 17, 1025), (2, 31, 2049)]                    # (D, S, N): a partial last workgroup per data set, three tiles


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _rows(basic, n, rng):
    """Distinct rows; alpha_not_scaled with Eta > 0 and Varsigma != 1.  a' in [0.5, 2.25]: with the trials below u spans [0.01, 7.6]."""
    cols = [rng.uniform(-2, 2, n), rng.uniform(0.6, 1.8, n), rng.uniform(0.2, 0.8, n), rng.uniform(0.1, 0.3, n)]
    cols += [rng.uniform(0.8, 1.2, n)] if basic else [rng.uniform(0.2, 1.5, n), rng.uniform(0.8, 1.2, n)]
    return np.stack(cols, 1).astype(np.float32)


def _trials(basic, D, N, rng):
    """[D, N, 2] in the model's format, every rt above every row's tau."""
    rt = rng.uniform(0.35, 2.0, (D, N))
    up = rng.random((D, N)) < 0.5
    if basic:
        return np.stack([rt, np.where(up, 1.0, -1.0)], -1).astype(np.float32)
    y = np.where(up, rt, -rt)
    return np.stack([y, (np.sign(y) + 1) / 2], -1).astype(np.float32)


def _yardstick(basic, p32, d32, S):
    """float64 (gradient, scale) of rows p32 against data sets d32 (row r scores set r // S), at the kernel's float32 t = rt - tau."""
    d = np.repeat(d32, S, 0)
    rt32 = np.abs(d[..., 0]) if not basic else d[..., 0]
    up = d[..., 1] > 0 if basic else d[..., 0] > 0
    t = (rt32 - p32[:, 3:4]).astype(np.float32).astype(np.float64)
    return G.row_grad(basic, p32.astype(np.float64), t, up)


def _model(engine, basic):
    return engine.BASIC_DDM_DC if basic else engine.ALPHA_NOT_SCALED


def _check(name, got, ref, scale):
    err = np.abs(got - ref) / scale
    print(f"{name}: max |gradient - yardstick| / scale per column {np.array2string(err.max(0), precision=2)}")
    assert np.all(np.isfinite(got)) and np.all(err <= G.BAR_B), (name, err.max(0))


@pytest.mark.parametrize("basic", [True, False], ids=["basic_ddm_dc", "alpha_not_scaled"])
@pytest.mark.parametrize("shape", PAIRED + STAGED, ids=lambda s: "x".join(str(x) for x in s))
def test_gradient_against_float64_and_the_values_bits(basic, shape):
    torch = _torch()
    from bayesflow_nddms_amd import engine
    rng = np.random.default_rng(sum(shape) + basic)
    (D, S, N) = shape if len(shape) == 3 else (shape[0], 1, shape[1])
    p32, d32 = _rows(basic, D * S, rng), _trials(basic, D, N, rng)
    p, d = torch.as_tensor(p32).cuda(), torch.as_tensor(d32).cuda()
    r = engine.wiener_log_likelihood_grad(_model(engine, basic), p, d, draws_per_dataset=S)
    assert r["loglik"].shape == (D * S,) and r["grad"].shape == (D * S, p32.shape[1]) and r["grad"].dtype == torch.float64
    ref, scale = _yardstick(basic, p32, d32, S)
    _check(f"{shape}", r["grad"].cpu().numpy(), ref, scale)
    # the value: bit for bit the forward kernel's sum
    fwd = engine.wiener_log_likelihood(_model(engine, basic), p, d, draws_per_dataset=S)["loglik"]
    assert torch.equal(r["loglik"], fwd) and torch.isfinite(fwd).all()


@pytest.mark.parametrize("basic", [True, False], ids=["basic_ddm_dc", "alpha_not_scaled"])
def test_gradient_bits_do_not_depend_on_the_layout(basic):
    torch = _torch()
    from bayesflow_nddms_amd import engine
    rng = np.random.default_rng(9)
    D, S, N = 2, 32, 1100                                                # N > one LDS tile
    p = torch.as_tensor(_rows(basic, D * S, rng)).cuda()
    d = torch.as_tensor(_trials(basic, D, N, rng)).cuda()
    wl = lambda s, data: engine.wiener_log_likelihood_grad(_model(engine, basic), p, data, draws_per_dataset=s)
    ref = wl(S, d)                                                       # broadcast layout, 2 x 32
    assert torch.isfinite(ref["grad"]).all()
    for s in (16, 8, 4, 1):                                              # broadcast 4 x 16; paired 8 x 8, 16 x 4 and 64 x 1 (repeated data sets)
        r = wl(s, d.repeat_interleave(S // s, 0))
        assert torch.equal(r["grad"], ref["grad"]) and torch.equal(r["loglik"], ref["loglik"]), s
    # the same row repeated 16 times on one data set (broadcast) against the row alone (paired)
    one = engine.wiener_log_likelihood_grad(_model(engine, basic), p[:3], d[:1].repeat_interleave(3, 0))
    rep = engine.wiener_log_likelihood_grad(_model(engine, basic), p[:3].repeat_interleave(16, 0), d[:1].repeat_interleave(3, 0), draws_per_dataset=16)
    assert torch.equal(rep["grad"], one["grad"].repeat_interleave(16, 0)) and torch.equal(one["grad"], ref["grad"][:3])


@pytest.mark.parametrize("basic", [True, False], ids=["basic_ddm_dc", "alpha_not_scaled"])
def test_prior_rows_meet_the_bar(basic):
    """The first 2 000 of the host test's 20 000 prior rows of each model, one trial per row with u in [1e-3, 50]."""
    torch = _torch()
    from bayesflow_nddms_amd import engine
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import wiener_host as H                                              # (trial_data)
    n = 2000
    p32, rt32, up, t = (x[:n] for x in C.prior_rows(20_000, basic))
    d32 = H.trial_data(basic, rt32, up)[:, None, :]
    r = engine.wiener_log_likelihood_grad(_model(engine, basic), torch.as_tensor(p32).cuda(), torch.as_tensor(d32).cuda())
    ref, scale = G.row_grad(basic, p32.astype(np.float64), t[:, None], up[:, None])
    assert np.all(np.isfinite(ref)) and np.all(scale > 0)               # no row left out
    _check("prior rows", r["grad"].cpu().numpy(), ref, scale)


def test_special_values_on_the_device():
    torch = _torch()
    from bayesflow_nddms_amd import engine
    rng = np.random.default_rng(4)
    P = _rows(True, 9, rng)
    data = torch.as_tensor(_trials(True, 9, 70, rng)).cuda()
    good = engine.wiener_log_likelihood_grad(engine.BASIC_DDM_DC, torch.as_tensor(P).cuda(), data)
    assert torch.isfinite(good["grad"]).all() and torch.isfinite(good["loglik"]).all()
    # invalid rows between valid ones: NaN there only
    bad = P.copy()
    bad[1, 0] = np.nan; bad[3, 1] = 0.0; bad[5, 2] = 1.0; bad[6, 4] = -1.0
    r = engine.wiener_log_likelihood_grad(engine.BASIC_DDM_DC, torch.as_tensor(bad).cuda(), data)
    for i in range(9):
        if i in (1, 3, 5, 6):
            assert torch.isnan(r["loglik"][i]) and torch.isnan(r["grad"][i]).all(), i
        else:
            assert torch.equal(r["loglik"][i], good["loglik"][i]) and torch.equal(r["grad"][i], good["grad"][i]), i
    # one censored trial (choice 0): the value is the forward kernel's, the gradient NaN in every column; the other rows unchanged
    d2 = data.clone()
    d2[2, 67, 1] = 0.0
    r2 = engine.wiener_log_likelihood_grad(engine.BASIC_DDM_DC, torch.as_tensor(P).cuda(), d2)
    fwd = engine.wiener_log_likelihood(engine.BASIC_DDM_DC, torch.as_tensor(P).cuda(), d2)["loglik"]
    assert torch.equal(r2["loglik"], fwd) and torch.isfinite(fwd[2]) and fwd[2] != good["loglik"][2]
    assert torch.isnan(r2["grad"][2]).all()
    keep = [i for i in range(9) if i != 2]
    assert torch.equal(r2["grad"][keep], good["grad"][keep])
    # rt <= tau: -inf in the value, NaN in every gradient column
    d3 = data.clone()
    d3[4, 5, 0] = 0.05
    r3 = engine.wiener_log_likelihood_grad(engine.BASIC_DDM_DC, torch.as_tensor(P).cuda(), d3)
    assert r3["loglik"][4] == -float("inf") and torch.isnan(r3["grad"][4]).all() and torch.equal(r3["grad"][:4], good["grad"][:4])
    # alpha_not_scaled: |Nu| > 5 has d/dNu == 0 exactly and the other columns of the row at Nu = +-5; y == 0 is NaN in both
    pa = torch.tensor([[7.0, 1.0, 0.5, 0.2, 0.5, 1.3], [5.0, 1.0, 0.5, 0.2, 0.5, 1.3], [-9.0, 1.0, 0.5, 0.2, 0.5, 1.3],
                       [-5.0, 1.0, 0.5, 0.2, 0.5, 1.3]]).cuda()
    y = torch.tensor([[0.5, -0.7, 0.9, 1.1]]).cuda()
    d4 = torch.stack([y, (torch.sign(y) + 1) / 2], -1)
    r4 = engine.wiener_log_likelihood_grad(engine.ALPHA_NOT_SCALED, pa, d4, draws_per_dataset=4)
    g = r4["grad"]
    assert g[0, 0] == 0.0 and g[2, 0] == 0.0 and g[1, 0] != 0.0 and g[3, 0] != 0.0 and torch.isfinite(g).all()
    assert torch.equal(g[0, 1:], g[1, 1:]) and torch.equal(g[2, 1:], g[3, 1:])
    assert r4["loglik"][0] == r4["loglik"][1] and r4["loglik"][2] == r4["loglik"][3]
    d5 = d4.clone()
    d5[0, 2, 0] = 0.0
    r5 = engine.wiener_log_likelihood_grad(engine.ALPHA_NOT_SCALED, pa, d5, draws_per_dataset=4)
    assert torch.isnan(r5["loglik"]).all() and torch.isnan(r5["grad"]).all()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_autograd_is_the_kernels_gradient_in_one_launch(dtype):
    torch = _torch()
    from bayesflow_nddms_amd import alpha_not_scaled, engine, likelihood
    dt = getattr(torch, dtype)
    rng = np.random.default_rng(12)
    D, S, N = 2, 5, 90
    raw = torch.as_tensor(rng.uniform(0.2, 1.2, (D * S, 6)), dtype=dt).cuda().requires_grad_(True)
    scale = torch.tensor([1.0, 1.0, 0.5, 0.2, 1.0, 1.0], dtype=dt).cuda()         # softplus(raw) * scale: beta < 0.73, tau < 0.3 < every rt
    data = torch.as_tensor(_trials(False, D, N, rng)).cuda().requires_grad_(True)
    go = torch.as_tensor(rng.normal(size=D * S)).cuda()
    n0 = engine.wiener_grad_launches()
    params = torch.nn.functional.softplus(raw) * scale
    ll = likelihood.wiener_loglik(engine.ALPHA_NOT_SCALED, params, data, draws_per_dataset=S)
    assert ll.dtype == torch.float64 and ll.shape == (D * S,) and ll.requires_grad
    ll.backward(go)
    assert engine.wiener_grad_launches() == n0 + 1                      # one launch per forward plus backward
    assert data.grad is None and raw.grad is not None and raw.grad.dtype == dt and torch.isfinite(raw.grad).all()
    # the same chain from the engine call
    raw2 = raw.detach().clone().requires_grad_(True)
    params2 = torch.nn.functional.softplus(raw2) * scale
    r = engine.wiener_log_likelihood_grad(engine.ALPHA_NOT_SCALED, params2.detach(), data.detach(), draws_per_dataset=S)
    params2.backward((go[:, None] * r["grad"]).to(dt))
    assert torch.equal(ll.detach(), r["loglik"]) and torch.equal(raw.grad, raw2.grad) and raw.grad.abs().max() > 0
    # nothing requiring grad: the same values, no graph
    plain = likelihood.wiener_loglik(engine.ALPHA_NOT_SCALED, params.detach(), data.detach(), draws_per_dataset=S)
    assert torch.equal(plain, r["loglik"]) and not plain.requires_grad
    # the model adapter is the engine call
    v, g = alpha_not_scaled.log_likelihood_and_grad(params.detach(), data.detach()[..., 0])
    assert torch.equal(v, r["loglik"]) and torch.equal(g, r["grad"])


def test_gradient_ascent_raises_the_log_likelihood():
    torch = _torch()
    from bayesflow_nddms_amd import engine, likelihood
    truth = np.array([1.0, 1.2, 0.45, 0.35, 0.5, 1.0])
    y = engine.simulratcliff(truth[None].astype(np.float32), 2000, seed=21, set_offset=0, want_summary=False)["trials"]
    start = truth * np.array([1.2, 0.8, 1.2, 0.8, 1.2, 0.8])             # every parameter off by 20 % (tau downwards: it stays below every rt)
    theta = torch.as_tensor(start[None]).cuda().requires_grad_(True)
    opt = torch.optim.Adam([theta], lr=0.002)                            # 20 steps move a parameter by 0.04 at the most
    first = None
    for _ in range(20):
        opt.zero_grad()
        ll = likelihood.wiener_loglik(engine.ALPHA_NOT_SCALED, theta, y)
        first = float(ll) if first is None else first
        (-ll.sum()).backward()
        assert torch.isfinite(theta.grad).all()
        opt.step()
    last = float(likelihood.wiener_loglik(engine.ALPHA_NOT_SCALED, theta.detach(), y))
    print(f"log-likelihood {first:.3f} -> {last:.3f} after 20 Adam steps")
    assert np.isfinite(first) and last > first


def test_capture_and_replay_give_the_eager_bits():
    torch = _torch()
    from bayesflow_nddms_amd import engine
    rng = np.random.default_rng(2)
    D, S, N = 3, 20, 300
    p = torch.as_tensor(_rows(False, D * S, rng)).cuda()
    d = torch.as_tensor(_trials(False, D, N, rng)).cuda()
    ref = engine.wiener_log_likelihood_grad(engine.ALPHA_NOT_SCALED, p, d, draws_per_dataset=S)
    torch.cuda.synchronize()
    with engine.graph_memory():
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side), torch.cuda.graph(g, stream=side):
            out = engine.wiener_log_likelihood_grad(engine.ALPHA_NOT_SCALED, p, d, draws_per_dataset=S)
        torch.cuda.synchronize()
        for _ in range(2):
            out["loglik"].fill_(0.0)
            out["grad"].fill_(0.0)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out["loglik"], ref["loglik"]) and torch.equal(out["grad"], ref["grad"])
        del g
        torch.cuda.synchronize()
