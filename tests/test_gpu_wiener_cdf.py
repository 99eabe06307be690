"""GPU tests of the Wiener first-passage distribution function (include/nddm.h: nddm_wiener_cdf; csrc/nddm_wiener_cdf.h): pointwise
accuracy against the float64 yardstick (tests/wiener_cdf_ref.py), consistency with the shipped density, the reference sampler's
tables, the KS distance of the product's exact sampler from the exact law, the timeouts, layout / launch / stream / capture
independence of the bits, the special rows and the Python surface."""
import os

import numpy as np
import pytest

import wiener_cdf_ref as C
import wiener_ref as W
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _simpson_log_grid(x0, x1, n):
    s = np.linspace(np.log(x0), np.log(x1), n)
    h = s[1] - s[0]
    w = np.ones(n)
    w[1:-1:2], w[2:-1:2] = 4.0, 2.0
    x = np.exp(s)
    return x, w * h / 3.0 * x


@pytest.mark.parametrize("basic,n", [(False, 20_000), (True, 2_000)])
def test_pointwise_accuracy_against_the_float64_yardstick(basic, n):
    """|F - yardstick| <= 2e-5 and |p_upper - yardstick| <= 2e-5, at the kernel's float32 t: the bar of the density's integrated mass."""
    torch = _torch()
    from bayesflow_nddms_amd import engine
    p32, rt32, up, t = C.accuracy_rows(n, basic)
    if basic:
        model, data = engine.BASIC_DDM_DC, np.stack([rt32, np.where(up, 1.0, -1.0)], 1)
    else:
        y32 = np.where(up, rt32, -rt32)
        model, data = engine.ALPHA_NOT_SCALED, np.stack([y32, (np.sign(y32) + 1) / 2], 1)
    r = engine.wiener_cdf(model, torch.as_tensor(p32).cuda(), torch.as_tensor(data.astype(np.float32)[:, None, :]).cuda())
    got, gp = r["cdf"][:, 0].double().cpu().numpy(), r["p_upper"].double().cpu().numpy()
    a, v, beta, _, s, eta = C.row_columns(p32, basic)
    ref, pref = C.cdf(t, up, a, v, beta, s, eta), C.p_upper(a, v, beta, s, eta)
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(gp)) and got.min() >= 0.0 and got.max() <= 1.0
    err, perr = np.abs(got - ref), np.abs(gp - pref)
    print(f"pointwise ({'basic_ddm_dc' if basic else 'alpha_not_scaled'}, {n} rows): max |F - ref| {err.max():.3g} (p99 "
          f"{np.percentile(err, 99):.3g}), max |p_upper - ref| {perr.max():.3g}")
    assert err.max() <= 2e-5 and perr.max() <= 2e-5


def test_consistent_with_the_shipped_density():
    """F(t2) - F(t1) is the Simpson mass of the device's own trial_logp on [t1, t2], t1 < u* a'^2 < t2, within
    6e-5: three 2e-5 bars (two values of F and the density's mass)."""
    torch = _torch()
    from bayesflow_nddms_amd import engine
    rng = np.random.default_rng(5)
    n = 12
    P = np.stack([rng.uniform(-3, 3, n), rng.uniform(0.6, 1.6, n), rng.uniform(0.2, 0.8, n), rng.uniform(0.1, 0.5, n),
                  np.r_[np.zeros(n // 2), rng.uniform(0.3, 2.0, n - n // 2)], rng.uniform(0.9, 1.3, n)], 1).astype(np.float32)
    ap2 = (P[:, 1].astype(np.float64) / P[:, 5]) ** 2
    u1, u2 = rng.uniform(0.05, 0.3, n), rng.uniform(0.45, 3.0, n)
    M = 4001
    worst = 0.0
    for up in (False, True):
        sgn = 1.0 if up else -1.0
        rows = []
        for i in range(n):
            x, wts = _simpson_log_grid(u1[i] * ap2[i], u2[i] * ap2[i], M)
            rows.append((x, wts))
        rt = np.stack([P[i, 3].astype(np.float64) + rows[i][0] for i in range(n)]).astype(np.float32)        # [n, M]
        y = torch.as_tensor(sgn * rt).cuda()
        d = torch.stack([y, (torch.sign(y) + 1) / 2], -1)
        pd = torch.as_tensor(P).cuda()
        lf = engine.wiener_log_likelihood(engine.ALPHA_NOT_SCALED, pd, d, per_trial=True, want_sum=False)["trial_logp"].double().cpu().numpy()
        F = engine.wiener_cdf(engine.ALPHA_NOT_SCALED, pd, d[:, [0, M - 1]].contiguous(), want_p_upper=False)["cdf"].double().cpu().numpy()
        t = (rt - P[:, 3:4]).astype(np.float32).astype(np.float64)                                          # the kernel's t
        for i in range(n):
            x, wts = rows[i]
            mass = np.sum(np.exp(lf[i]) * wts * (t[i] / x))
            worst = max(worst, abs((F[i, 1] - F[i, 0]) - mass))
            assert t[i, 0] < 0.375 * ap2[i] < t[i, -1]
            assert abs((F[i, 1] - F[i, 0]) - mass) <= 6e-5, (up, i, F[i], mass)
    print(f"density consistency: max |dF - mass| {worst:.3g}")


def test_reference_samplers_tables():
    """The ten sets of tests/golden/ratcliff.npz against their own quantile tables (the float64 yardstick gives 0.0015 .. 0.0029 and
    |P_up - pupper| <= 0.0019: tests/test_wiener_cdf_host.py); control: the same tables against the next set's row."""
    torch = _torch()
    from bayesflow_nddms_amd import diagnostics, engine
    g = np.load(os.path.join(GOLDEN, "ratcliff.npz"))
    sets = g["sets"].astype(np.float32)
    B = sets.shape[0]
    yq = np.stack([g[f"yq_s{i}"] for i in range(B)]).astype(np.float32)
    tr = torch.as_tensor(np.stack([yq, (np.sign(yq) + 1) / 2], -1)).cuda()
    q = np.arange(4001) / 4000.0
    G = diagnostics.signed_cdf_analytic(tr, torch.as_tensor(sets).cuda(), engine.ALPHA_NOT_SCALED)
    assert G.dtype == torch.float32 and tuple(G.shape) == (B, 4001)
    G = G.double().cpu().numpy()
    pu = engine.wiener_cdf(engine.ALPHA_NOT_SCALED, torch.as_tensor(sets).cuda(), tr, want_cdf=False)["p_upper"].cpu().numpy()
    Gx = diagnostics.signed_cdf_analytic(tr, torch.as_tensor(np.roll(sets, -1, 0)).cuda(), engine.ALPHA_NOT_SCALED).double().cpu().numpy()
    for i in range(B):
        d, dp = np.max(np.abs(G[i] - q)[1:-1]), abs(float(pu[i]) - g[f"pupper_s{i}"][0])
        dx = np.max(np.abs(Gx[i] - q)[1:-1])
        print(f"set {i}: max |G(yq) - q| {d:.4f}, |p_upper - pupper| {dp:.4f}; against the next set's row {dx:.3f}")
        assert d <= 0.005 and dp <= 0.005, (i, d, dp)
        assert dx > 0.05, (i, dx)


def test_ks_analytic_on_the_exact_sampler():
    """The inputs and the bar of test_gpu_wiener.py::test_density_matches_the_exact_sampler, in one call and without a fixture."""
    torch = _torch()
    from bayesflow_nddms_amd import diagnostics, engine
    g = np.load(os.path.join(GOLDEN, "ratcliff.npz"))
    sets = g["sets"].astype(np.float32)
    n = 200_000
    sim = engine.simulratcliff(sets, n, seed=77, set_offset=0, fast=False, want_summary=False)["trials"]
    pd = torch.as_tensor(sets).cuda()
    ks = diagnostics.ks_analytic(sim, pd, engine.ALPHA_NOT_SCALED)
    assert ks.dtype == torch.float64 and ks.is_cuda and tuple(ks.shape) == (sets.shape[0],)
    G = diagnostics.signed_cdf_analytic(sim, pd, engine.ALPHA_NOT_SCALED).double().cpu().numpy()
    y = sim[..., 0].cpu().numpy()
    ks = ks.cpu().numpy()
    i = np.arange(1, n + 1) / n
    for b in range(sets.shape[0]):
        Gs = G[b][np.argsort(y[b], kind="stable")]
        want = max(np.max(np.abs(i - Gs)), np.max(np.abs(i - 1.0 / n - Gs)))
        print(f"set {b}: KS {ks[b]:.4f} (NumPy restatement {want:.6f})")
        assert abs(ks[b] - want) <= 1e-6, (b, ks[b], want)
        assert ks[b] < 0.005, (b, ks[b])
    # a set that holds a timeout has no KS distance; its neighbours keep theirs
    sim2 = sim[:, :5000].clone()
    ref2 = diagnostics.ks_analytic(sim2, pd, engine.ALPHA_NOT_SCALED)
    sim2[3, 17, 0] = 0.0
    sim2[3, 17, 1] = 0.5
    got2 = diagnostics.ks_analytic(sim2, pd, engine.ALPHA_NOT_SCALED)
    keep = [b for b in range(sets.shape[0]) if b != 3]
    assert torch.isnan(got2[3]) and torch.equal(got2[keep], ref2[keep]) and not torch.isnan(ref2).any()


def test_timeouts_give_the_distribution_function_over_both_boundaries():
    """The three rows of test_gpu_wiener.py::test_timeouts_are_right_censored: on choice 0 the value is 1 - S of the float64 survival series."""
    torch = _torch()
    from bayesflow_nddms_amd import engine
    P = np.array([[0.0, 3.0, 0.5, 0.3, 0.5], [0.3, 2.5, 0.4, 0.2, 0.6], [-0.2, 3.5, 0.6, 0.4, 0.7]], np.float32)
    sim = engine.simulate(engine.BASIC_DDM_DC, P, 2000, dt=0.01, max_steps=400, seed=3, set_offset=0, want_summary=False)["trials"]
    F = engine.wiener_cdf(engine.BASIC_DDM_DC, torch.as_tensor(P).cuda(), sim, want_p_upper=False)["cdf"].double().cpu().numpy()
    d = sim.cpu().numpy()
    n_cens, worst = 0, 0.0
    for i in range(P.shape[0]):
        cens = d[i, :, 1] == 0
        n_cens += cens.sum()
        t = (d[i, cens, 0] - P[i, 3]).astype(np.float32).astype(np.float64)
        p = P[i].astype(np.float64)
        ref = np.array([1.0 - np.exp(W.log_survival(tt, p[1], p[0], p[2], p[4])) for tt in t])
        worst = max(worst, np.max(np.abs(F[i, cens] - ref)))
        assert np.all(np.abs(F[i, cens] - ref) <= 2e-5), i
        assert np.all(np.isfinite(F[i])) and F[i].min() >= 0.0 and F[i].max() <= 1.0
    print(f"timeouts: {n_cens} of them, max |cdf - (1 - S)| {worst:.3g}")
    assert n_cens > 500


def _rows(n, rng):
    return np.stack([rng.uniform(-2, 2, n), rng.uniform(0.6, 1.8, n), rng.uniform(0.2, 0.8, n), rng.uniform(0.1, 0.3, n),
                     np.where(rng.random(n) < 0.3, 0.0, rng.uniform(0, 1.5, n)), rng.uniform(0.8, 1.2, n)], 1).astype(np.float32)


@pytest.mark.parametrize("N", [1, 63, 65, 1025])
def test_layout_launch_stream_and_capture_give_the_same_bits(N):
    torch = _torch()
    from bayesflow_nddms_amd import engine
    rng = np.random.default_rng(9 + N)
    R = 35
    p = torch.as_tensor(_rows(R, rng)).cuda()
    one = engine.simulratcliff(_rows(1, rng), N, seed=1, set_offset=0, want_summary=False)["trials"]        # [1, N, 2]
    wc = lambda s, d: engine.wiener_cdf(engine.ALPHA_NOT_SCALED, p, d, draws_per_dataset=s)
    same = lambda r, ref: torch.equal(r["cdf"], ref["cdf"]) and torch.equal(r["p_upper"], ref["p_upper"])
    ref = wc(35, one)                                                                                      # broadcast layout, a ragged last chunk of 3 rows
    assert tuple(ref["cdf"].shape) == (R, N) and not torch.isnan(ref["cdf"]).any()
    for s in (5, 1):                                                                                       # paired layout, D x S = 7 x 5 and 35 x 1
        assert same(wc(s, one.repeat_interleave(R // s, 0)), ref), s
    # P(upper) alone, and the distribution function alone, are the same values
    assert torch.equal(engine.wiener_cdf(engine.ALPHA_NOT_SCALED, p, one, draws_per_dataset=35, want_cdf=False)["p_upper"], ref["p_upper"])
    assert torch.equal(engine.wiener_cdf(engine.ALPHA_NOT_SCALED, p, one, draws_per_dataset=35, want_p_upper=False)["cdf"], ref["cdf"])
    # the basic model on both layouts (its timeouts included: every seventh trial is made one)
    pb = p[:, [0, 1, 2, 3, 5]].contiguous()
    db = torch.stack([one[..., 0].abs(), torch.sign(one[..., 0])], -1)
    db[:, ::7, 1] = 0.0
    rb = engine.wiener_cdf(engine.BASIC_DDM_DC, pb, db, draws_per_dataset=35)
    assert same(engine.wiener_cdf(engine.BASIC_DDM_DC, pb, db.repeat_interleave(7, 0), draws_per_dataset=5), rb)
    # a side stream
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        r = wc(35, one)
    st.synchronize()
    assert same(r, ref)
    # captured (one kernel node), replayed twice
    torch.cuda.synchronize()
    with engine.graph_memory():
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side), torch.cuda.graph(g, stream=side):
            out = wc(35, one)
        torch.cuda.synchronize()
        for _ in range(2):
            out["cdf"].fill_(-1.0)
            out["p_upper"].fill_(-1.0)
            g.replay()
            torch.cuda.synchronize()
            assert same(out, ref)
        del g
        torch.cuda.synchronize()


def test_special_rows():
    torch = _torch()
    from bayesflow_nddms_amd import engine
    rng = np.random.default_rng(4)
    P = np.tile(np.array([[1.0, 1.2, 0.5, 0.3, 1.0]], np.float32), (8, 1))
    P[:, 0] = rng.uniform(-1, 1, 8)
    data = torch.as_tensor(np.stack([rng.uniform(0.4, 2.0, (8, 50)), rng.choice([-1.0, 0.0, 1.0], (8, 50))], -1), dtype=torch.float32).cuda()
    good = engine.wiener_cdf(engine.BASIC_DDM_DC, torch.as_tensor(P).cuda(), data)
    assert not torch.isnan(good["cdf"]).any() and not torch.isnan(good["p_upper"]).any()
    bad = P.copy()
    bad[0, 3] = -0.1; bad[1, 0] = np.nan; bad[2, 2] = 0.0; bad[3, 1] = 0.0; bad[4, 1] = np.inf; bad[5, 2] = 1.0; bad[6, 4] = -1.0
    r = engine.wiener_cdf(engine.BASIC_DDM_DC, torch.as_tensor(bad).cuda(), data)
    for i in range(8):
        if i < 7:
            assert torch.isnan(r["p_upper"][i]) and torch.isnan(r["cdf"][i]).all(), i
        else:
            assert torch.equal(r["p_upper"][i], good["p_upper"][i]) and torch.equal(r["cdf"][i], good["cdf"][i]), i
    # alpha_not_scaled: Eta < 0 is invalid too, its neighbours unaffected
    pa = torch.tensor([[1.0, 1.0, 0.5, 0.2, 0.5, 1.0], [1.0, 1.0, 0.5, 0.2, -0.5, 1.0], [1.0, 1.0, 0.5, 0.2, 0.5, 1.0]]).cuda()
    ya = torch.tensor([[0.5, -0.7, 1.1]]).cuda()
    da = torch.stack([ya, (torch.sign(ya) + 1) / 2], -1)
    ra = engine.wiener_cdf(engine.ALPHA_NOT_SCALED, pa, da, draws_per_dataset=3)
    assert torch.isnan(ra["cdf"][1]).all() and torch.isnan(ra["p_upper"][1])
    assert torch.equal(ra["cdf"][0], ra["cdf"][2]) and not torch.isnan(ra["cdf"][0]).any()
    # rt <= tau: 0, on either boundary and for a timeout
    d2 = data[:1, :6].clone()
    d2[0, :, 0] = torch.tensor([0.3, 0.1, 0.3, 0.1, 0.3, 0.0])
    d2[0, :, 1] = torch.tensor([1.0, 1.0, -1.0, -1.0, 0.0, 0.0])
    r2 = engine.wiener_cdf(engine.BASIC_DDM_DC, torch.as_tensor(P[:1]).cuda(), d2)["cdf"]
    assert (r2 == 0.0).all()
    # alpha_not_scaled: y == 0 is NaN; |Nu| > 5 is scored as clipped
    pc = torch.tensor([[7.0, 1.0, 0.5, 0.2, 0.5, 1.0], [5.0, 1.0, 0.5, 0.2, 0.5, 1.0], [-9.0, 1.0, 0.5, 0.2, 0.5, 1.0],
                       [-5.0, 1.0, 0.5, 0.2, 0.5, 1.0]]).cuda()
    y = torch.tensor([[0.5, -0.7, 0.0, 1.1]]).cuda()
    d3 = torch.stack([y, (torch.sign(y) + 1) / 2], -1)
    r3 = engine.wiener_cdf(engine.ALPHA_NOT_SCALED, pc, d3, draws_per_dataset=4)
    assert torch.isnan(r3["cdf"][:, 2]).all()
    keep = [0, 1, 3]
    assert torch.equal(r3["cdf"][0, keep], r3["cdf"][1, keep]) and torch.equal(r3["cdf"][2, keep], r3["cdf"][3, keep])
    assert torch.equal(r3["p_upper"][0], r3["p_upper"][1]) and torch.equal(r3["p_upper"][2], r3["p_upper"][3])
    # an extreme row: finite and inside [0, 1] at every time, on both boundaries, and monotone to P(boundary)
    pe = torch.tensor([[5.0, 2.5, 0.5, 0.2, 3.0, 0.8], [5.0, 2.5, 0.98, 0.2, 3.0, 0.8], [-5.0, 2.5, 0.02, 0.2, 3.0, 0.8],
                       [-5.0, 2.5, 0.98, 0.2, 3.0, 0.8]]).cuda()
    tt = torch.as_tensor(np.concatenate([[1e-30, 1e-12], np.geomspace(1e-6, 1e6, 1500), [1e12, 1e30, np.inf]]), dtype=torch.float32).cuda()
    ye = torch.cat([0.2 + tt, -(0.2 + tt)])[None]
    re = engine.wiener_cdf(engine.ALPHA_NOT_SCALED, pe, torch.stack([ye, (torch.sign(ye) + 1) / 2], -1), draws_per_dataset=4)
    assert torch.isfinite(re["cdf"]).all() and (re["cdf"] >= 0).all() and (re["cdf"] <= 1).all()
    assert torch.isfinite(re["p_upper"]).all() and (re["p_upper"] >= 0).all() and (re["p_upper"] <= 1).all()
    m = tt.numel()
    # at t = inf the upper boundary's value IS p_upper; the lower one's is P(lower), worked out on its own: two 2e-5 bars apart at most
    assert torch.equal(re["cdf"][:, m - 1], re["p_upper"]) and torch.allclose(re["cdf"][:, 2 * m - 1], 1 - re["p_upper"], rtol=0, atol=4e-5)
    assert (re["cdf"][:, 1:m] >= re["cdf"][:, :m - 1] - 2e-5).all() and (re["cdf"][:, m + 1:] >= re["cdf"][:, m:2 * m - 1] - 2e-5).all()
    a, v, beta, _, s, eta = C.row_columns(pe.cpu().numpy())
    assert np.max(np.abs(re["p_upper"].double().cpu().numpy() - C.p_upper(a, v, beta, s, eta))) <= 2e-5


def test_python_surface():
    torch = _torch()
    from bayesflow_nddms_amd import alpha_not_scaled, basic_ddm_dc, engine
    from bayesflow_nddms_amd.likelihood import dwiener_logpdf, pwiener, wiener_choice_prob
    # pwiener broadcasts as dwiener_logpdf does
    q = torch.tensor([[0.6], [-0.9]]).cuda()
    al = torch.tensor([1.0, 1.5, 2.0]).cuda()
    grid = pwiener(q, al, 0.3, 0.5, 1.0)
    assert grid.shape == dwiener_logpdf(q, al, 0.3, 0.5, 1.0).shape == (2, 3) and grid.dtype == torch.float32 and grid.is_cuda
    ref = C.cdf(np.float64(np.float32(0.6) - np.float32(0.3)), True, np.float32(1.5), 1.0, 0.5)
    assert abs(float(grid[0, 1]) - float(ref)) <= 2e-5
    ref = C.cdf(np.float64(np.float32(0.9) - np.float32(0.3)), False, np.float32(2.0), 1.0, 0.5)
    assert abs(float(grid[1, 2]) - float(ref)) <= 2e-5
    assert pwiener(0.7, 1.2, 0.3, 0.4, 0.5).shape == () and pwiener(np.array([0.7, -0.8]), 1.2, 0.3, 0.4, 0.5).shape == (2,)
    # parameters constant along the last axis (one row, many trials) and one row per element are the same values
    qs = torch.tensor([0.5, -0.6, 0.9, -1.4]).cuda()
    assert torch.equal(pwiener(qs, 1.2, 0.3, 0.4, 0.5), pwiener(qs, torch.full((4,), 1.2).cuda(), 0.3, 0.4, 0.5))
    # the two boundaries' distribution functions add up to 1 in the limit
    for alpha, beta, delta in ((1.0, 0.5, 0.0), (1.7, 0.3, 1.2), (0.8, 0.7, -2.5)):
        tot = float(pwiener(1e3, alpha, 0.3, beta, delta) + pwiener(-1e3, alpha, 0.3, beta, delta))
        assert abs(tot - 1.0) <= 4e-5, (alpha, beta, delta, tot)             # each boundary's limit is within the 2e-5 bar of its probability
    # the choice probability: the closed form at eta = 0, the yardstick with eta, no clipping of the drift
    al = np.array([0.8, 1.0, 1.5, 2.2]); be = np.array([0.3, 0.5, 0.6, 0.45]); de = np.array([-2.0, 0.0, 1.0, 7.0]); vs = np.array([1.0, 0.9, 1.2, 1.3])
    got = wiener_choice_prob(al, be, de, 0.0, vs).double().cpu().numpy()
    want = np.array([W.p_upper(a, v, b, s) for a, v, b, s in zip(al.astype(np.float32), de.astype(np.float32), be.astype(np.float32), vs.astype(np.float32))])
    assert got.shape == (4,) and np.max(np.abs(got - want)) <= 2e-5
    got = wiener_choice_prob(al, be, de, 1.5, vs).double().cpu().numpy()
    assert np.max(np.abs(got - C.p_upper(al, de, be, vs, 1.5))) <= 2e-5
    # the per-model helpers are the engine call
    rng = np.random.default_rng(8)
    D, S, N = 3, 20, 40
    th = np.stack([rng.uniform(-1, 1, D * S), rng.uniform(0.8, 1.5, D * S), rng.uniform(0.4, 0.6, D * S), rng.uniform(0.2, 0.4, D * S),
                   rng.uniform(0.8, 1.2, D * S)], 1).astype(np.float32)
    sim = engine.simulate(engine.BASIC_DDM_DC, th[:D], N, dt=0.01, max_steps=400, seed=2, set_offset=0, want_summary=False)["trials"]
    pd = torch.as_tensor(th).cuda()
    assert torch.equal(basic_ddm_dc.cdf(pd, sim), engine.wiener_cdf(engine.BASIC_DDM_DC, pd, sim, draws_per_dataset=S)["cdf"])
    pa = torch.cat([pd[:, :4], torch.full((D * S, 1), 0.7).cuda(), pd[:, 4:]], 1).contiguous()
    ya = engine.simulratcliff(pa[:D], N, seed=5, set_offset=0, want_summary=False)["trials"]
    assert torch.equal(alpha_not_scaled.cdf(pa, ya[..., 0]), engine.wiener_cdf(engine.ALPHA_NOT_SCALED, pa, ya, draws_per_dataset=S)["cdf"])
    one = alpha_not_scaled.cdf(pa[0].cpu().numpy(), ya[0, :, 0].cpu().numpy())
    assert one.shape == (1, N) and torch.equal(one[0], engine.wiener_cdf(engine.ALPHA_NOT_SCALED, pa[:1], ya[:1])["cdf"][0])
