"""GPU tests of the Wiener first-passage quantile function (include/nddm.h: nddm_wiener_quantile; csrc/nddm_wiener_quantile.h): the
solver's residual against the shipped distribution function and against the float64 yardstick (tests/wiener_cdf_ref.py), the
non-decision time, the reference sampler's tables, layout / launch / stream / capture independence of the bits, the special values
and the Python surface."""
import os

import numpy as np
import pytest

import wiener_cdf_ref as C
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _bits_equal(a, b):
    """torch.equal on the bit patterns: NaN and +inf results count as equal to themselves."""
    torch = _torch()
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _data(model, rt, up):
    """[n, m] response times and boundaries (True: upper) in the model's trial format, float32 [n, m, 2]."""
    from bayesflow_nddms_amd import engine
    rt, up = np.asarray(rt, np.float32), np.asarray(up, bool)
    if model == engine.BASIC_DDM_DC:
        return np.stack([rt, np.where(up, 1.0, -1.0).astype(np.float32)], -1)
    y = np.where(up, rt, -rt).astype(np.float32)
    return np.stack([y, ((np.sign(y) + 1) / 2).astype(np.float32)], -1)


def _cdf_and_limit(model, p32, q, up):
    """The shipped distribution function at the times q [n] on the boundaries `up`, and its limit there, P(boundary) as the device has
    it (the value at rt = inf), float64 [n] each.  Rows with tau = 0, so that rt - tau is q exactly."""
    torch = _torch()
    from bayesflow_nddms_amd import engine
    rt = np.stack([np.where(np.isfinite(q), q, 1.0), np.full(q.shape, np.inf)], 1)
    d = _data(model, rt, np.stack([up, up], 1))
    r = engine.wiener_cdf(model, torch.as_tensor(p32).cuda(), torch.as_tensor(d).cuda(), want_p_upper=False)["cdf"].double().cpu().numpy()
    return r[:, 0], r[:, 1]


@pytest.mark.parametrize("basic,n", [(False, 20_000), (True, 2_000)])
def test_residual_against_the_shipped_distribution_function_and_the_float64_yardstick(basic, n):
    """The rows of the distribution function's accuracy test with tau = 0 (rt == t exactly: with tau = 0.5 the float32 rounding of tau + t
    alone moves F by up to 2.1e-5 on these rows), conditional p ~ U(0.001, 0.999) on the row's drawn boundary, rows with float64
    P(boundary) >= 0.01 kept (at least 80 % of them).  With q the returned time:
      (i)   the shipped wiener_cdf at q is within 2e-5 of the device's target p P_device (the solver's residual);
      (ii)  the float64 yardstick at q is within 6e-5 of p P_float64 (three 2e-5 bars: F at q, the residual, P);
      (iii) in defective mode, with the float32 target of (ii), the yardstick at q is within 4e-5 of it."""
    torch = _torch()
    from bayesflow_nddms_amd import engine
    model = engine.BASIC_DDM_DC if basic else engine.ALPHA_NOT_SCALED
    p32, _, up, _ = C.accuracy_rows(n, basic)
    p32 = p32.copy()
    p32[:, 3] = 0.0
    a, v, beta, _, s, eta = C.row_columns(p32, basic)
    pu = C.p_upper(a, v, beta, s, eta)
    P64 = np.where(up, pu, 1.0 - pu)
    keep = P64 >= 0.01
    print(f"{'basic_ddm_dc' if basic else 'alpha_not_scaled'}: {keep.mean():.3f} of {n} rows have P(boundary) >= 0.01")
    assert keep.mean() >= 0.80
    pc = np.random.default_rng(21).uniform(0.001, 0.999, n).astype(np.float32)
    code = np.where(up, 1.0, -1.0).astype(np.float32)
    pd = torch.as_tensor(p32).cuda()
    req = torch.as_tensor(np.stack([pc, code], 1)[:, None, :]).cuda()
    q = engine.wiener_quantile(model, pd, req, conditional=True)["quantile"]
    assert q.dtype == torch.float32 and tuple(q.shape) == (n, 1)
    q = q[:, 0].double().cpu().numpy()
    assert np.all(np.isfinite(q[keep])) and np.all(q[keep] > 0.0)
    Fdev, Pdev = _cdf_and_limit(model, p32, q, up)
    r1 = np.abs(Fdev - pc.astype(np.float64) * Pdev)[keep]
    r2 = np.abs(C.cdf(q, up, a, v, beta, s, eta) - pc.astype(np.float64) * P64)[keep]
    tgt = (pc.astype(np.float64) * P64).astype(np.float32)
    reqd = torch.as_tensor(np.stack([tgt, code], 1)[:, None, :]).cuda()
    qd = engine.wiener_quantile(model, pd, reqd)["quantile"][:, 0].double().cpu().numpy()
    assert np.all(np.isfinite(qd[keep]))
    r3 = np.abs(C.cdf(qd, up, a, v, beta, s, eta) - tgt.astype(np.float64))[keep]
    print(f"  max (i) |wiener_cdf(q) - p P_device| {r1.max():.3g}, (ii) |yardstick(q) - p P_float64| {r2.max():.3g}, "
          f"(iii) defective |yardstick(q) - target| {r3.max():.3g}")
    assert r1.max() <= 2e-5
    assert r2.max() <= 6e-5
    assert r3.max() <= 4e-5


def _rows(n, rng, tau=(0.1, 0.5)):
    return np.stack([rng.uniform(-2, 2, n), rng.uniform(0.6, 1.8, n), rng.uniform(0.2, 0.8, n), rng.uniform(*tau, n),
                     np.where(rng.random(n) < 0.3, 0.0, rng.uniform(0, 1.5, n)), rng.uniform(0.8, 1.2, n)], 1).astype(np.float32)


def _requests(D, n, rng, pmax=1.0):
    """[D, n, 2] requests on both boundaries, every seventh on either (code 0)."""
    code = rng.choice([-1.0, 1.0], (D, n))
    code[:, ::7] = 0.0
    return np.stack([rng.uniform(0.0, pmax, (D, n)), code], -1).astype(np.float32)


def test_non_decision_time_enters_in_the_last_add_alone():
    torch = _torch()
    from bayesflow_nddms_amd import engine
    rng = np.random.default_rng(12)
    p = _rows(35, rng)
    assert p[:, 3].min() > 0.1 and p[:, 3].max() < 0.5
    p0 = p.copy()
    p0[:, 3] = 0.0
    req = torch.as_tensor(_requests(1, 24, rng)).cuda()
    for model, cols in ((engine.ALPHA_NOT_SCALED, slice(None)), (engine.BASIC_DDM_DC, [0, 1, 2, 3, 5])):
        for cond in (False, True):
            a = engine.wiener_quantile(model, torch.as_tensor(p[:, cols]).cuda(), req, draws_per_dataset=35, conditional=cond)["quantile"]
            b = engine.wiener_quantile(model, torch.as_tensor(p0[:, cols]).cuda(), req, draws_per_dataset=35, conditional=cond)["quantile"]
            assert torch.isfinite(b).sum() > 35 * 8
            want = torch.as_tensor(p[:, 3:4]).cuda() + b
            ok = ~torch.isnan(b)                                        # (a NaN has no bits to compare: p beyond P(boundary), defective)
            assert torch.equal(torch.isnan(a), ~ok) and _bits_equal(a[ok], want[ok]), (model, cond)


def test_reference_samplers_tables():
    """The ten sets of tests/golden/ratcliff.npz (4001-point quantile tables of the signed RT from 2e5 reference trials): every level k / 4000,
    k = 40, 80, ..., 3960, not within 0.01 of P(lower), as a defective request on its boundary (the split from wiener_cdf's p_upper); the
    returned signed time lies between yq[k - 20] and yq[k + 20] -- the 0.005 bar of the distribution function's test, in ranks (the float64
    yardstick alone is at most 12 ranks off).  Control: the next set's row is more than 200 ranks off somewhere."""
    torch = _torch()
    from bayesflow_nddms_amd import engine
    g = np.load(os.path.join(GOLDEN, "ratcliff.npz"))
    sets = g["sets"].astype(np.float32)
    B = sets.shape[0]
    ks = np.arange(40, 3961, 40)
    lev = ks / 4000.0

    def signed_quantiles(rows):
        pd = torch.as_tensor(rows).cuda()
        pu = engine.wiener_cdf(engine.ALPHA_NOT_SCALED, pd, torch.zeros((B, 1, 2)).cuda(), want_cdf=False)["p_upper"].double().cpu().numpy()
        plo = 1.0 - pu
        upper = lev[None, :] > plo[:, None]
        p = np.where(upper, lev[None, :] - plo[:, None], plo[:, None] - lev[None, :])
        use = np.abs(lev[None, :] - plo[:, None]) > 0.01
        req = np.stack([np.where(use, p, 0.0), np.where(upper, 1.0, -1.0)], -1).astype(np.float32)
        q = engine.wiener_quantile(engine.ALPHA_NOT_SCALED, pd, torch.as_tensor(req).cuda())["quantile"].double().cpu().numpy()
        return np.where(upper, q, -q), use

    y, use = signed_quantiles(sets)
    yx, usex = signed_quantiles(np.roll(sets, -1, 0))
    for i in range(B):
        yq = g[f"yq_s{i}"].astype(np.float64)
        k, yi = ks[use[i]], y[i][use[i]]
        assert len(k) >= 90 and np.all(np.isfinite(yi)), i
        rank = np.searchsorted(yq, yi)
        kx, yxi = ks[usex[i]], yx[i][usex[i]]
        dx = np.max(np.abs(np.searchsorted(yq, yxi[np.isfinite(yxi)]) - kx[np.isfinite(yxi)]))
        print(f"set {i}: {len(k)} levels, max rank distance {np.max(np.abs(rank - k))}; against the next set's row {dx}")
        assert np.all(yq[k - 20] <= yi) and np.all(yi <= yq[k + 20]), (i, np.max(np.abs(rank - k)))
        assert dx > 200, (i, dx)


@pytest.mark.parametrize("n", [1, 63, 65, 1025])
def test_layout_launch_stream_and_capture_give_the_same_bits(n):
    torch = _torch()
    from bayesflow_nddms_amd import engine
    rng = np.random.default_rng(9 + n)
    R = 35
    pa = torch.as_tensor(_rows(R, rng)).cuda()
    pb = pa[:, [0, 1, 2, 3, 5]].contiguous()
    one = torch.as_tensor(_requests(1, n, rng)).cuda()                                                     # [1, n, 2]
    assert n < 7 or (one[0, ::7, 1] == 0).all()
    for model, p in ((engine.ALPHA_NOT_SCALED, pa), (engine.BASIC_DDM_DC, pb)):
        for cond in (False, True):
            wq = lambda s, d: engine.wiener_quantile(model, p, d, draws_per_dataset=s, conditional=cond)["quantile"]
            ref = wq(35, one)                                                                              # broadcast layout, a ragged last chunk of 3 rows
            assert tuple(ref.shape) == (R, n) and (n == 1 or torch.isfinite(ref).any())
            for s in (5, 1):                                                                               # paired layout, D x S = 7 x 5 and 35 x 1
                assert _bits_equal(wq(s, one.repeat_interleave(R // s, 0)), ref), (model, cond, s)
    wq = lambda: engine.wiener_quantile(engine.ALPHA_NOT_SCALED, pa, one, draws_per_dataset=35, conditional=True)["quantile"]
    ref = wq()
    # a side stream
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        r = wq()
    st.synchronize()
    assert _bits_equal(r, ref)
    # captured (one kernel node), replayed twice
    torch.cuda.synchronize()
    with engine.graph_memory():
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side), torch.cuda.graph(g, stream=side):
            out = wq()
        torch.cuda.synchronize()
        for _ in range(2):
            out.fill_(-1.0)
            g.replay()
            torch.cuda.synchronize()
            assert _bits_equal(out, ref)
        del g
        torch.cuda.synchronize()


def test_special_values():
    torch = _torch()
    from bayesflow_nddms_amd import engine
    nan, inf = float("nan"), float("inf")
    rng = np.random.default_rng(4)
    # the seven kinds of invalid row of the distribution function's test, and an untouched eighth
    P = np.tile(np.array([[1.0, 1.2, 0.5, 0.3, 1.0]], np.float32), (8, 1))
    P[:, 0] = rng.uniform(-1, 1, 8)
    req = torch.as_tensor(np.stack([rng.uniform(0.0, 0.15, (8, 50)), rng.choice([-1.0, 0.0, 1.0], (8, 50))], -1), dtype=torch.float32).cuda()
    for cond in (False, True):
        good = engine.wiener_quantile(engine.BASIC_DDM_DC, torch.as_tensor(P).cuda(), req, conditional=cond)["quantile"]
        assert torch.isfinite(good).all() and (good >= torch.as_tensor(P[:, 3:4]).cuda()).all()
        bad = P.copy()
        bad[0, 3] = -0.1; bad[1, 0] = np.nan; bad[2, 2] = 0.0; bad[3, 1] = 0.0; bad[4, 1] = np.inf; bad[5, 2] = 1.0; bad[6, 4] = -1.0
        r = engine.wiener_quantile(engine.BASIC_DDM_DC, torch.as_tensor(bad).cuda(), req, conditional=cond)["quantile"]
        assert torch.isnan(r[:7]).all() and torch.equal(r[7], good[7])
    # alpha_not_scaled: Eta < 0 is invalid too, its neighbours unaffected; |Nu| > 5 is answered as clipped
    pa = torch.tensor([[1.0, 1.0, 0.5, 0.2, 0.5, 1.0], [1.0, 1.0, 0.5, 0.2, -0.5, 1.0], [1.0, 1.0, 0.5, 0.2, 0.5, 1.0],
                       [7.0, 1.0, 0.5, 0.2, 0.5, 1.0], [5.0, 1.0, 0.5, 0.2, 0.5, 1.0], [-9.0, 1.0, 0.5, 0.2, 0.5, 1.0],
                       [-5.0, 1.0, 0.5, 0.2, 0.5, 1.0]]).cuda()
    ra = engine.wiener_quantile(engine.ALPHA_NOT_SCALED, pa, req[:1, :21].contiguous(), draws_per_dataset=7, conditional=True)["quantile"]
    assert torch.isnan(ra[1]).all() and torch.isfinite(ra[0]).all() and torch.equal(ra[0], ra[2])
    assert torch.equal(ra[3], ra[4]) and torch.equal(ra[5], ra[6]) and torch.isfinite(ra[3:]).all()
    # p NaN, p < 0, a NaN code: NaN; p == 0: tau -- in both modes, on every code
    row = torch.tensor([[0.5, 1.2, 0.45, 0.3, 1.0]]).cuda()
    cases = torch.tensor([[[nan, 1.0], [nan, -1.0], [nan, 0.0], [-0.1, 1.0], [-1e-30, -1.0], [-inf, 0.0], [0.3, nan], [0.0, nan],
                           [0.0, 1.0], [0.0, -1.0], [0.0, 0.0], [0.2, 3.0], [0.2, 1.0], [0.2, -0.5], [0.2, -1.0]]]).cuda()
    for cond in (False, True):
        r = engine.wiener_quantile(engine.BASIC_DDM_DC, row, cases, conditional=cond)["quantile"][0]
        assert torch.isnan(r[:8]).all() and (r[8:11] == row[0, 3]).all(), (cond, r)
        assert torch.isfinite(r[11:]).all() and r[11] == r[12] and r[13] == r[14]                      # the code's sign names the boundary
    # the limits: P(boundary) as the device has it is the distribution function's value at rt = inf
    lim = engine.wiener_cdf(engine.BASIC_DDM_DC, row, torch.tensor([[[inf, 1.0], [inf, -1.0]]]).cuda(), want_p_upper=False)["cdf"][0]
    one = torch.ones(()).cuda()
    for P_b, code in ((lim[0], 1.0), (lim[1], -1.0)):
        c = torch.full((), code).cuda()
        above, below = torch.nextafter(P_b, one), torch.nextafter(P_b, 0 * one)
        d = torch.stack([torch.stack([x, c]) for x in (above, P_b, below, one, 0.5 * P_b)])[None]
        r = engine.wiener_quantile(engine.BASIC_DDM_DC, row, d)["quantile"][0]                           # defective: p > P NaN, p == P +inf
        assert torch.isnan(r[0]) and r[1] == inf and not torch.isnan(r[2]) and r[2] >= row[0, 3] and torch.isnan(r[3]) and torch.isfinite(r[4])
        d = torch.stack([torch.stack([x, c]) for x in (torch.nextafter(one, 2 * one), one, torch.nextafter(one, 0 * one), 2 * one, 0.5 * one)])[None]
        r = engine.wiener_quantile(engine.BASIC_DDM_DC, row, d, conditional=True)["quantile"][0]         # conditional: p > 1 NaN, p == 1 +inf
        assert torch.isnan(r[0]) and r[1] == inf and not torch.isnan(r[2]) and r[2] >= row[0, 3] and torch.isnan(r[3]) and torch.isfinite(r[4])
    # either boundary (code 0): the limit is 1 in both modes
    d = torch.tensor([[[1.0, 0.0], [1.0000001, 0.0], [2.0, 0.0], [0.5, 0.0]]]).cuda()
    for cond in (False, True):
        r = engine.wiener_quantile(engine.BASIC_DDM_DC, row, d, conditional=cond)["quantile"][0]
        assert r[0] == inf and torch.isnan(r[1:3]).all() and torch.isfinite(r[3])
    # a boundary that is never reached in float32 (P(lower) == 0): conditional NaN, defective NaN beyond p == 0
    never = torch.tensor([[40.0, 3.0, 0.5, 0.3, 1.0]]).cuda()
    assert engine.wiener_cdf(engine.BASIC_DDM_DC, never, torch.tensor([[[inf, -1.0]]]).cuda(), want_p_upper=False)["cdf"][0, 0] == 0.0
    d = torch.tensor([[[0.5, -1.0], [1e-30, -1.0], [0.0, -1.0]]]).cuda()
    for cond in (False, True):
        r = engine.wiener_quantile(engine.BASIC_DDM_DC, never, d, conditional=cond)["quantile"][0]
        assert torch.isnan(r[:2]).all() and r[2] == never[0, 3], (cond, r)
    # a target the float32 G does not reach at the bracket's upper end: +inf.  On either boundary G ends at P(lower) + P(upper) as the
    # device has them, which is below 1 on some rows
    pr = torch.as_tensor(_rows(35, rng)).cuda()
    both = torch.cat([torch.full((35, 1, 1), inf).cuda(), torch.ones((35, 1, 1)).cuda()], -1)
    P_up = engine.wiener_cdf(engine.ALPHA_NOT_SCALED, pr, both, want_p_upper=False)["cdf"][:, 0]
    lower = torch.cat([torch.full((35, 1, 1), -inf).cuda(), torch.zeros((35, 1, 1)).cuda()], -1)
    P_lo = engine.wiener_cdf(engine.ALPHA_NOT_SCALED, pr, lower, want_p_upper=False)["cdf"][:, 0]
    end = P_lo + P_up
    short = end < 1.0
    assert short.any() and torch.isfinite(end).all()
    d = torch.stack([torch.nextafter(end, 2 * torch.ones_like(end)), torch.zeros_like(end)], -1)[:, None, :].contiguous()
    r = engine.wiener_quantile(engine.ALPHA_NOT_SCALED, pr, d)["quantile"][:, 0]
    assert (r[short] == inf).all()
    d[:, 0, 0] = torch.nextafter(end, torch.zeros_like(end))
    r = engine.wiener_quantile(engine.ALPHA_NOT_SCALED, pr, d)["quantile"][:, 0]
    assert torch.isfinite(r[short]).all() and (r[short] >= pr[short, 3]).all()


def test_extreme_rows_and_either_boundary():
    """The four extreme rows of the distribution function's test (|Nu| = 5, Eta = 3, beta .02 / .98): conditional p on a grid of 200 values
    in [1e-6, 1 - 1e-6] on both boundaries is finite or +inf and >= tau, and the shipped wiener_cdf of every finite result is within 2e-5
    of its target.  Code 0: pwiener(q) + pwiener(-q) is within 4e-5 of p."""
    torch = _torch()
    from bayesflow_nddms_amd import engine
    from bayesflow_nddms_amd.likelihood import pwiener, qwiener
    pe = torch.tensor([[5.0, 2.5, 0.5, 0.2, 3.0, 0.8], [5.0, 2.5, 0.98, 0.2, 3.0, 0.8], [-5.0, 2.5, 0.02, 0.2, 3.0, 0.8],
                       [-5.0, 2.5, 0.98, 0.2, 3.0, 0.8]]).cuda()
    grid = torch.as_tensor(np.concatenate([np.geomspace(1e-6, 0.5, 100), 1.0 - np.geomspace(0.5, 1e-6, 100)]), dtype=torch.float32).cuda()
    m = grid.numel()
    pp = torch.cat([grid, grid])
    code = torch.cat([torch.ones(m), -torch.ones(m)]).cuda()
    q = engine.wiener_quantile(engine.ALPHA_NOT_SCALED, pe, torch.stack([pp, code], -1)[None].contiguous(), draws_per_dataset=4, conditional=True)["quantile"]
    assert not torch.isnan(q).any() and (q >= 0.2).all()
    fin = torch.isfinite(q)
    y = torch.where(fin, q, torch.ones_like(q)) * code
    F = engine.wiener_cdf(engine.ALPHA_NOT_SCALED, pe.repeat_interleave(2 * m, 0), torch.stack([y, (torch.sign(y) + 1) / 2], -1).reshape(-1, 1, 2).contiguous(),
                          want_p_upper=False)["cdf"].reshape(4, 2 * m)
    yi = torch.full((1, 2), float("inf")).cuda() * torch.tensor([1.0, -1.0]).cuda()
    lim = engine.wiener_cdf(engine.ALPHA_NOT_SCALED, pe, torch.stack([yi, (torch.sign(yi) + 1) / 2], -1), draws_per_dataset=4, want_p_upper=False)["cdf"]
    target = pp[None, :].double() * torch.cat([lim[:, :1].expand(4, m), lim[:, 1:].expand(4, m)], 1).double()
    res = (F.double() - target).abs()[fin]
    print(f"extreme rows: {int(fin.sum())} finite of {fin.numel()}, max |wiener_cdf(q) - target| {float(res.max()):.3g}")
    assert res.max() <= 2e-5
    # either boundary, through the RWiener surface
    p = torch.tensor([0.01, 0.2, 0.5, 0.8, 0.99]).cuda()
    for alpha, tau, beta, delta in ((1.0, 0.3, 0.5, 0.0), (1.7, 0.25, 0.3, 1.2), (0.8, 0.5, 0.7, -2.5)):
        qq = qwiener(p, alpha, tau, beta, delta, resp="both")
        tot = pwiener(qq, alpha, tau, beta, delta) + pwiener(-qq, alpha, tau, beta, delta)
        assert torch.isfinite(qq).all() and (tot - p).abs().max() <= 4e-5, (alpha, beta, delta, tot)


def test_python_surface():
    torch = _torch()
    from bayesflow_nddms_amd import alpha_not_scaled, basic_ddm_dc, engine
    from bayesflow_nddms_amd.likelihood import pwiener, qwiener, wiener_rt_quantiles
    # qwiener broadcasts as pwiener does
    p = torch.tensor([[0.1], [0.2]]).cuda()
    al = torch.tensor([1.0, 1.5, 2.0]).cuda()
    for resp, sgn in (("upper", 1.0), ("lower", -1.0)):
        q = qwiener(p, al, 0.3, 0.5, 0.5, resp=resp)
        ref = pwiener(sgn * q, al, 0.3, 0.5, 0.5)
        assert q.shape == ref.shape == (2, 3) and q.dtype == ref.dtype == torch.float32 and q.is_cuda and q.device == ref.device
        assert torch.isfinite(q).all() and (q > 0.3).all()
        assert (ref - p).abs().max() <= 2e-5, (resp, ref)
    assert qwiener(0.2, 1.2, 0.3, 0.4, 0.5).shape == () and qwiener(np.array([0.2, 0.1]), 1.2, 0.3, 0.4, 0.5, resp="lower").shape == (2,)
    ps = torch.tensor([0.05, 0.1, 0.2, 0.3]).cuda()
    assert torch.equal(qwiener(ps, 1.2, 0.3, 0.4, 0.5), qwiener(ps, torch.full((4,), 1.2).cuda(), 0.3, 0.4, 0.5))
    # beyond P(boundary) there is no such time
    assert torch.isnan(qwiener(0.9, 1.0, 0.3, 0.5, 0.5, resp="lower")) and torch.isfinite(qwiener(0.9, 1.0, 0.3, 0.5, 0.5, resp="both"))
    # wiener_rt_quantiles: [..., 2, Q], non-decreasing along Q, the engine call
    probs = (.1, .3, .5, .7, .9)
    al = np.array([0.8, 1.0, 1.5, 2.2]); be = np.array([0.3, 0.5, 0.6, 0.45]); de = np.array([-2.0, 0.0, 1.0, 3.0]); vs = np.array([1.0, 0.9, 1.2, 1.3])
    ta = np.array([[0.2], [0.35]])
    got = wiener_rt_quantiles(probs, al, ta, be, de, 0.7, vs)
    assert got.shape == (2, 4, 2, 5) and got.dtype == torch.float32 and got.is_cuda and torch.isfinite(got).all()
    assert (got[..., 1:] >= got[..., :-1]).all() and (got >= torch.as_tensor(ta, dtype=torch.float32).cuda()[:, :, None, None]).all()
    rows = np.stack([np.broadcast_to(x, (2, 4)) for x in (de, al, be, ta, np.float64(0.7), vs)], -1).reshape(8, 6)
    req = np.stack([np.r_[probs, probs], np.r_[-np.ones(5), np.ones(5)]], -1)[None]
    want = engine.wiener_quantile(engine.ALPHA_NOT_SCALED, rows, req, draws_per_dataset=8, conditional=True)["quantile"]
    assert torch.equal(got.reshape(8, 10), want)
    assert wiener_rt_quantiles(probs, 1.2, 0.3, 0.4, 0.5).shape == (2, 5)
    # no clipping of the drift: |delta| > 5 equals the basic model's (unclipped) answer, and differs from delta = 5
    big = wiener_rt_quantiles(probs, 1.0, 0.3, 0.5, 7.0)
    unclipped = basic_ddm_dc.quantile(np.array([7.0, 1.0, 0.5, 0.3, 1.0]), probs)[0]
    assert torch.allclose(big[1], unclipped[1], rtol=1e-4, atol=0) and not torch.allclose(big[1], wiener_rt_quantiles(probs, 1.0, 0.3, 0.5, 5.0)[1], rtol=1e-2)
    # the per-model helpers are the engine call
    rng = np.random.default_rng(8)
    R = 40
    th = np.stack([rng.uniform(-1, 1, R), rng.uniform(0.8, 1.5, R), rng.uniform(0.4, 0.6, R), rng.uniform(0.2, 0.4, R), rng.uniform(0.8, 1.2, R)], 1).astype(np.float32)
    pd = torch.as_tensor(th).cuda()
    qb = basic_ddm_dc.quantile(pd, probs)
    assert tuple(qb.shape) == (R, 2, 5) and torch.equal(qb.reshape(R, 10), engine.wiener_quantile(engine.BASIC_DDM_DC, pd, req, draws_per_dataset=R, conditional=True)["quantile"])
    assert torch.equal(basic_ddm_dc.quantile(th, probs), qb) and torch.equal(basic_ddm_dc.quantile(th[0])[0], qb[0])
    pa = torch.cat([pd[:, :4], torch.full((R, 1), 0.7).cuda(), pd[:, 4:]], 1).contiguous()
    qa = alpha_not_scaled.quantile(pa, probs)
    assert tuple(qa.shape) == (R, 2, 5) and torch.equal(qa.reshape(R, 10), engine.wiener_quantile(engine.ALPHA_NOT_SCALED, pa, req, draws_per_dataset=R, conditional=True)["quantile"])
    assert (qa[..., 1:] >= qa[..., :-1]).all()


def test_quantile_probability_on_the_exact_sampler():
    """4 sets x 20 000 trials of engine.simulratcliff.  The predicted quantile q_pred[b, side, j] is located in the sorted observed response
    times of its boundary: of the n observed there, m are <= q_pred, and m / n is within 0.005 N / n of probs[j], N = 20 000 the set's
    trial count -- the 0.005 KS bar of the distribution function's test on the exact sampler, restated for the conditional level."""
    torch = _torch()
    from bayesflow_nddms_amd import diagnostics, engine
    probs = (.1, .3, .5, .7, .9)
    P = np.array([[0.3, 1.2, 0.5, 0.3, 0.5, 1.0], [-0.2, 1.5, 0.5, 0.2, 0.0, 1.1], [0.1, 0.9, 0.55, 0.4, 1.0, 0.9], [-0.4, 1.1, 0.55, 0.25, 0.3, 1.0]], np.float32)
    N = 20_000
    sim = engine.simulratcliff(P, N, seed=QP_SEED, set_offset=0, fast=False, want_summary=False)["trials"]
    qp = diagnostics.quantile_probability(sim, torch.as_tensor(P[:, None, :]).cuda(), engine.ALPHA_NOT_SCALED, probs)
    assert tuple(qp["observed"].shape) == (4, 2, 5) and tuple(qp["predicted"].shape) == (4, 1, 2, 5)
    assert tuple(qp["p_upper_observed"].shape) == (4,) and tuple(qp["p_upper_predicted"].shape) == (4, 1)
    assert all(v.is_cuda and v.dtype == torch.float32 for v in qp.values())
    pu = engine.wiener_cdf(engine.ALPHA_NOT_SCALED, torch.as_tensor(P).cuda(), sim, want_cdf=False)["p_upper"]
    assert torch.equal(qp["p_upper_predicted"][:, 0], pu)
    y = sim[..., 0].double().cpu().numpy()
    pred, obs = qp["predicted"][:, 0].double().cpu().numpy(), qp["observed"].double().cpu().numpy()
    for b in range(4):
        n_up = int((y[b] > 0).sum())
        assert abs(float(qp["p_upper_observed"][b]) - n_up / N) <= 1e-6
        for side, rts in ((0, -y[b][y[b] < 0]), (1, y[b][y[b] > 0])):
            n = len(rts)
            assert np.allclose(obs[b, side], np.quantile(rts.astype(np.float32).astype(np.float64), probs), rtol=1e-6, atol=0)
            level = np.array([(rts <= pred[b, side, j]).sum() / n for j in range(5)])
            dev = np.max(np.abs(level - np.array(probs)))
            print(f"set {b} side {side}: n {n}, max |m / n - p| {dev:.4f} (bar {0.005 * N / n:.4f})")
            assert dev <= 0.005 * N / n, (b, side, level)
    # a boundary with fewer than Q responses has no observed quantiles; its neighbour keeps them
    few = sim[:1, :8].clone()
    few[0, :, 0] = torch.tensor([0.5, 0.6, 0.7, 0.8, 0.9, 1.0, -0.7, -0.9]).cuda()
    r = diagnostics.quantile_probability(few, torch.as_tensor(P[:1, None, :]).cuda(), engine.ALPHA_NOT_SCALED, probs)
    assert torch.isnan(r["observed"][0, 0]).all() and torch.isfinite(r["observed"][0, 1]).all() and abs(float(r["p_upper_observed"][0]) - 0.75) < 1e-6


# the seed of the sample above.  The bar is about two standard deviations of the SAMPLE's own noise at this trial count (m / n has
# standard deviation 0.005 at p = 0.5, n = 10 000, against a bar of 0.01), so a sample drawn blindly misses it about every other time
# whatever is tested: of the seeds 1 .. 12, six miss it against the FLOAT64 YARDSTICK's own quantiles (tests/wiener_cdf_ref.py, bisected on
# the host; the samples from the sampler's CPU restatement, oracle.philox_ratcliff, which the device equals bit for bit).  The seed was
# chosen with the code under test out of the loop: it is the first of 1, 2, 3, ... whose sample is within 0.7 of the bar of the
# yardstick's quantiles on all eight boundaries (worst boundary: 0.66 of its bar; seed 1: 1.04).  tests/quantile_probability_seed.py
# repeats the choice without a GPU (its output: profiles/r10_quantile_probability_seed.txt).
QP_SEED = 2
