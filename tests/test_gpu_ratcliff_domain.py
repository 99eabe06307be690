"""nddm_simulratcliff flags the rows it cannot sample (the two rules of csrc/nddm_ratcliff.h), in both modes and through every path a
summary takes; inside the generator's box its law is the first-passage law in float64; and the fast mode's values, summaries and
external datum hold at the shapes where the hand-out, the tiling and the flush can go wrong.  The CPU side of the same checks:
tests/test_ratcliff_domain_host.py."""
import functools

import numpy as np
import pytest

import prior_util
import ratcliff_domain_cases as rc

pytestmark = pytest.mark.gpu

SEED, OFFSET = 2026, (1 << 36) + 11
BOUNDARY_ROWS = np.array([[8.0, 1.0, 0.0, 0.3, 0.0, 1.0], [-9.0, 1.0, 1.0, 0.3, 0.0, 1.0], [0.0, 0.8, 0.5, 0.15, 0.0, 1.4]], np.float32)
SHAPES_N = [1, 63, 300, 513, 1200]


def _mixed_rows():
    """-> (params [106, 6], indices of the invalid rows): invalid rows, ladder rows and boundary rows among 90 rows of the prior."""
    pr = prior_util.alpha_ns_prior(90, 77)
    p = np.concatenate([pr[:30], rc.INVALID_ROWS, pr[30:60], rc.LADDER_ROWS, pr[60:], BOUNDARY_ROWS])
    return p, np.arange(30, 30 + len(rc.INVALID_ROWS))


@functools.lru_cache(maxsize=None)
def _oracle(N):
    import oracle
    return oracle.philox_ratcliff(_mixed_rows()[0], N, seed=SEED, set_offset=OFFSET, ext_sigma=0.1, ext_mode=0, want_ext=True, threads=8)


def _device(p, N, fast, seed=SEED, set_offset=OFFSET, **kw):
    """Through DEVICE tensors (host arrays with an invalid row are refused before any launch) -> dict of numpy arrays."""
    import torch
    from bayesflow_nddms_amd import engine
    r = engine.simulratcliff(torch.as_tensor(np.ascontiguousarray(p, np.float32)).cuda(), N, seed=seed, set_offset=set_offset, fast=fast, **kw)
    return {k: r[k].cpu().numpy() for k in ("trials", "summary", "ext") if k in r}


@pytest.mark.parametrize("N", SHAPES_N)
def test_mixed_batch_exact_mode_equals_the_oracle(N):
    """NaN masks and bits: trials, summaries (one tile, and split sets through combine_partials_kernel) and ext."""
    p, bad = _mixed_rows()
    g, o = _device(p, N, False, ext_sigma=0.1, ext_mode=0, want_ext=True), _oracle(N)
    for k in ("trials", "summary", "ext"):
        assert rc.same_bits(g[k], o[k]), k
    rc.assert_rule_1(g, bad, N)
    rc.assert_missing_is_nan_count(g)


@pytest.mark.parametrize("N", SHAPES_N)
def test_mixed_batch_fast_mode(N):
    p, bad = _mixed_rows()
    f = _device(p, N, True, ext_sigma=0.1, ext_mode=0, want_ext=True)
    rc.assert_rule_1(f, bad, N)
    rc.assert_missing_is_nan_count(f)
    assert np.array_equal(np.isnan(f["ext"]), np.isnan(p[:, 1]))
    # rows without a missing trial: the exact mode's responses and times (the bars of test_simulratcliff_bit_parity)
    e = _device(p, N, False, want_summary=False)["trials"]
    rows = f["summary"][:, 2] == 0
    assert rows.sum() >= 93                                  # the prior rows, the boundary rows and the ladder's first
    fy, ey = f["trials"][rows, :, 0], e[rows, :, 0]
    same = np.sign(fy) == np.sign(ey)
    assert same.mean() > 0.9999 and np.abs(fy - ey)[same].max() < 1e-5
    if N >= 300:                                             # the ladder's last rows lose trials to the cap in this mode too
        assert np.all(f["summary"][70:73, 2] > 0) and f["summary"][68, 2] == 0, f["summary"][68:73, 2]


@pytest.mark.parametrize("fast,seed", [(False, 5), (True, 5), (False, 6), (True, 6)])
def test_corner_law_on_the_device(fast, seed):
    r = _device(rc.CORNER_ROWS, rc.CORNER_N, fast, seed=seed, set_offset=0)
    assert np.all(r["summary"][:, 2] == 0) and not np.any(np.isnan(r["trials"]))       # first: no trial met a cap
    rc.assert_corner_law(r["trials"][..., 0])


def _moments(rt, n):
    """float64 mean and variance over the leading n entries' worth of a masked sum (n > 0)."""
    m = rt.sum() / n
    return m, ((rt - m) ** 2).sum() / n


@pytest.mark.parametrize("B,N", [(1, 1), (3, 2), (130, 7), (67, 100), (37, 300), (5, 513), (3, 1200)])
def test_fast_mode_properties(B, N):
    """(130, 7): more than one group of 64 tiles, the last one partial; (5, 513), (3, 1200): split sets.

    The summary's moments are, by definition (csrc/nddm_ratcliff.h, oracle section D), those of the decision time in units of
    2^-16 s -- Tau + 2^-16 mean(round(2^16 (|y| - Tau))) -- and the float64 recomputation from the trials is of that quantity, at the
    tolerances of test_full_size_properties (whose time unit, dt, is exact).  The plain mean of |y| is printed and held to what the
    unit allows: half a unit, 2^-17 s = 7.6e-6, plus those tolerances."""
    p = prior_util.alpha_ns_prior(B, 400 + B)
    so = 5 * B + 3
    r = _device(p, N, True, set_offset=so, ext_sigma=0.1, ext_mode=0, want_ext=True)
    t, s = r["trials"], r["summary"]
    y, acc = t[..., 0], t[..., 1]
    assert np.all(np.isfinite(t)) and np.all(np.isfinite(r["ext"]))
    assert np.all((acc == 0) | (acc == 1)) and np.array_equal(acc, (np.sign(y) + 1) / 2)
    assert np.all(np.abs(y) >= p[:, 3:4])
    up = y > 0
    assert np.array_equal(s[:, 0], up.sum(1)) and np.array_equal(s[:, 1], (~up).sum(1)) and np.all(s[:, 2] == 0)
    tau = p[:, 3:4].astype(np.float64)
    units = np.floor((np.abs(y).astype(np.float64) - tau) * 65536.0 + 0.5)
    rt_q, rt = tau + units / 65536.0, np.abs(y).astype(np.float64)
    worst_plain = 0.0
    for b in range(B):
        m, v = _moments(rt_q[b], N)
        assert np.isclose(s[b, 3], m, rtol=2e-6, atol=2e-6), (b, s[b, 3], m)
        assert np.isclose(s[b, 4], v, rtol=2e-3, atol=1e-7), (b, s[b, 4], v)
        worst_plain = max(worst_plain, abs(s[b, 3] - rt[b].mean()))
        assert abs(s[b, 3] - rt[b].mean()) <= 2.0 ** -17 + 2e-6 + 2e-6 * rt[b].mean()
        n_up = int(up[b].sum())
        if n_up:
            m, v = _moments(rt_q[b][up[b]], n_up)
            assert np.isclose(s[b, 5], m, rtol=2e-6, atol=2e-6), (b, s[b, 5], m)
            assert np.isclose(s[b, 6], v, rtol=2e-3, atol=1e-7), (b, s[b, 6], v)
        else:
            assert np.isnan(s[b, 5]) and np.isnan(s[b, 6])
    print("mean_rt against the plain float64 mean of |y|: worst %.3g" % worst_plain)
    assert np.allclose(s[:, 9], acc.astype(np.float64).mean(1), rtol=0, atol=1e-6)
    # without the trials: the same summary bits
    assert rc.same_bits(_device(p, N, True, set_offset=so, want_trials=False)["summary"], s)
    # row blocks alone at their own set index: the same bits
    for lo, hi in {(0, 1), (B // 2, min(B, B // 2 + 3)), (B - 1, B), (max(0, B - 66), B)}:
        sub = _device(p[lo:hi], N, True, set_offset=so + lo, ext_sigma=0.1, ext_mode=0, want_ext=True)
        for k in ("trials", "summary", "ext"):
            assert rc.same_bits(sub[k], r[k][lo:hi]), (lo, hi, k)


@pytest.mark.parametrize("ext_mode", [0, 1])
def test_fast_mode_ext(ext_mode):
    """ext = centre + ext_sigma N(0, 1), centre Alpha (ext_mode 0) or 1: mean and spread of ext - centre within 4 sigma of their own
    sampling error (0.1 / sqrt(B) and 0.1 / sqrt(2 B))."""
    B = 20000
    p = prior_util.alpha_ns_prior(B, 9)
    e = _device(p, 2, True, set_offset=0, ext_sigma=0.1, ext_mode=ext_mode, want_ext=True, want_trials=False)["ext"].astype(np.float64)
    d = e - (p[:, 1].astype(np.float64) if ext_mode == 0 else 1.0)
    print("ext - centre: mean %.2e, std %.5f" % (d.mean(), d.std()))
    assert abs(d.mean()) < 2.8e-3
    assert abs(d.std() - 0.1) < 2e-3
