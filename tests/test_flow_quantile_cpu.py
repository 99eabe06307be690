"""Posterior quantiles (csrc/train_quantile.hip, amortizer.py: draw_quantiles / posterior_summary, diagnostics.summary) as far as a
machine without a GPU can hold them: the library's exports and host refusals, and the PyTorch evaluation of the definition -- the path
every CPU tensor takes and the one the kernel is held to bit for bit (tests/test_gpu_flow_quantile.py) -- against a NumPy recomputation
of the same formula (bit-equal) and against np.quantile (to the rounding of its other expression for the position)."""
import ctypes

import numpy as np
import pytest

PROBS = (0.0, .005, .025, .1, 1.0 / 3.0, .5, .975, .995, 1.0)
DEFAULT = (.005, .025, .5, .975, .995)
NAMES = {.5: "median", .025: "95lower", .975: "95upper", .005: "99lower", .995: "99upper"}
# np.quantile forms the position h by another expression than (n - 1) * p: the two differ by a few ulp of a number <= 2^15, i.e. <=
# 2^-35, and the quantile is continuous in h with slope at most the column's range
NP_BOUND = 2.0 ** -30


def reference(theta, probs, box=None):
    """The definition, in NumPy, one (set, column, probability) at a time: theta float32 [B, S, D] -> (quantiles [B, K, D] float64,
    order [B, K, 2, D] float32, n_inside [B])."""
    theta = np.asarray(theta, dtype=np.float32)
    B, S, D = theta.shape
    K = len(probs)
    quant, order, n_in = np.full((B, K, D), np.nan), np.full((B, K, 2, D), np.nan, dtype=np.float32), np.zeros(B, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        inside = np.isfinite(theta).all(axis=-1)
        if box is not None:
            lo, hi = (np.asarray(v, dtype=np.float32) for v in box)
            inside &= ((theta >= lo) & (theta <= hi)).all(axis=-1)
    for b in range(B):
        n = n_in[b] = int(inside[b].sum())
        if n == 0:
            continue
        for d in range(D):
            xs = np.sort(theta[b, inside[b], d])
            for k, p in enumerate(probs):
                h = np.float64(n - 1) * np.float64(p)
                j = int(np.floor(h))
                g = h - np.float64(j)
                a, c = xs[j], xs[min(j + 1, n - 1)]
                order[b, k, 0, d], order[b, k, 1, d] = a, c
                quant[b, k, d] = np.float64(a) + (np.float64(c) - np.float64(a)) * g
    return quant, order, n_in


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def check_against_reference(res, theta, probs, box=None):
    """res: draw_quantiles' dictionary (tensors) for theta (numpy float32): order equal as numbers (-0 == +0), quantiles bit for bit."""
    quant, order, n_in = reference(theta, probs, box)
    got_q, got_o, got_n = (res[k].cpu().numpy() for k in ("quantiles", "order", "n_inside"))
    assert got_q.dtype == np.float64 and got_o.dtype == np.float32 and got_n.dtype == np.int64
    assert got_q.shape == quant.shape and got_o.shape == order.shape and np.array_equal(got_n, n_in)
    assert np.array_equal(got_o, order, equal_nan=True)
    assert np.array_equal(bits(got_q), bits(quant)), np.abs(got_q - quant).max()


def crafted_cases():
    """(name, theta float32 [B, S, D], box or None): the rows a selection goes wrong on."""
    rng = np.random.default_rng(12)
    tiny = np.float32(1.4e-45)
    ties = rng.choice(np.array([-1.5, 0.25, 0.25000003, 7.0], dtype=np.float32), size=(2, 300, 3))
    zeros = rng.choice(np.array([0.0, -0.0, 1e-3, -1e-3], dtype=np.float32), size=(1, 129, 2), p=[.4, .4, .1, .1])
    denorm = (rng.integers(-40, 41, size=(1, 200, 2)).astype(np.float32) * tiny).astype(np.float32)
    same = np.full((1, 70, 2), 2.5, dtype=np.float32)
    same[0, :, 1] = rng.normal(size=70)
    mags = np.array([1e-38, 3e38, 1.0, 1e-45, 1e20, 1e-20, 65504.0, 0.0], dtype=np.float32)
    mixed = (rng.choice(mags, size=(2, 257, 3)) * rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=(2, 257, 3))).astype(np.float32)
    bad = rng.normal(size=(2, 150, 4)).astype(np.float32)
    bad[0, 3, 1], bad[0, 77, 2], bad[0, 149, 0], bad[1, 0, 3] = np.nan, np.inf, -np.inf, np.nan
    one = rng.normal(size=(2, 90, 3)).astype(np.float32)
    one[:, :, 0] = rng.uniform(2.0, 3.0, size=(2, 90))
    one[0, 41, 0], one[1, 5, 0] = 0.5, 0.25                         # the only rows whose column 0 lies in [0, 1]
    box_one = ([0.0, -100.0, -100.0], [1.0, 100.0, 100.0])
    box_none = ([10.0, -100.0, -100.0], [11.0, 100.0, 100.0])
    return [("ties", ties, None), ("zeros", zeros, None), ("denormals", denorm, None), ("one value", same, None), ("key map", mixed, None),
            ("nan / inf in another column", bad, None), ("one row inside", one, box_one), ("no row inside", one, box_none)]


def test_library_exports_the_entry_and_refuses_bad_arguments_on_the_host():
    """Called with null pointers everywhere, on the host: had the entry read or launched anything, this would not return."""
    from bayesflow_nddms_amd import _train_lib, build
    raw = ctypes.CDLL(build.build_train())
    assert hasattr(raw, "nddm_train_draw_quantiles") and hasattr(raw, "nddm_train_draw_quantiles_max_draws")
    L = _train_lib.lib()
    assert L is not None, "libnddm_train.so did not build / load"
    cap = L.nddm_train_draw_quantiles_max_draws()
    assert cap >= 10000
    good = (ctypes.c_double * 17)(*([0.5] * 17))
    pg = ctypes.addressof(good)

    def rc(B=1, S=100, D=5, K=5, probs=pg, theta=None, lo=None, hi=None, quant=None):
        return L.nddm_train_draw_quantiles(B, S, D, theta, lo, hi, probs, K, quant, None, None, None)

    assert rc() == 1                                                # a valid shape, null theta / quant
    assert rc(B=0) == 1 and rc(S=0) == 1 and rc(S=cap + 1) == 1 and rc(D=0) == 1 and rc(D=9) == 1 and rc(K=0) == 1 and rc(K=17) == 1
    assert rc(probs=None) == 1
    buf = (ctypes.c_char * 64)()
    a = ctypes.addressof(buf)
    for bad in (-0.1, 1.5, float("nan")):
        p = (ctypes.c_double * 5)(0.5, 0.5, bad, 0.5, 0.5)
        assert rc(probs=ctypes.addressof(p)) == 1 and rc(probs=ctypes.addressof(p), theta=a, quant=a) == 1, bad
    assert rc(theta=None, quant=a) == 1 and rc(theta=a, quant=None) == 1
    assert rc(theta=a, quant=a, lo=a) == 1 and rc(theta=a, quant=a, hi=a) == 1


@pytest.mark.parametrize("S", [1, 2, 3, 63, 64, 65, 257, 1000, 10001])
def test_draw_quantiles_on_cpu_tensors(S):
    import torch
    from bayesflow_nddms_amd.amortizer import draw_quantiles
    rng = np.random.default_rng(S)
    worst = 0.0
    for D in (1, 5, 8):
        for scale in (1e-3, 1.0, 1e4):
            theta = (rng.normal(size=(2, S, D)) * scale).astype(np.float32)
            res = draw_quantiles(torch.from_numpy(theta), PROBS)
            assert all(not v.is_cuda for v in res.values())
            check_against_reference(res, theta, PROBS)
            assert np.array_equal(res["order"][:, 0, 0].numpy(), theta.min(axis=1)) and np.array_equal(res["order"][:, -1, 1].numpy(), theta.max(axis=1))
            x = theta.astype(np.float64)
            want = np.quantile(x, PROBS, axis=1).transpose(1, 0, 2)                      # [B, K, D]
            span = (x.max(axis=1) - x.min(axis=1))[:, None, :]
            err = np.abs(res["quantiles"].numpy() - want)
            assert np.all(err <= NP_BOUND * span), (D, scale, (err / np.where(span > 0, span, 1.0)).max())
            worst = max(worst, float((err / np.where(span > 0, span, 1.0)).max()))
    print("S", S, "worst |quantile - np.quantile| / range", worst)
    one = draw_quantiles(torch.from_numpy(theta[0]), PROBS)                             # [S, D]: one set
    assert one["quantiles"].shape == (1, len(PROBS), 8) and torch.equal(one["quantiles"][0], res["quantiles"][0])


def test_crafted_rows():
    import torch
    from bayesflow_nddms_amd.amortizer import draw_quantiles
    for name, theta, box in crafted_cases():
        res = draw_quantiles(torch.from_numpy(theta), PROBS, box=box)
        check_against_reference(res, theta, PROBS, box)
        q, n = res["quantiles"].numpy(), res["n_inside"].numpy()
        if name == "zeros":
            assert not np.signbit(res["order"].numpy()[res["order"].numpy() == 0]).any()            # zeros come back as +0
        if name == "one value":
            assert np.all(q[:, :, 0] == 2.5)
        if name == "nan / inf in another column":
            assert n.tolist() == [147, 149] and np.all(np.isfinite(q))
            keep = np.isfinite(theta[0]).all(axis=-1)
            assert np.array_equal(res["order"][0, -1, 1].numpy(), theta[0][keep].max(axis=0))       # the row left EVERY column
        if name == "one row inside":
            assert n.tolist() == [1, 1]
            for b, r in ((0, 41), (1, 5)):
                assert np.all(q[b] == theta[b, r].astype(np.float64)[None, :]) and np.all(res["order"][b].numpy() == theta[b, r])
        if name == "no row inside":
            assert n.tolist() == [0, 0] and np.isnan(q).all() and np.isnan(res["order"].numpy()).all()
    with pytest.raises(ValueError):
        draw_quantiles(torch.zeros(1, 4, 3), [0.5, 2.0])
    with pytest.raises(ValueError):
        draw_quantiles(torch.zeros(1, 4, 3), [0.5], box=([0.0] * 2, [1.0] * 2))


def _amortizer(B, n=40, seed=0):
    import torch
    from bayesflow_nddms_amd.amortizer import AmortizedPosterior, InvariantNetwork, InvertibleNetwork
    torch.manual_seed(seed)
    am = AmortizedPosterior(InvertibleNetwork(num_params=5), InvariantNetwork()).eval()
    conf = {"summary_conditions": torch.randn(B, n, 2), "direct_conditions": torch.full((B, 1), float(np.log(n)))}
    return am, conf


def check_summary(s, draws, probs, box=None):
    """posterior_summary's dictionary against the formula on `draws` [B, S, P] float32, and its named keys against its rows."""
    quant, _, n_in = reference(draws, probs, box)
    assert s["quantiles"].dtype == np.float64 and np.array_equal(bits(s["quantiles"]), bits(quant))
    assert np.array_equal(s["n_outside"], draws.shape[1] - n_in) and np.array_equal(s["probs"], np.asarray(probs, dtype=np.float64))
    for k, p in enumerate(probs):
        if p in NAMES:
            assert np.array_equal(bits(s[NAMES[p]]), bits(s["quantiles"][:, k]))
    assert {"mean", "std", "quantiles", "probs", "n_outside", "n_samples"} <= set(s)
    assert set(NAMES.values()) & set(s) == {NAMES[p] for p in probs if p in NAMES}


def test_posterior_summary_on_the_cpu():
    """B = 3, S = 400.  One launch holds all sets, so the draws are sample()'s under the same seed; the moments are posterior_moments'
    bit for bit; the quantiles are the formula on the call's own draws; a box at the draws' own 10 % / 90 % column quantiles (a share
    in (0.2, 0.9) outside, as tests/test_flow_sample_cpu.py asserts it) leaves the quantiles of the inside draws alone; and one set per
    launch (z_bytes=1) gives what the sets give drawn one at a time, within 1e-5 of the draws' scale (that file's argument: the same
    base normals, the networks at batch 1 instead of 3; an order statistic moves by no more than the largest change of a draw)."""
    import torch
    B, S = 3, 400
    am, conf = _amortizer(B, seed=2)
    torch.manual_seed(9)
    draws = am.sample(conf, S)
    torch.manual_seed(9)
    m = am.posterior_moments(conf, S)
    torch.manual_seed(9)
    s = am.posterior_summary(conf, S, keep_draws=True)
    assert s["n_samples"] == S and s["draws"].dtype == np.float32 and np.array_equal(s["draws"], draws)
    assert np.array_equal(bits(s["mean"]), bits(m["mean"])) and np.array_equal(bits(s["std"]), bits(m["sd"]))
    assert np.array_equal(s["n_outside"], m["n_outside"]) and s["mean"].shape == s["median"].shape == (B, 5)
    check_summary(s, s["draws"], DEFAULT)
    assert set(NAMES.values()) <= set(s)
    torch.manual_seed(9)
    plain = am.posterior_summary(conf, S, probs=(.5, .1))
    assert "draws" not in plain and "95lower" not in plain and np.array_equal(bits(plain["median"]), bits(s["median"]))
    check_summary(plain, draws, (.5, .1))
    d64 = draws.astype(np.float64)
    lo, hi = np.quantile(d64.reshape(-1, 5), 0.1, axis=0), np.quantile(d64.reshape(-1, 5), 0.9, axis=0)
    lo32, hi32 = lo.astype(np.float32), hi.astype(np.float32)
    inside = ((draws >= lo32) & (draws <= hi32)).all(axis=-1)
    share = 1.0 - inside.mean()
    assert 0.2 < share < 0.9, share
    torch.manual_seed(9)
    mb = am.posterior_moments(conf, S, box=(lo, hi))
    torch.manual_seed(9)
    sb = am.posterior_summary(conf, S, box=(lo, hi), keep_draws=True)
    assert np.array_equal(sb["draws"], draws) and np.array_equal(sb["n_outside"], (~inside).sum(axis=1))
    assert np.array_equal(bits(sb["mean"]), bits(mb["mean"])) and np.array_equal(bits(sb["std"]), bits(mb["sd"]))
    check_summary(sb, draws, DEFAULT, box=(lo32, hi32))
    for b in range(B):
        assert np.array_equal(bits(sb["median"][b]), bits(reference(draws[b][inside[b]][None], (.5,))[0][0, 0]))
    scale = np.abs(draws).max()
    torch.manual_seed(9)
    one = am.posterior_summary(conf, S, z_bytes=1)
    torch.manual_seed(9)
    ref = np.stack([am.sample({k: v[b:b + 1] for k, v in conf.items()}, S) for b in range(B)])
    assert np.abs(one["mean"] - ref.astype(np.float64).mean(axis=1)).max() <= 1e-5 * scale
    assert np.abs(one["quantiles"] - reference(ref, DEFAULT)[0]).max() <= 1e-5 * scale
    with pytest.raises(ValueError):
        am.posterior_summary(conf, 10, box=([0.0] * 4, [1.0] * 4))
    with pytest.raises(ValueError):
        am.posterior_summary(conf, 10, probs=(.5, 2.0))


def check_mcmc_summary(res, samples):
    names = ("mean", "std", "median", "95lower", "95upper", "99lower", "99upper")
    assert set(res) == {k for k in samples if not k.startswith("_")}
    for key, r in res.items():
        x = np.asarray(samples[key], dtype=np.float64)
        allsamps = x.reshape(x.shape[:-2] + (-1,))
        assert tuple(r) == names
        for name in names:
            assert r[name].shape == x.shape[:-2] and r[name].dtype == np.float64, (key, name)
        assert np.array_equal(r["mean"], np.mean(allsamps, axis=-1)) and np.array_equal(r["std"], np.std(allsamps, axis=-1))
        span = allsamps.max(axis=-1) - allsamps.min(axis=-1)
        for name, p in zip(names[2:], (.5, .025, .975, .005, .995)):
            assert np.all(np.abs(r[name] - np.quantile(allsamps, p, axis=-1)) <= NP_BOUND * span), (key, name)


def test_mcmc_summary():
    """A synthetic sample dictionary in the JAGS layout ([..., iterations, chains], float32 values as the fits return them): the keys, the
    shapes [4] / [], the quantiles against np.quantile within the bound above, mean / std NumPy's; the `_` key is skipped."""
    from bayesflow_nddms_amd import diagnostics
    rng = np.random.default_rng(3)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)      # noqa: E731
    samples = {"delta": f32(rng.normal(1.0, 2.0, size=(4, 50, 3))), "sigma": f32(rng.gamma(2.0, size=(50, 3))), "_hidden": np.zeros((2, 2))}
    res = diagnostics.summary(samples)
    check_mcmc_summary(res, samples)
    assert res["delta"]["median"].shape == (4,) and res["sigma"]["median"].shape == () and "_hidden" not in res
