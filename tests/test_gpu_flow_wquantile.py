"""Weighted posterior quantiles on the device (csrc/train_wquantile.hip: one workgroup sorts a (set, column)'s (key, row) items in LDS
and scans the integer weights in sorted order; amortizer.py: weighted_draw_quantiles, posterior_importance(probs=...)): held to the
definition as tests/wquantile_ref.py recomputes it in Python integers -- bit for bit, on the kernel's own integer weights -- at the
smallest shapes a selection kernel goes wrong at, to the PyTorch evaluation on the same device tensors, to draw_quantiles' kernel at
equal weights, to its outputs' bounds, to independence of neighbours and row order, and through the public call."""
import ctypes

import numpy as np
import pytest

from test_flow_wquantile_cpu import DEFAULT, NAMES, OLD_KEYS, PROBS, check_crafted, check_properties
from wquantile_ref import bits, check, crafted_cases, quantize, skewed_log_w

pytestmark = pytest.mark.gpu


def _lib():
    from bayesflow_nddms_amd import _train_lib
    L = _train_lib.lib()
    assert L is not None, "libnddm_train.so did not build / load"
    return L


def _cap():
    return _lib().nddm_train_weighted_quantiles_max_draws()


def _same_bits(a, b):
    import torch
    v = {4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(v), b.contiguous().view(v))


def _same(a, b, keys=("quantiles", "order", "n_positive")):
    return all(_same_bits(a[k], b[k]) for k in keys)


def _fallback(theta, probs, **kw):
    """weighted_draw_quantiles with the kernel gated off: the PyTorch evaluation, on the same (device) tensors."""
    from bayesflow_nddms_amd import amortizer
    gate = amortizer._wquantile_lib
    amortizer._wquantile_lib = lambda *a: None
    try:
        return amortizer.weighted_draw_quantiles(theta, probs, **kw)
    finally:
        amortizer._wquantile_lib = gate


@pytest.mark.parametrize("B,S,D", [(1, 1, 2), (1, 2, 5), (3, 63, 5), (2, 64, 8), (1, 65, 1), (2, 257, 7), (1, 513, 3), (1, 4097, 3), (1, 10000, 5),
                                   (1, "cap", 2), (1, "cap + 1", 2)], ids=lambda v: str(v))
def test_exact_weighted_order_statistics(B, S, D):
    """One draw, either side of a wave and of the padding block of 64, S either side of the instantiations' sizes (... 257 take the
    512-item kernel, 513 the 4096, 4097, 10 000 -- the reference's -- and the cap the 16 384); cap + 1 takes the PyTorch evaluation and
    must give the same definition.  The kernel equals the reference evaluated on its OWN returned integer weights, bit for bit; those
    are within 1 of NumPy's; and given those weights the kernel equals the PyTorch evaluation on the same device tensors, bit for bit."""
    import torch
    from bayesflow_nddms_amd import amortizer
    kernel = S != "cap + 1"
    S = {"cap": _cap(), "cap + 1": _cap() + 1}.get(S, S)
    rng = np.random.default_rng(S + D)
    theta = (rng.normal(size=(B, S, D)) * rng.choice([1e-3, 1.0, 1e4], size=(1, 1, D))).astype(np.float32)
    lw = skewed_log_w(rng, B, S)
    t, w = torch.from_numpy(theta).cuda(), torch.from_numpy(lw).cuda()
    assert (amortizer._wquantile_lib(t, len(PROBS), w) is not None) == kernel
    res = amortizer.weighted_draw_quantiles(t, PROBS, log_w=w, want_weights=True)
    assert all(v.is_cuda for v in res.values())
    W = res["weights"].cpu().numpy()
    assert W.dtype == np.int64 and W.shape == (B, S) and np.abs(W - quantize(lw)).max() <= 1 and W.min() >= 0
    check(res, theta, W, PROBS)
    check_properties(res, theta, W)
    given = amortizer.weighted_draw_quantiles(t, PROBS, weights=res["weights"])
    ref = _fallback(t, PROBS, weights=res["weights"])
    assert _same(res, given) and _same(res, ref)
    assert np.array_equal(t.cpu().numpy(), theta) and np.array_equal(bits(w.cpu().numpy()), bits(lw))      # (the inputs are only read)


def test_crafted_rows():
    import torch
    from bayesflow_nddms_amd import amortizer
    for name, theta, lw in crafted_cases():
        t, w = torch.from_numpy(theta).cuda(), torch.from_numpy(lw).cuda()
        keep = t.clone()
        assert amortizer._wquantile_lib(t, len(PROBS), w) is not None
        res = amortizer.weighted_draw_quantiles(t, PROBS, log_w=w, want_weights=True)
        W = res["weights"].cpu().numpy()
        assert np.abs(W - quantize(lw)).max() <= 1, name
        check(res, theta, W, PROBS)
        check_properties(res, theta, W)
        check_crafted(name, res, theta, lw, W)
        assert _same(res, _fallback(t, PROBS, weights=res["weights"])), name
        assert _same_bits(t, keep), name


@pytest.mark.parametrize("S", [1, 64, 65, 1000, 10000])
def test_equal_weights_equal_the_unweighted_kernel(S):
    import torch
    from bayesflow_nddms_amd import amortizer
    rng = np.random.default_rng(S)
    theta = rng.normal(size=(2, S, 3)).astype(np.float32)
    if S > 1:
        theta[0, 0, 1] = np.nan
    t = torch.from_numpy(theta).cuda()
    assert amortizer._quantile_lib(t, len(PROBS)) is not None
    plain = amortizer.draw_quantiles(t, PROBS)
    for level in (0.0, -731.25):
        w = torch.full((2, S), level, dtype=torch.float64, device="cuda")
        assert amortizer._wquantile_lib(t, len(PROBS), w) is not None
        res = amortizer.weighted_draw_quantiles(t, PROBS, log_w=w)
        assert _same_bits(res["quantiles"], plain["quantiles"]) and _same_bits(res["order"], plain["order"])
        assert torch.equal(res["n_positive"], plain["n_inside"])


def test_a_set_depends_on_its_own_rows_only():
    """A repeated launch repeats every bit; set 1 of a B = 3 launch is that set launched alone; permuting the rows of sets whose
    values are distinct (rows and weights together) changes nothing."""
    import torch
    from bayesflow_nddms_amd.amortizer import weighted_draw_quantiles
    rng = np.random.default_rng(8)
    B, S, D = 3, 1000, 5
    theta = rng.normal(size=(B, S, D)).astype(np.float32)
    assert all(len(np.unique(theta[b, :, d])) == S for b in range(B) for d in range(D))
    theta[1, 7, 2] = np.nan
    lw = skewed_log_w(rng, B, S)
    t, w = torch.from_numpy(theta).cuda(), torch.from_numpy(lw).cuda()
    a, b = (weighted_draw_quantiles(t, PROBS, log_w=w, want_weights=True) for _ in range(2))
    alone = weighted_draw_quantiles(t[1:2].contiguous(), PROBS, log_w=w[1:2].contiguous(), want_weights=True)
    perm = torch.from_numpy(rng.permutation(S)).cuda()
    mixed = weighted_draw_quantiles(t[:, perm].contiguous(), PROBS, log_w=w[:, perm].contiguous(), want_weights=True)
    assert 0 < int(a["n_positive"].min()) and int(a["n_positive"].max()) < S
    for k in ("quantiles", "order", "n_positive", "weights"):
        assert _same_bits(a[k], b[k]) and _same_bits(a[k][1:2], alone[k]), k
    assert _same(a, mixed) and _same_bits(a["weights"][:, perm], mixed["weights"])


@pytest.mark.parametrize("S", [65, 513])
def test_nothing_is_written_outside_the_outputs(S):
    """quant, order, n_positive and w_out are interior pointers into larger buffers filled with a sentinel: the guards on both sides are
    unchanged and every output element was written; theta and log_w keep their bits; null `order`, `n_positive` and `w_out` are
    accepted, and so are integer weights in place of log_w."""
    import torch
    L = _lib()
    B, D, G, sent = 3, 5, 4096, -12345.0
    K = len(PROBS)
    rng = np.random.default_rng(S)
    theta = torch.from_numpy(rng.normal(size=(B, S, D)).astype(np.float32)).cuda()
    lw = torch.from_numpy(rng.normal(size=(B, S))).cuda()                                # (finite: every weight >= 1, none equal to the sentinel)
    keep, keep_w = theta.clone(), lw.clone()
    probs = (ctypes.c_double * K)(*PROBS)
    big_q = torch.full((2 * G + B * K * D,), sent, dtype=torch.float64, device="cuda")
    big_o = torch.full((2 * G + B * K * 2 * D,), sent, dtype=torch.float32, device="cuda")
    big_n = torch.full((2 * G + B,), -12345, dtype=torch.int64, device="cuda")
    big_w = torch.full((2 * G + B * S,), -12345, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def launch(order, n_positive, w_out, log_w=lw.data_ptr(), w_in=None):
        return L.nddm_train_weighted_quantiles(B, S, D, theta.data_ptr(), log_w, w_in, ctypes.addressof(probs), K, big_q[G:].data_ptr(),
                                               order, n_positive, w_out, st)

    assert launch(big_o[G:].data_ptr(), big_n[G:].data_ptr(), big_w[G:].data_ptr()) == 0
    torch.cuda.synchronize()
    for big, n, s in ((big_q, B * K * D, sent), (big_o, B * K * 2 * D, sent), (big_n, B, -12345), (big_w, B * S, -12345)):
        assert bool((big[:G] == s).all()) and bool((big[G + n:] == s).all())
        assert not bool((big[G:G + n] == s).any())
    res = {"quantiles": big_q[G:G + B * K * D].view(B, K, D), "order": big_o[G:G + B * K * 2 * D].view(B, K, 2, D), "n_positive": big_n[G:G + B]}
    W = big_w[G:G + B * S].view(B, S).clone()
    check(res, keep.cpu().numpy(), W.cpu().numpy(), PROBS)
    first = big_q.clone()
    for with_weights in (False, True):
        big_q.fill_(sent)
        big_o.fill_(sent)
        big_n.fill_(-12345)
        big_w.fill_(-12345)
        assert (launch(None, None, None, log_w=None, w_in=W.data_ptr()) if with_weights else launch(None, None, None)) == 0
        torch.cuda.synchronize()
        assert _same_bits(big_q, first) and bool((big_o == sent).all()) and bool((big_n == -12345).all()) and bool((big_w == -12345).all())
    assert _same_bits(theta, keep) and _same_bits(lw, keep_w)


def _people(ragged):
    """3 basic_ddm_dc data sets of 12 trials (ragged: 12, 9 and 7, as observed_batch pads them) and an untrained amortizer centred on
    the prior, as tests/test_gpu_flow_importance.py::test_public_path makes its own."""
    import torch
    from bayesflow_nddms_amd import basic_ddm_dc
    from bayesflow_nddms_amd.amortizer import AmortizedPosterior, InvariantNetwork, InvertibleNetwork, observed_batch
    torch.manual_seed(0)
    theta = np.array([[1.0, 1.2, 0.5, 0.3, 1.0], [0.2, 1.0, 0.45, 0.25, 1.1], [-0.8, 1.4, 0.55, 0.35, 0.9]], dtype=np.float32)
    sim = np.asarray(basic_ddm_dc.batch_simulate_trials(theta, 12, seed=2023, set_offset=0, with_summary=False)["sim_data"], dtype=np.float32)
    am = AmortizedPosterior(InvertibleNetwork(num_params=5), InvariantNetwork()).cuda().eval()
    with torch.no_grad():
        width = torch.tensor([1.0, 0.3, 0.15, 0.1, 0.3], device="cuda")
        am.inference_net.an_scale[0].copy_(-torch.log(width))
        am.inference_net.an_bias[0].copy_(-torch.tensor([0.0, 1.0, 0.5, 0.3, 1.0], device="cuda") / width)
    if ragged:
        return am, observed_batch([sim[0], sim[1, :9], sim[2, :7]], device="cuda")
    return am, {"summary_conditions": torch.from_numpy(sim).cuda(), "direct_conditions": torch.full((3, 1), float(np.log(12.0)), device="cuda")}


@pytest.mark.parametrize("ragged", [False, True], ids=["equal counts", "ragged"])
def test_public_path(monkeypatch, ragged):
    """B = 3, S = 2000, 12 trials.  probs=None returns the old keys; with probs, mean / std / ess / log_evidence (every old number) keep
    their bits under the same seed; the quantiles equal weighted_draw_quantiles on keep_draws' / keep_weights' outputs (the same log
    weights: the same integer weights, so bit for bit) and the reference on those integer weights; the named keys are there; the
    kernel was called, once per launch; and one set per launch (a small z_bytes) gives each set the bits of one launch of all sets
    whose every launch is seeded alike (the sampler, the weights and the selection are functions of a set's own rows)."""
    import torch
    from bayesflow_nddms_amd.amortizer import weighted_draw_quantiles
    B, S, P = 3, 2000, 5
    am, conf = _people(ragged)
    L = _lib()
    calls = []
    real = L.nddm_train_weighted_quantiles
    monkeypatch.setattr(L, "nddm_train_weighted_quantiles", lambda *a: calls.append(a[:3]) or real(*a))
    torch.manual_seed(21)
    old = am.posterior_importance(conf, S)
    assert set(old) == OLD_KEYS and not calls
    torch.manual_seed(21)
    new = am.posterior_importance(conf, S, probs=DEFAULT, keep_draws=True, keep_weights=True)
    assert calls == [(B, S, P)]
    assert set(new) == OLD_KEYS | {"quantiles", "probs", "draws", "log_q", "log_w"} | set(NAMES.values())
    for k in OLD_KEYS - {"n_samples"}:
        assert np.array_equal(bits(old[k]), bits(new[k])), k
    assert new["quantiles"].shape == (B, 5, P) and np.isfinite(new["quantiles"]).all() and np.array_equal(new["probs"], np.asarray(DEFAULT))
    for k, p in enumerate(DEFAULT):
        assert np.array_equal(bits(new[NAMES[p]]), bits(new["quantiles"][:, k]))
    draws, log_w = torch.as_tensor(new["draws"], device="cuda"), torch.as_tensor(new["log_w"], device="cuda")
    again = weighted_draw_quantiles(draws, DEFAULT, log_w=log_w, want_weights=True)
    assert len(calls) == 2 and np.array_equal(bits(again["quantiles"].cpu().numpy()), bits(new["quantiles"]))
    W = again["weights"].cpu().numpy()
    assert np.abs(W - quantize(new["log_w"])).max() <= 1 and int(again["n_positive"].min()) > 20
    check(again, new["draws"], W, DEFAULT)
    print("public path: ess", new["ess"], "n_positive", again["n_positive"].tolist(), "median", new["median"][0])
    # two launches (2 + 1 sets) and three (one set each) against one launch, every launch's base normals seeded per set
    with torch.no_grad():
        cond = am._conditions(conf)
    monkeypatch.setattr(am, "_conditions", lambda d: cond)
    randn = torch.randn

    def seeded(n, *a, **kw):                                   # the base normals of a launch: set b's under seed 100 + b, whatever the launch
        parts = []
        for _ in range(n // S):
            torch.manual_seed(100 + seeded.b)
            parts.append(randn(S, *a, **kw))
            seeded.b += 1
        return torch.cat(parts, dim=0)

    results = []
    for z_bytes in (64 << 20, 2 * 4 * S * P, 4 * S * P):
        seeded.b = 0
        monkeypatch.setattr(torch, "randn", seeded)
        n_calls = len(calls)
        results.append(am.posterior_importance(conf, S, probs=DEFAULT, z_bytes=z_bytes))
        monkeypatch.setattr(torch, "randn", randn)
        assert len(calls) - n_calls == {64 << 20: 1, 2 * 4 * S * P: 2, 4 * S * P: 3}[z_bytes]
    for other in results[1:]:
        for k in ("mean", "std", "ess", "log_evidence", "quantiles", "median", "99upper"):
            assert np.array_equal(bits(other[k]), bits(results[0][k])), k
