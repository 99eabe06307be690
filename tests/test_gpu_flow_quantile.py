"""Posterior quantiles on the device (csrc/train_quantile.hip: one workgroup sorts a (set, column)'s keys in LDS; amortizer.py:
draw_quantiles, posterior_summary; diagnostics.summary): held to the definition as tests/test_flow_quantile_cpu.py recomputes it in
NumPy -- bit for bit -- at the smallest shapes a selection kernel goes wrong at, to the PyTorch evaluation on the crafted rows, to its
outputs' bounds, to independence of neighbours and row order, and through the public calls."""
import ctypes

import numpy as np
import pytest

from test_flow_quantile_cpu import DEFAULT, bits, check_against_reference, check_mcmc_summary, check_summary, crafted_cases

pytestmark = pytest.mark.gpu

PROBS = DEFAULT + (0.0, 1.0)


def _lib():
    from bayesflow_nddms_amd import _train_lib
    L = _train_lib.lib()
    assert L is not None, "libnddm_train.so did not build / load"
    return L


def _cap():
    return _lib().nddm_train_draw_quantiles_max_draws()


def _same_bits(a, b):
    import torch
    v = {4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(v), b.contiguous().view(v))


def _fallback(theta, probs, box=None):
    """draw_quantiles with the kernel gated off: the PyTorch evaluation, on the same (device) tensor."""
    from bayesflow_nddms_amd import amortizer
    gate = amortizer._quantile_lib
    amortizer._quantile_lib = lambda *a: None
    try:
        return amortizer.draw_quantiles(theta, probs, box=box)
    finally:
        amortizer._quantile_lib = gate


@pytest.mark.parametrize("B,S,D", [(1, 1, 2), (1, 2, 5), (3, 63, 5), (2, 64, 8), (1, 65, 1), (2, 257, 7), (1, 1000, 5), (1, 10000, 5), (1, "cap", 2),
                                   (1, "cap + 1", 2)], ids=lambda v: str(v))
def test_exact_order_statistics(B, S, D):
    """One draw, either side of a wave, a non-power-of-two S, S either side of the instantiations' sizes' use (63 ... 257 take the
    512-key kernel, 1000 the 4096, 10 000 -- the reference's -- the 16 384, the cap the 32 768); cap + 1 takes the PyTorch evaluation."""
    import torch
    from bayesflow_nddms_amd import amortizer
    kernel = S != "cap + 1"
    S = {"cap": _cap(), "cap + 1": _cap() + 1}.get(S, S)
    rng = np.random.default_rng(S + D)
    theta = (rng.normal(size=(B, S, D)) * rng.choice([1e-3, 1.0, 1e4], size=(1, 1, D))).astype(np.float32)
    t = torch.from_numpy(theta).cuda()
    assert (amortizer._quantile_lib(t, len(PROBS)) is not None) == kernel
    res = amortizer.draw_quantiles(t, PROBS)
    assert all(v.is_cuda for v in res.values())
    check_against_reference(res, theta, PROBS)
    assert np.array_equal(t.cpu().numpy(), theta)                                        # (theta is only read)


def test_crafted_rows_equal_the_pytorch_evaluation():
    import torch
    from bayesflow_nddms_amd import amortizer
    for name, theta, box in crafted_cases():
        t = torch.from_numpy(theta).cuda()
        keep = t.clone()
        assert amortizer._quantile_lib(t, len(PROBS)) is not None
        res, ref = amortizer.draw_quantiles(t, PROBS, box=box), _fallback(t, PROBS, box)
        for k in ("quantiles", "order", "n_inside"):
            assert _same_bits(res[k], ref[k]), (name, k)
        check_against_reference(res, theta, PROBS, box)
        assert _same_bits(t, keep), name


@pytest.mark.parametrize("S", [65, 257])
def test_nothing_is_written_outside_the_outputs(S):
    """quant, order and n_inside are interior pointers into larger buffers filled with a finite sentinel: the guards on both sides are
    unchanged and every output element was written; theta keeps its bits; null `order` and null `n_inside` are accepted."""
    import torch
    L = _lib()
    B, D, G, sent = 3, 5, 4096, -12345.0
    K = len(PROBS)
    rng = np.random.default_rng(S)
    theta = torch.from_numpy(rng.normal(size=(B, S, D)).astype(np.float32)).cuda()
    keep = theta.clone()
    probs = (ctypes.c_double * K)(*PROBS)
    big_q = torch.full((2 * G + B * K * D,), sent, dtype=torch.float64, device="cuda")
    big_o = torch.full((2 * G + B * K * 2 * D,), sent, dtype=torch.float32, device="cuda")
    big_n = torch.full((2 * G + B,), -12345, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def launch(order, n_inside):
        return L.nddm_train_draw_quantiles(B, S, D, theta.data_ptr(), None, None, ctypes.addressof(probs), K, big_q[G:].data_ptr(),
                                           order, n_inside, st)

    assert launch(big_o[G:].data_ptr(), big_n[G:].data_ptr()) == 0
    torch.cuda.synchronize()
    for big, n in ((big_q, B * K * D), (big_o, B * K * 2 * D), (big_n, B)):
        assert bool((big[:G] == sent).all()) and bool((big[G + n:] == sent).all())
        assert not bool((big[G:G + n] == sent).any())
    res = {"quantiles": big_q[G:G + B * K * D].view(B, K, D), "order": big_o[G:G + B * K * 2 * D].view(B, K, 2, D), "n_inside": big_n[G:G + B]}
    check_against_reference(res, keep.cpu().numpy(), PROBS)
    first = big_q.clone()
    big_o.fill_(sent)
    big_n.fill_(-12345)
    assert launch(None, None) == 0
    torch.cuda.synchronize()
    assert _same_bits(big_q, first) and bool((big_o == sent).all()) and bool((big_n == -12345).all())
    assert _same_bits(theta, keep)


def test_a_set_depends_on_its_own_rows_only():
    """A repeated launch repeats every bit; set 1 of a B = 3 launch is that set launched alone; permuting a set's rows changes nothing."""
    import torch
    from bayesflow_nddms_amd.amortizer import draw_quantiles
    rng = np.random.default_rng(8)
    B, S, D = 3, 1000, 5
    theta = rng.normal(size=(B, S, D)).astype(np.float32)
    theta[1, 7, 2] = np.nan
    t = torch.from_numpy(theta).cuda()
    box = ([-2.5] * D, [2.5] * D)
    a, b = draw_quantiles(t, PROBS, box=box), draw_quantiles(t, PROBS, box=box)
    alone = draw_quantiles(t[1:2].contiguous(), PROBS, box=box)
    perm = torch.from_numpy(rng.permutation(S)).cuda()
    mixed = draw_quantiles(t[:, perm].contiguous(), PROBS, box=box)
    assert 0 < int(a["n_inside"].min()) and int(a["n_inside"].max()) < S
    for k in ("quantiles", "order", "n_inside"):
        assert _same_bits(a[k], b[k]) and _same_bits(a[k][1:2], alone[k]) and _same_bits(a[k], mixed[k]), k


def _amortizer():
    """The default network on basic_ddm_dc's configured batches, made ill-conditioned as tests/test_gpu_flow_sample.py::_net makes its own."""
    import torch
    from bayesflow_nddms_amd import basic_ddm_dc
    from bayesflow_nddms_amd.amortizer import AmortizedPosterior, InvariantNetwork, InvertibleNetwork
    torch.manual_seed(0)
    np.random.seed(2023)
    am = AmortizedPosterior(InvertibleNetwork(num_params=5), InvariantNetwork()).cuda().eval()
    net = am.inference_net
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(1.5)
        for p in list(net.an_scale) + list(net.an_bias):
            p.copy_(0.3 * torch.randn_like(p))
    gm = basic_ddm_dc.make_generative_model(batched=True, device_prior=True, as_numpy=False)
    return am, basic_ddm_dc.configurator(gm(3))


def test_public_path(monkeypatch):
    """B = 3, S = 1000: posterior_summary's quantiles are the formula on its own draws, with and without priors.prior_box("basic") (the
    ill-conditioned network throws draws outside it or not -- n_outside is compared either way); mean / std / n_outside are
    posterior_moments' bits under the same seed; the same numbers without keep_draws; and one set per launch gives each set's numbers
    as that set run alone under the same per-launch seed.  Both kernels are on the path (the sampler's and the selection's entries
    are counted)."""
    import torch
    from bayesflow_nddms_amd import priors
    B, S, P = 3, 1000, 5
    am, conf = _amortizer()
    L = _lib()
    calls = []
    real = L.nddm_train_draw_quantiles
    monkeypatch.setattr(L, "nddm_train_draw_quantiles", lambda *a: calls.append(a[:3]) or real(*a))
    for box in (None, priors.prior_box("basic")):
        torch.manual_seed(21)
        m = am.posterior_moments(conf, S, box=box)
        torch.manual_seed(21)
        s = am.posterior_summary(conf, S, box=box, keep_draws=True)
        assert s["draws"].shape == (B, S, P) and calls[-1] == (B, S, P)
        for a, b in ((s["mean"], m["mean"]), (s["std"], m["sd"])):
            assert np.array_equal(bits(a), bits(b))
        assert np.array_equal(s["n_outside"], m["n_outside"])
        check_summary(s, s["draws"], DEFAULT, box=None if box is None else tuple(np.asarray(v, dtype=np.float32) for v in box))
        torch.manual_seed(21)
        plain = am.posterior_summary(conf, S, box=box)
        assert "draws" not in plain
        for k in ("mean", "std", "quantiles", "median", "95lower", "95upper", "99lower", "99upper"):
            assert np.array_equal(bits(plain[k]), bits(s[k])), k
    # One set per launch against each set run alone, every launch seeded alike.  Both take the SAME condition rows (the summary
    # network's float32 GEMMs may round a set's row otherwise at batch 1 than at batch 3, which is not this call's business):
    # the sampler and the selection are functions of a set's own rows, so the numbers are equal bit for bit.
    n_calls = len(calls)
    with torch.no_grad():
        cond = am._conditions(conf)
    one = []
    for b in range(B):
        monkeypatch.setattr(am, "_conditions", lambda d, b=b: cond[b:b + 1])
        torch.manual_seed(100 + b)
        one.append(am.posterior_summary(None, S))
    monkeypatch.setattr(am, "_conditions", lambda d: cond)
    seeds = iter(range(100, 100 + B))
    randn = torch.randn
    monkeypatch.setattr(torch, "randn", lambda *a, **kw: (torch.manual_seed(next(seeds)), randn(*a, **kw))[1])
    per_set = am.posterior_summary(None, S, z_bytes=4 * S * P)
    monkeypatch.setattr(torch, "randn", randn)
    assert len(calls) == n_calls + 2 * B and calls[-1] == (1, S, P)
    for b in range(B):
        for k in ("mean", "std", "quantiles", "median", "n_outside"):
            assert np.array_equal(bits(per_set[k][b:b + 1]), bits(one[b][k])), (b, k)


def test_mcmc_summary_on_a_small_fit(monkeypatch):
    """One hmc_fit of 2 participants x 40 trials, 2 chains, 20 + 40 iterations: diagnostics.summary through the kernel equals, bit for
    bit, the PyTorch evaluation on the same samples, and np.quantile within the CPU file's bound."""
    import sys
    import os
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import wiener_hmc_host as H
    from bayesflow_nddms_amd import amortizer, basic_ddm_dc, diagnostics
    fit = basic_ddm_dc.fit_hmc(H.example_data(2, 40, 31), chains=2, warmup=20, samples=40, thin=1, seed=8)
    samples = {k: fit[k] for k in ("alpha", "ndt", "beta", "delta", "varsigma")}
    samples["_skipped"] = fit["log_post"]
    L = _lib()
    calls = []
    real = L.nddm_train_draw_quantiles
    monkeypatch.setattr(L, "nddm_train_draw_quantiles", lambda *a: calls.append(a[:3]) or real(*a))
    dev = diagnostics.summary(samples)
    assert calls == [(2, 80, 1)] * 5
    monkeypatch.setattr(amortizer, "_quantile_lib", lambda *a: None)
    ref = diagnostics.summary(samples)
    assert len(calls) == 5
    for key in ref:
        for name in ref[key]:
            assert np.array_equal(bits(dev[key][name]), bits(ref[key][name])), (key, name)
    for v in samples.values():
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v)               # (the fit's samples are float32 values)
    check_mcmc_summary(dev, samples)
