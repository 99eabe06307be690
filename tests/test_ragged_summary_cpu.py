"""CPU tests of the ragged batch -- data sets of different trial counts in one amortizer call: the PyTorch definition
(InvariantNetwork.forward(x, counts=...), which `summarize` takes wherever its kernels do not apply), the dict key `summary_counts`
through AmortizedPosterior, `observed_batch`, and the likelihood's view of a zero padding row on the host build of csrc/nddm_wiener.h."""
import os
import shutil
import sys
import tempfile

import numpy as np
import pytest
import torch

from bayesflow_nddms_amd.amortizer import AmortizedPosterior, InvariantNetwork, InvertibleNetwork, observed_batch
from conftest import ROOT

B, N, COUNTS = 5, 131, (131, 64, 65, 1, 100)
RTOL, ATOL = 1e-4, 1e-5           # tests/test_gpu_training.py's bound for "padding is invisible"
HAVE_CXX = not (shutil.which("g++") is None and shutil.which("c++") is None and shutil.which("clang++") is None)


def _net(blocks, seed=5, **kw):
    torch.manual_seed(seed)
    net = InvariantNetwork(num_equiv=blocks, **kw)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.copy_(0.1 * torch.randn_like(p))          # non-zero biases
    return net


def _trials(b=B, n=N, seed=7):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([0.3 + 2.0 * torch.rand(b, n, generator=g), (torch.rand(b, n, generator=g) < 0.7).float() * 2.0 - 1.0], dim=-1)


@pytest.mark.parametrize("blocks", [0, 1, 2])
def test_each_row_is_the_network_on_its_own_trials(blocks):
    """forward(x, counts=...) and summarize(x, counts), with and without direct conditions: row b is the network on x[b:b+1, :counts[b]];
    NaN in the padding changes no bit."""
    net, x = _net(blocks), _trials()
    direct = torch.log(torch.tensor(COUNTS, dtype=torch.float32)).view(B, 1)
    with torch.no_grad():
        alone = torch.cat([net(x[b:b + 1, :c]) for b, c in enumerate(COUNTS)])
        poisoned = x.clone()
        for b, c in enumerate(COUNTS):
            poisoned[b, c:] = float("nan")
        for counts in (COUNTS, list(COUNTS), torch.tensor(COUNTS), np.array(COUNTS, dtype=np.int32)):
            got = net(x, counts=counts)
            assert got.shape == (B, net.summary_dim) and torch.allclose(got, alone, rtol=RTOL, atol=ATOL)
            assert torch.equal(net(poisoned, counts=counts), got)
            assert torch.equal(net.summarize(x, counts), got) and torch.equal(net.summarize(poisoned, counts), got)
        with_d = net(x, counts=COUNTS, direct=direct)
        assert torch.equal(with_d, torch.cat([got, direct], dim=-1)) and torch.equal(net.summarize(x, COUNTS, direct), with_d)
        # no counts: every set has N trials
        assert torch.allclose(net.summarize(x), net(x, counts=[N] * B), rtol=RTOL, atol=ATOL) and torch.equal(net.summarize(x), net(x))


def test_counts_are_validated_on_the_host_and_exclude_the_batch_shared_forms():
    net, x = _net(1), _trials()
    mask, inv_n = torch.ones(1, N, 1), torch.tensor(1.0 / N)
    for kw in (dict(mask=mask, inv_n=inv_n), dict(n_valid=torch.tensor([100.0]))):
        with pytest.raises(ValueError, match="cannot be combined"):
            net(x, counts=COUNTS, **kw)
    for bad in ((131, 64, 65, 0, 100), (131, 64, 65, 1, 132), (131, 64, 65, 1), torch.tensor((131, 64, 65, -3, 100))):
        with pytest.raises(ValueError, match="counts"):
            net(x, counts=bad)
        with pytest.raises(ValueError, match="counts"):
            net.summarize(x, bad)


def test_the_existing_call_forms_keep_their_bits():
    """No mask, mask + inv_n and n_valid: the call with the new keyword absent and with counts=None is the same function twice."""
    net, x = _net(2), _trials()
    mask, inv_n, nv = (torch.arange(N) < 100).float().view(1, N, 1), torch.tensor(1.0 / 100), torch.tensor([100.0])
    direct = torch.randn(B, 3)
    with torch.no_grad():
        for args, kw in (((x,), {}), ((x, mask, inv_n), {}), ((x,), dict(n_valid=nv)), ((x,), dict(direct=direct)), ((x, mask, inv_n), dict(direct=direct))):
            assert torch.equal(net(*args, **kw), net(*args, counts=None, **kw))
        assert torch.allclose(net(x, mask, inv_n), net(x, counts=[100] * B), rtol=RTOL, atol=ATOL)


def _sets(counts=COUNTS, d=2, seed=11):
    rng = np.random.default_rng(seed)
    return [np.stack([0.3 + 2.0 * rng.random(n), np.sign(rng.random(n) - 0.3)] + [rng.normal(size=n)] * (d - 2), axis=1).astype(np.float32)
            for n in counts]


def test_observed_batch():
    sets = _sets()
    ob = observed_batch(sets)
    x, c, d = ob["summary_conditions"], ob["summary_counts"], ob["direct_conditions"]
    assert set(ob) == {"summary_conditions", "summary_counts", "direct_conditions"}
    assert x.shape == (B, N, 2) and x.dtype == torch.float32 and c.shape == (B,) and c.dtype == torch.int32 and d.shape == (B, 1) and d.dtype == torch.float32
    assert c.tolist() == list(COUNTS)
    assert np.array_equal(d[:, 0].numpy(), np.log(np.array(COUNTS, dtype=np.float64)).astype(np.float32))
    for b, s in enumerate(sets):
        assert np.array_equal(x[b, :len(s)].numpy(), s) and not x[b, len(s):].any()
    assert observed_batch([s.tolist() for s in sets[:2]])["summary_conditions"].shape == (2, 131, 2)       # (plain sequences too)
    with pytest.raises(ValueError, match="n_b >= 1"):
        observed_batch(sets + [np.zeros((0, 2), np.float32)])
    with pytest.raises(ValueError, match="same number of columns"):
        observed_batch(sets + _sets((7,), d=3))
    with pytest.raises(ValueError, match="at least one"):
        observed_batch([])


def _amortizer():
    torch.manual_seed(1)
    return AmortizedPosterior(InvertibleNetwork(num_params=5, num_coupling_layers=3, hidden=32), _net(2)).eval()


def test_sample_on_a_ragged_batch_gives_every_set_the_draws_of_its_own_condition():
    """sample(observed_batch(...), S) against the flow's inverse fed per-set conditions -- each from the summary network on the set's own
    trials and its log n -- and the same base normals.  (Without the feature the key is ignored and the padding summarised.)"""
    am, sets, S = _amortizer(), _sets(), 40
    ob = observed_batch(sets)
    torch.manual_seed(3)
    got = am.sample(ob, S, to_numpy=False)
    with torch.no_grad():
        cond = torch.cat([torch.cat([am.summary_net(torch.as_tensor(s)[None]), torch.tensor([[np.log(len(s))]], dtype=torch.float32)], dim=-1)
                          for s in sets])
        torch.manual_seed(3)
        z = torch.randn(B * S, 5)
        want = am.inference_net.inverse(z, cond.repeat_interleave(S, dim=0)).view(B, S, 5)
    assert got.shape == (B, S, 5) and torch.allclose(got, want, rtol=RTOL, atol=ATOL)
    torch.manual_seed(3)
    assert torch.allclose(am.sample(ob, S, to_numpy=False, fused=True), want, rtol=RTOL, atol=ATOL)
    # log_posterior takes the same dict
    lp = am.log_posterior(dict(ob, parameters=got), to_numpy=False)
    assert lp.shape == (B, S) and torch.isfinite(lp).all()
    m = am.posterior_moments(ob, S)
    assert m["mean"].shape == (B, 5) and np.isfinite(m["mean"]).all()


def test_summary_counts_excludes_the_batch_shared_keys_and_trains_through_pytorch():
    am, ob = _amortizer(), observed_batch(_sets())
    for extra in (dict(summary_n=torch.tensor([100.0])), dict(summary_mask=(torch.ones(1, N, 1), torch.tensor(1.0 / N)))):
        with pytest.raises(ValueError, match="cannot be combined"):
            am.sample(dict(ob, **extra), 3)
    loss = am.compute_loss(dict(ob, parameters=torch.randn(B, 5)))
    loss.backward()
    grads = [p.grad for p in am.summary_net.parameters()]
    assert torch.isfinite(loss) and all(g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0 for g in grads)
    assert all(torch.isfinite(p.grad).all() for p in am.inference_net.parameters() if p.grad is not None)
    # a dict without the key takes the path it took: the same call twice
    plain = {k: v for k, v in ob.items() if k != "summary_counts"}
    with torch.no_grad():
        assert torch.equal(am._conditions(plain), am._conditions(dict(plain)))
        assert not torch.allclose(am._conditions(plain), am._conditions(ob), rtol=RTOL, atol=ATOL)      # (there the padding is summarised)


@pytest.mark.skipif(not HAVE_CXX, reason="no host C++ compiler")
def test_a_zero_padding_row_is_log_one_to_the_likelihood_on_the_host():
    """csrc/nddm_wiener.h compiled for the host (tools/wiener_grad_host.py): (rt 0, choice 0) is a timeout censored at t = -tau <= 0 and
    scores log 1 = 0 with zero partials, so a row of trials padded with such rows has the log-likelihood and gradient of the trials."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import wiener_grad_host as GH
    good, tr = [0.8, 1.2, 0.45, 0.2, 1.1], [[0.6, 1.0], [0.9, -1.0], [1.4, 1.0], [1.1, 0.0]]
    with tempfile.TemporaryDirectory() as td:
        exe = GH.build(td)
        ev = lambda D: GH.evaluate(exe, td, 0, np.asarray([good], np.float32), np.asarray([D], np.float32), censored=True)      # noqa: E731
        ll, g = ev(tr)
        ll_pad, g_pad = ev(tr + [[0.0, 0.0]] * 5)
    assert np.isfinite(ll[0]) and ll[0] < 0 and np.array_equal(ll, ll_pad) and np.array_equal(g, g_pad)
