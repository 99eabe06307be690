"""Importance weights of the amortizer's draws on the device: the flow's log density out of the fused sampler (csrc/train_sample.hip:
flow_sample_logq_kernel) against the float64 forward of the same network with PyTorch's float32 composition as the yardstick
(tests/train_yardstick.py); the draws, sums and counts unmoved by it; stores confined to the outputs; the weight-and-reduce kernel
(csrc/train_importance.hip) against a recomputation from its own log weights; the three kernels end to end against an independent
float64 posterior (tests/flow_importance_ref.py, tests/golden/flow_importance.npz); and the public path."""
import copy
import math
import os

import numpy as np
import pytest

from flow_importance_ref import GOLDEN, PROPOSAL_DRAWS, PROPOSAL_SEED, mean_bound, numpy_importance, proposal_flow, special_inputs
from train_yardstick import _F64Yardstick

pytestmark = pytest.mark.gpu

U = 2.0 ** -52       # two orders of a recursive float64 sum of n terms differ by at most n 2^-52 sum|x_i|
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (layers, B, S, D, C): the battery of tests/test_gpu_flow_sample.py -- one draw; one short of / one past a 64-row and a 128-row tile;
# several tiles; D = 2 and 8; L = 1 and 8; C = 1 and the d + C = 32 edge: the shapes at which a per-row accumulator can go wrong
CASES = ((1, 1, 1, 5, 11), (1, 3, 5, 5, 11), (2, 1, 63, 5, 11), (6, 3, 65, 5, 11), (6, 1, 257, 5, 11), (6, 2, 130, 8, 11), (3, 4, 40, 2, 1),
         (6, 1, 129, 7, 12), (2, 5, 19, 3, 11), (8, 2, 33, 4, 28), (2, 1, 16, 6, 11), (6, 1, 1000, 5, 11))


def _net(D, C, layers, scale=None):
    """An InvertibleNetwork made ill-conditioned as tests/test_gpu_flow_sample.py makes its own."""
    import torch
    from bayesflow_nddms_amd.amortizer import InvertibleNetwork
    net = InvertibleNetwork(num_params=D, cond_dim=C, num_coupling_layers=layers, seed=layers).cuda().eval()
    with torch.no_grad():
        for p in net.parameters():
            p.mul_((3.0 if layers == 1 else 1.5) if scale is None else scale)
        for p in list(net.an_scale) + list(net.an_bias):
            p.copy_(0.3 * torch.randn_like(p))
    return net


def _launch(net, z, cond, **kw):
    import torch
    with torch.no_grad():
        L = net._sample_lib(z, cond)
        assert L is not None, "the fused sampler does not take this network / these tensors"
        return net._fused_sample(L, z, cond, **kw)


def _density64(net64, theta, cond_rep):
    """log q at theta through the float64 FORWARD: -|z|^2 / 2 - (D / 2) log 2 pi + log|det|."""
    z, log_det = net64(theta.double(), cond_rep.double())
    return -0.5 * (z ** 2).sum(-1) - 0.5 * theta.shape[-1] * math.log(2.0 * math.pi) + log_det


def test_log_q_against_float64():
    """Reference: the float64 copy's forward at the kernel's OWN theta (its z and log|det|); yardstick: inverse_with_log_density in float32,
    held to the same reference at ITS own theta.  _F64Yardstick takes one reference per tensor, so the kernel's error is carried over
    to the yardstick's reference (fused := ref_plain + (log_q_fused - ref_fused), in float64): both errors are then taken against
    ref_plain and scaled by its rms, the magnitude of log q in the case.  Default bounds: pooled relative rms fused <= 2 x PyTorch-f32 +
    32 x 2^-24, no case beyond 8 x."""
    import torch
    torch.manual_seed(3)
    yard = _F64Yardstick()
    for case in CASES:
        layers, B, S, D, C = case
        net = _net(D, C, layers)
        net64 = copy.deepcopy(net).double()
        z, cond = torch.randn(B, S, D, device="cuda"), torch.randn(B, C, device="cuda")
        z2, cond_rep = z.reshape(B * S, D), cond.repeat_interleave(S, dim=0)
        with torch.no_grad():
            assert net._sample_lib(z, cond) is not None, case
            th, lq = net.inverse_per_set(z, cond, log_density=True)
            assert th.shape == (B, S, D) and lq.shape == (B, S) and lq.dtype == torch.float32
            assert torch.equal(th, net.inverse_per_set(z, cond)), case
            th_p, lq_p = net.inverse_with_log_density(z2, cond_rep)
            ref_fused, ref_plain = _density64(net64, th.reshape(B * S, D), cond_rep), _density64(net64, th_p, cond_rep)
        assert bool(torch.isfinite(lq).all()), case
        yard.add("log_q", case, [ref_plain + (lq.reshape(-1).double() - ref_fused)], [lq_p], [ref_plain], ["log_q"])
    ratios = yard.finish()
    print(ratios)
    with open(os.path.join(ROOT, "profiles", "r31_flow_importance_yardstick.txt"), "w") as f:
        f.write("tests/test_gpu_flow_importance.py::test_log_q_against_float64: pooled relative rms error against float64, fused / pytorch f32\n")
        for k, v in ratios.items():
            f.write(f"{k}: {v}\n")


def test_asking_for_log_q_moves_nothing_else():
    """theta, sums and n_outside of a launch with log_q are those of a launch without it, bit for bit; log_q alone (no draws, no
    statistics) is a valid launch with the same bits; set 1 of B = 3 is the launch of set 1 alone, the first 63 draws of S = 65 the S = 63
    launch, log_q included; a repeated launch repeats every bit."""
    import torch
    torch.manual_seed(5)
    net = _net(5, 11, 6)
    z, cond = torch.randn(3, 65, 5, device="cuda"), torch.randn(3, 11, device="cuda")
    th0, sums0, n0 = _launch(net, z, cond, moments=True)
    th, sums, n_out, lq = _launch(net, z, cond, moments=True, log_q=True)
    assert torch.equal(th, th0) and torch.equal(sums, sums0) and torch.equal(n_out, n0)
    only = _launch(net, z, cond, draws=False, log_q=True)
    assert only[0] is None and only[1] is None and only[2] is None and torch.equal(only[3], lq)
    alone = _launch(net, z[1:2].contiguous(), cond[1:2].contiguous(), log_q=True)
    assert torch.equal(alone[0][0], th[1]) and torch.equal(alone[3][0], lq[1])
    short = _launch(net, z[:, :63].contiguous(), cond, log_q=True)
    assert torch.equal(short[0], th[:, :63]) and torch.equal(short[3], lq[:, :63])
    again = _launch(net, z, cond, moments=True, log_q=True)
    assert all(torch.equal(a, b) for a, b in zip(again, (th, sums, n_out, lq)))


def _guarded(n, dtype, sent, G=4096):
    import torch
    big = torch.full((2 * G + n,), sent, dtype=dtype, device="cuda")
    return big, big[G:G + n]


@pytest.mark.parametrize("B,S", [(1, 1), (2, 63), (3, 65)])
def test_nothing_is_written_outside_the_outputs(B, S):
    """log_q and every output of nddm_train_importance are views into sentinel-filled buffers with 4096-element guards: the guards are
    intact after the launches and every output element was written (the inputs' log_q is the sampler's own)."""
    import torch
    from bayesflow_nddms_amd.amortizer import importance_weights
    torch.manual_seed(6)
    D, sent = 5, -12345.0
    net = _net(D, 11, 2, scale=0.5)
    z, cond = torch.randn(B, S, D, device="cuda"), torch.randn(B, 11, device="cuda")
    big_q, view_q = _guarded(B * S, torch.float32, sent)
    th, _, _, lq = _launch(net, z, cond, log_q=True, log_q_out=view_q.view(B, S))
    assert lq.data_ptr() == view_q.data_ptr()
    shapes = {"log_evidence": (B,), "ess": (B,), "max_share": (B,), "mean": (B, D), "sd": (B, D), "n_zero": (B,), "n_nan": (B,), "log_w": (B, S)}
    bufs = {k: _guarded(int(np.prod(s)), torch.int64 if k.startswith("n_") else torch.float64, -12345 if k.startswith("n_") else sent)
            for k, s in shapes.items()}
    log_lik = torch.randn(B, S, dtype=torch.float64, device="cuda") - 20.0
    theta = (0.2 * torch.tanh(th) + torch.tensor([0.0, 1.0, 0.5, 0.5, 1.0], device="cuda")).contiguous()      # inside the prior's support
    res = importance_weights(theta, lq, log_lik, "basic", want_log_w=True, out={k: v[1].view(shapes[k]) for k, v in bufs.items()})
    torch.cuda.synchronize()
    for k, (big, view) in list(bufs.items()) + [("log_q", (big_q, view_q))]:
        G, n, s = 4096, view.numel(), (-12345 if k.startswith("n_") else sent)
        assert res.get(k, lq).data_ptr() == view.data_ptr(), k
        assert bool((big[:G] == s).all()) and bool((big[G + n:] == s).all()), k
        assert not bool((view == s).any()), k
    assert bool(torch.isfinite(res["mean"]).all()) and res["n_zero"].tolist() == [0] * B and res["n_nan"].tolist() == [0] * B


def test_reduce_kernel_against_its_own_log_weights():
    """B = 3, S = 300, D = 5 with the special rows of the CPU test (tests/flow_importance_ref.py::special_inputs).  The returned log_w obey
    the rule (NumPy's: equal where -inf, 1e-13 relative where finite -- the prior's logs differ by ulps) and the counts are equal as
    integers.  With u = exp(log_w - max log_w) recomputed in NumPy from the RETURNED log_w and theta, each float64 sum the outputs are made
    of -- sum u = 1 / max_share, sum u^2 = (sum u)^2 / ess, sum u theta = mean sum u, sum u theta^2 = (sd^2 + mean^2) sum u -- is within
    (S + 4) 2^-52 sum|terms| of NumPy's: S 2^-52 is the any-order bound, the 4 allows exp's few-ulp difference between the device's
    and NumPy's.  A set's outputs at B = 1 are its outputs at B = 3, bit for bit, and do not depend on asking for log_w."""
    import torch
    from bayesflow_nddms_amd.amortizer import _importance_lib, importance_weights
    S, D = 300, 5
    theta, log_q, log_lik = special_inputs(S)
    ref = numpy_importance(theta, log_q, log_lik)
    t, q, ll = (torch.as_tensor(v, device="cuda") for v in (theta, log_q, log_lik))
    assert _importance_lib(t, q, ll) is not None
    got_t = importance_weights(t, q, ll, "basic", want_log_w=True)
    got = {k: v.cpu().numpy() for k, v in got_t.items()}
    assert got["n_zero"].tolist() == ref["n_zero"].tolist() == [3, S, 0] and got["n_nan"].tolist() == ref["n_nan"].tolist() == [2, 0, 0]
    lw = got["log_w"]
    assert np.array_equal(np.isneginf(lw), np.isneginf(ref["log_w"])) and not np.isnan(lw).any()
    fin = np.isfinite(lw)
    assert np.all(np.abs(lw[fin] - ref["log_w"][fin]) <= 1e-13 * np.abs(ref["log_w"][fin]))
    assert np.isnan(got["mean"][1]).all() and np.isnan(got["sd"][1]).all() and np.isnan(got["max_share"][1])
    assert got["ess"][1] == 0.0 and np.isneginf(got["log_evidence"][1])
    th64 = theta.astype(np.float64)
    for b in (0, 2):
        pos = np.isfinite(lw[b])
        m = lw[b].max()
        u = np.exp(lw[b][pos] - m)
        sw = 1.0 / got["max_share"][b]
        pairs = [("sum u", sw, u), ("sum u^2", sw * sw / got["ess"][b], u * u)]
        for d in range(D):
            pairs.append((f"sum u theta_{d}", got["mean"][b, d] * sw, u * th64[b, pos, d]))
            pairs.append((f"sum u theta_{d}^2", (got["sd"][b, d] ** 2 + got["mean"][b, d] ** 2) * sw, u * th64[b, pos, d] ** 2))
        for name, kernel, terms in pairs:
            err, bound = abs(kernel - terms.sum()), (S + 4) * U * np.abs(terms).sum()
            print(f"set {b} {name}: error / bound {err / bound:.3g}")
            assert err <= bound, (b, name, kernel, terms.sum(), err, bound)
        le = m + np.log(u.sum() / S)
        assert abs(got["log_evidence"][b] - le) <= (S + 4) * U + 2 * U * abs(le), (b, got["log_evidence"][b], le)
    assert abs(got["ess"][2] - 1.0) < S * math.exp(-40.0) and abs(got["max_share"][2] - 1.0) < S * math.exp(-40.0)
    for b in range(3):
        one = importance_weights(t[b:b + 1].contiguous(), q[b:b + 1].contiguous(), ll[b:b + 1].contiguous(), "basic")
        assert "log_w" not in one
        for k, v in one.items():
            assert torch.equal(v[0].view(torch.int64), got_t[k][b].view(torch.int64)), (b, k)      # (bits: nan == nan)
    # the torch evaluation of the same definition on the device (float64 theta is not the kernel's to take)
    assert _importance_lib(t.double(), q, ll) is None
    other = importance_weights(t.double(), q, ll, "basic")
    for k in ("log_evidence", "ess", "max_share", "mean", "sd"):
        a, r = other[k].cpu().numpy(), got[k]
        ok = np.isfinite(r)
        assert np.array_equal(np.isnan(a), np.isnan(r)) and np.all(np.abs(a[ok] - r[ok]) <= 1e-11 * (1.0 + np.abs(r[ok]))), k
    assert torch.equal(other["n_zero"], got_t["n_zero"]) and torch.equal(other["n_nan"], got_t["n_nan"])


def test_end_to_end_against_an_independent_float64_posterior():
    """One basic_ddm_dc data set of 12 trials (tests/golden/flow_importance.npz) whose posterior mean, sd and log evidence the committed
    script tests/flow_importance_ref.py computed in float64 by importance sampling from the prior (its effective size is stored with
    them).  q is flow_importance_ref.proposal_flow: a near-identity flow, wide and off-centre in beta; the base normals are the CPU
    generator's under PROPOSAL_SEED, the draws the CPU check of the proposal saw.  Sampler with log q -> the Wiener likelihood launch ->
    the weight-and-reduce kernel.  CONDITION: the device run's ESS is at least 5 % of the 20 000 draws (1250 .. 1280 over three seeds
    on the CPU).  Bounds, four Monte-Carlo standard errors of the difference: per column |mean_dev - mean_ref| <= 4 sd_ref sqrt(1 / ESS_dev
    + 1 / ESS_ref); |log evidence_dev - log evidence_ref| <= 4 sqrt(1 / ESS_dev + 1 / ESS_ref).  The UNWEIGHTED mean of the same draws
    misses the first bound in the beta column (by a factor of about 4): without the weights the test fails."""
    import torch
    from bayesflow_nddms_amd import engine
    from bayesflow_nddms_amd.amortizer import importance_weights
    g = np.load(GOLDEN)
    net = proposal_flow(g["mean"], g["sd"]).cuda()
    z = torch.randn(1, PROPOSAL_DRAWS, 5, generator=torch.Generator().manual_seed(PROPOSAL_SEED)).cuda()
    cond = torch.zeros(1, 11, device="cuda")
    with torch.no_grad():
        assert net._sample_lib(z, cond) is not None
        th, lq = net.inverse_per_set(z, cond, log_density=True)
    trials = torch.as_tensor(g["trials"], device="cuda")[None]
    ll = engine.wiener_log_likelihood(engine.BASIC_DDM_DC, th.view(-1, 5), trials, draws_per_dataset=PROPOSAL_DRAWS)["loglik"].view(1, -1)
    w = {k: v.cpu().numpy()[0] for k, v in importance_weights(th, lq, ll, "basic").items()}
    ess, ess_ref = float(w["ess"]), float(g["ess"])
    print("ess", ess, "of", PROPOSAL_DRAWS, "n_zero", int(w["n_zero"]), "n_nan", int(w["n_nan"]), "max_share", float(w["max_share"]))
    assert int(w["n_nan"]) == 0
    assert ess >= 0.05 * PROPOSAL_DRAWS, ess
    bound = mean_bound(g["sd"], ess, ess_ref)
    err, err_plain = np.abs(w["mean"] - g["mean"]), np.abs(th[0].double().mean(dim=0).cpu().numpy() - g["mean"])
    print("weighted |mean - ref| / bound", err / bound, "unweighted", err_plain / bound)
    print("log evidence", float(w["log_evidence"]), "ref", float(g["log_evidence"]), "bound", 4.0 * math.sqrt(1.0 / ess + 1.0 / ess_ref))
    assert np.all(err <= bound), (err, bound)
    assert abs(float(w["log_evidence"]) - float(g["log_evidence"])) <= 4.0 * math.sqrt(1.0 / ess + 1.0 / ess_ref)
    assert np.any(err_plain > bound), (err_plain, bound)


def test_public_path(monkeypatch):
    """AmortizedPosterior.posterior_importance on basic_ddm_dc's configured batches: keep_draws returns the draws of sample(fused=True)
    under the same seed, bit for bit, and its numbers are importance_weights' on those draws, their log_q and the likelihood launch's
    values; one set per launch (a small z_bytes) gives each set the numbers of a B = 1 call at the same place of the random stream (the
    summary network is taken out of the comparison: a batch of two and a batch of one need not give a row the same bits);
    log_posterior at the kept draws -- the forward -- agrees with the sampler's log_q as two float32 evaluations of one float64
    number do: _F64Yardstick's bound with the float64 forward as the reference; models without a likelihood here are refused."""
    import torch
    from bayesflow_nddms_amd import basic_ddm_dc, diagnostics, engine
    from bayesflow_nddms_amd.amortizer import AmortizedPosterior, InvariantNetwork, InvertibleNetwork, importance_weights
    torch.manual_seed(0)
    np.random.seed(2023)
    B, S, P = 2, 257, 5
    gm = basic_ddm_dc.make_generative_model(batched=True, device_prior=True, as_numpy=False)
    am = AmortizedPosterior(InvertibleNetwork(num_params=P), InvariantNetwork()).cuda().eval()
    with torch.no_grad():                                     # an untrained flow, but centred on the prior: most draws inside its support
        width = torch.tensor([1.0, 0.3, 0.15, 0.1, 0.3], device="cuda")
        am.inference_net.an_scale[0].copy_(-torch.log(width))
        am.inference_net.an_bias[0].copy_(-torch.tensor([0.0, 1.0, 0.5, 0.3, 1.0], device="cuda") / width)
    conf = basic_ddm_dc.configurator(gm(B))
    torch.manual_seed(21)
    draws = am.sample(conf, S, fused=True, to_numpy=False)
    torch.manual_seed(21)
    r = am.posterior_importance(conf, S, keep_draws=True, keep_weights=True)
    assert r["n_samples"] == S and r["mean"].shape == (B, P) and r["std"].shape == (B, P) and r["draws"].dtype == np.float32
    assert all(r[k].shape == (B,) and r[k].dtype == np.float64 for k in ("ess", "log_evidence", "max_share"))
    assert np.array_equal(r["draws"], draws.cpu().numpy()) and r["log_w"].shape == (B, S) and r["log_q"].shape == (B, S)
    ll = diagnostics.posterior_log_likelihood(draws, conf["summary_conditions"], engine.BASIC_DDM_DC)
    w = importance_weights(draws.contiguous(), torch.as_tensor(r["log_q"], device="cuda"), ll, "basic", want_log_w=True)
    for k in ("mean", "sd", "ess", "log_evidence", "max_share", "n_zero", "n_nan", "log_w"):
        assert np.array_equal(w[k].cpu().numpy(), r["std" if k == "sd" else k], equal_nan=True), k
    assert np.array_equal(r["n_zero"] + r["n_nan"], np.isneginf(r["log_w"]).sum(axis=1)) and not np.isnan(r["log_w"]).any()
    print("public path: ess", r["ess"], "n_zero", r["n_zero"], "n_nan", r["n_nan"], "log evidence", r["log_evidence"])
    # one set per launch
    with torch.no_grad():
        cond_all = am._conditions(conf)
    monkeypatch.setattr(am, "_conditions", lambda d: cond_all[d["rows"]])
    part = lambda rows: {"rows": rows, "summary_conditions": conf["summary_conditions"][rows]}      # noqa: E731
    torch.manual_seed(22)
    split = am.posterior_importance(part(slice(0, 2)), S, z_bytes=1, keep_draws=True)
    torch.manual_seed(22)
    first = am.posterior_importance(part(slice(0, 1)), S, keep_draws=True)
    second = am.posterior_importance(part(slice(1, 2)), S, keep_draws=True)          # (the stream goes on where the first call left it)
    for k in ("mean", "std", "ess", "log_evidence", "max_share", "n_zero", "n_nan", "draws", "log_q"):
        assert np.array_equal(split[k][0], first[k][0], equal_nan=True) and np.array_equal(split[k][1], second[k][0], equal_nan=True), k
    assert not np.array_equal(split["draws"][0], split["draws"][1])
    # the forward's density at the kept draws against the sampler's
    lp = am.log_posterior(dict(part(slice(0, 2)), parameters=torch.as_tensor(split["draws"], device="cuda")), to_numpy=False)
    assert lp.shape == (B, S)
    net64 = copy.deepcopy(am.inference_net).double()
    with torch.no_grad():
        ref = _density64(net64, torch.as_tensor(split["draws"], device="cuda").reshape(B * S, P), cond_all.repeat_interleave(S, dim=0))
    yard = _F64Yardstick()
    yard.add("public", (B, S), [torch.as_tensor(split["log_q"], device="cuda").reshape(-1)], [lp.reshape(-1)], [ref], ["log_q"])
    print(yard.finish())
    with pytest.raises(NotImplementedError, match="single_trial_logpdf"):
        am.posterior_importance(conf, S, model="single")
