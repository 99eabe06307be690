"""The fused posterior sampler on the device (csrc/train_sample.hip: the flow's inverse as one kernel, amortizer.py: inverse_per_set,
sample(fused=True), posterior_moments): held to a float64 inverse of the same network with PyTorch's float32 composition as the
yardstick (tests/train_yardstick.py), row by row independence, stores confined to the outputs, the fused float64 statistics against a
recomputation from the same launch's draws, and the public path."""
import copy
import os

import numpy as np
import pytest

from train_yardstick import _F64Yardstick

pytestmark = pytest.mark.gpu

U = 2.0 ** -52       # the bound of the sums: recursive float64 summation of n terms in ANY order is within n u sum|x_i| (u = 2^-53) of
#                      the exact sum, so two orders differ by at most n 2^-52 sum|x_i|


def _net(D, C, layers, scale=None):
    """An InvertibleNetwork made ill-conditioned as tests/test_gpu_training.py::test_fused_flow_equals_the_pytorch_path makes its own."""
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


def _quantile_box(draws):
    """(lo, hi) float32 [D]: the 10 % / 90 % column quantiles of the finite draws."""
    import torch
    d = draws.reshape(-1, draws.shape[-1])
    d = d[torch.isfinite(d).all(dim=-1)]
    return torch.quantile(d, 0.1, dim=0).contiguous(), torch.quantile(d, 0.9, dim=0).contiguous()


CASES = ((1, 1, 1, 5, 11), (1, 3, 5, 5, 11), (2, 1, 63, 5, 11), (6, 3, 65, 5, 11), (6, 1, 257, 5, 11), (6, 2, 130, 8, 11), (3, 4, 40, 2, 1),
         (6, 1, 129, 7, 12), (2, 5, 19, 3, 11), (8, 2, 33, 4, 28), (2, 1, 16, 6, 11), (6, 1, 1000, 5, 11))


def test_fused_inverse_against_float64():
    """(layers, B, S, D, C): one draw; one short of / one past a 64-row and a 128-row tile; several tiles; D = 2 and 8; L = 1 and 8;
    C = 1 and the d + C = 32 edge.  Reference: the float64 copy's `inverse` on the expanded condition; yardstick: `inverse` in float32.
    _F64Yardstick's default bounds: pooled relative rms fused - f64 <= 2 x PyTorch-f32 - f64 + 32 x 2^-24, no case beyond 8 x.  Second
    group, the round trip: the float64 FORWARD of both float32 results against z."""
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
            fused = net.inverse_per_set(z, cond)
            assert fused.shape == (B, S, D) and fused.dtype == torch.float32
            fused = fused.reshape(B * S, D)
            plain = net.inverse(z2, cond_rep)
            exact = net64.inverse(z2.double(), cond_rep.double())
            back_fused, back_plain = (net64(v.double(), cond_rep.double())[0] for v in (fused, plain))
        assert bool(torch.isfinite(fused).all()), case
        yard.add("inverse", case, [fused], [plain], [exact], ["theta"])
        yard.add("round trip", case, [back_fused], [back_plain], [z2.double()], ["z"])
    ratios = yard.finish()
    print(ratios)
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r27_flow_sample_yardstick.txt")
    with open(path, "w") as f:
        f.write("tests/test_gpu_flow_sample.py::test_fused_inverse_against_float64: pooled relative rms error against float64, fused / pytorch f32\n")
        for k, v in ratios.items():
            f.write(f"{k}: {v}\n")


def test_a_draw_depends_on_its_own_row_only():
    """Set 1 of a B = 3 launch is the launch of set 1 alone; the first 63 draws of an S = 65 launch are the S = 63 launch on the same z
    rows; an identical launch repeats every bit, the statistics included."""
    import torch
    torch.manual_seed(5)
    net = _net(5, 11, 6)
    z, cond = torch.randn(3, 65, 5, device="cuda"), torch.randn(3, 11, device="cuda")
    th, sums, n_out = _launch(net, z, cond, moments=True)
    alone = _launch(net, z[1:2].contiguous(), cond[1:2].contiguous())[0]
    assert torch.equal(alone[0], th[1])
    short = _launch(net, z[:, :63].contiguous(), cond)[0]
    assert torch.equal(short, th[:, :63])
    th2, sums2, n_out2 = _launch(net, z, cond, moments=True)
    assert torch.equal(th2, th) and torch.equal(sums2, sums) and torch.equal(n_out2, n_out)


@pytest.mark.parametrize("B,S", [(1, 1), (2, 63), (3, 65)])
def test_nothing_is_written_outside_the_outputs(B, S):
    """theta, the sums and the counts are views into larger buffers filled with a sentinel: after the launch the guards on both sides
    are unchanged (a stray store lands in a guard) and every element of the outputs was written."""
    import torch
    torch.manual_seed(6)
    D, G, sent = 5, 4096, -12345.0
    net = _net(D, 11, 2)
    z, cond = torch.randn(B, S, D, device="cuda"), torch.randn(B, 11, device="cuda")
    big_t = torch.full((2 * G + B * S * D,), sent, device="cuda")
    big_s = torch.full((2 * G + B * 2 * D,), sent, dtype=torch.float64, device="cuda")
    big_n = torch.full((2 * G + B,), -12345, dtype=torch.int64, device="cuda")
    out, sums, n_out = big_t[G:G + B * S * D].view(B, S, D), big_s[G:G + B * 2 * D].view(B, 2 * D), big_n[G:G + B]
    _launch(net, z, cond, moments=True, out=out, sums=sums, n_outside=n_out)
    torch.cuda.synchronize()
    for big, n in ((big_t, B * S * D), (big_s, B * 2 * D), (big_n, B)):
        assert bool((big[:G] == sent).all()) and bool((big[G + n:] == sent).all())
        assert not bool((big[G:G + n] == sent).any())
    ref = _launch(net, z, cond)[0]
    assert torch.equal(out, ref) and bool((n_out == 0).all())


def test_fused_statistics_against_the_same_launchs_draws():
    """The float64 sums of theta and theta^2 over the inside draws, recomputed with torch from the draws the same launch returned:
    |sum_kernel - sum_ref| <= S 2^-52 sum|theta| (and sum theta^2 for the squares) -- the worst case of recursive summation for either
    order; n_outside equal as integers with a box at the draws' own 10 % / 90 % quantiles (a share in (0.2, 0.9) outside); a z row set
    to inf is counted outside and left out of the sums.  Statistics-only and draws-only launches repeat the full launch's bits, and a
    set's statistics at B = 1 are its statistics at B = 3."""
    import torch
    torch.manual_seed(7)
    B, S, D = 3, 300, 5
    net = _net(D, 11, 6)
    z, cond = torch.randn(B, S, D, device="cuda"), torch.randn(B, 11, device="cuda")
    z[1, 17, 2] = float("inf")
    free = _launch(net, z, cond, moments=True)
    assert not bool(torch.isfinite(free[0][1, 17]).all()) and free[2].tolist() == [0, 1, 0]
    box = _quantile_box(free[0])
    th, sums, n_out = _launch(net, z, cond, box=box, moments=True)
    same_bits = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))      # noqa: E731 (the inf row's draw is nan: nan != nan)
    assert same_bits(th, free[0])
    inside = torch.isfinite(th).all(dim=-1) & ((th >= box[0]) & (th <= box[1])).all(dim=-1)
    assert not bool(inside[1, 17])
    share = 1.0 - float(inside.double().mean())
    assert 0.2 < share < 0.9, share
    assert torch.equal(n_out, (~inside).sum(dim=1))
    t64 = torch.where(inside[..., None], th.double(), torch.zeros((), dtype=torch.float64, device="cuda"))
    for (got, free_got), ref, mag in (((sums[:, :D], free[1][:, :D]), t64.sum(dim=1), t64.abs().sum(dim=1)),
                                      ((sums[:, D:], free[1][:, D:]), (t64 * t64).sum(dim=1), (t64 * t64).sum(dim=1))):
        assert bool(torch.isfinite(got).all())
        err, bound = (got - ref).abs(), S * U * mag
        print("fused statistics: max error / bound", float((err / bound).max()))
        assert bool((err <= bound).all()), (err, bound)
        assert bool(torch.isfinite(free_got[[0, 2]]).all())               # (without a box the sets without the inf row sum every draw)
    only = _launch(net, z, cond, box=box, draws=False, moments=True)
    assert only[0] is None and torch.equal(only[1], sums) and torch.equal(only[2], n_out)
    draws = _launch(net, z, cond, box=box)
    assert draws[1] is None and draws[2] is None and same_bits(draws[0], th)
    for b in range(B):
        one = _launch(net, z[b:b + 1].contiguous(), cond[b:b + 1].contiguous(), box=box, draws=False, moments=True)
        assert torch.equal(one[1][0], sums[b]) and int(one[2][0]) == int(n_out[b])


@pytest.mark.parametrize("B", [1, 3])
def test_public_path(B, monkeypatch):
    """A real AmortizedPosterior on basic_ddm_dc's configured batches: sample(fused=True) has sample()'s shapes and is inverse_per_set on
    the same base normals, bit for bit; sample() never calls the new entry (it runs with the entry replaced by one that raises, and
    fused=True then does raise); reject_outside returns in-box draws only and counts them; posterior_moments under the same seed gives
    the float64 moments of sample(fused=True)'s draws to the summation bound (+ the roundings of the divisions: 2^-52 relative)."""
    import torch
    from bayesflow_nddms_amd import _train_lib, basic_ddm_dc
    from bayesflow_nddms_amd.amortizer import AmortizedPosterior, InvariantNetwork, InvertibleNetwork
    torch.manual_seed(0)
    np.random.seed(2023)
    S, P = 257, 5
    gm = basic_ddm_dc.make_generative_model(batched=True, device_prior=True, as_numpy=False)
    am = AmortizedPosterior(InvertibleNetwork(num_params=P), InvariantNetwork()).cuda().eval()
    conf = basic_ddm_dc.configurator(gm(B))
    net, seen = am.inference_net, []
    real = net.inverse_per_set
    monkeypatch.setattr(net, "inverse_per_set", lambda z, cond: seen.append((z, cond, real(z, cond))) or seen[-1][2])
    torch.manual_seed(21)
    out = am.sample(conf, S, fused=True, to_numpy=False)
    assert out.shape == ((S, P) if B == 1 else (B, S, P)) and out.is_cuda and am.last_redrawn == 0
    (z, cond, got), = seen
    assert z.shape == (B, S, P) and cond.shape == (B, 11)
    assert net._sample_lib(z, cond) is None                   # (here a gradient could be asked for: the kernel is no autograd node)
    torch.manual_seed(21)
    assert torch.equal(z.reshape(B * S, P), torch.randn(B * S, P, device="cuda"))            # the generator is consumed as sample() consumes it
    with torch.no_grad():                                     # as sample() runs
        assert net._sample_lib(z, cond) is not None
        assert torch.equal(out.reshape(B, S, P), got) and torch.equal(got, real(z, cond)) and torch.equal(got, _launch(net, z, cond)[0])
    as_np = am.sample(conf, S, fused=True)
    assert isinstance(as_np, np.ndarray) and as_np.shape == tuple(out.shape)
    # the fused draws are the default's draws to float32 round-off (an untrained flow is well conditioned: 1e-4 of the scale is ~1000 ulp)
    torch.manual_seed(21)
    plain = am.sample(conf, S, to_numpy=False)
    assert float((plain - out).abs().max()) <= 1e-4 * float(plain.abs().max())
    # moments, same seed
    torch.manual_seed(21)
    m = am.posterior_moments(conf, S)
    t64 = out.reshape(B, S, P).double()
    s1, s2, a1 = (v.cpu().numpy() for v in (t64.sum(dim=1), (t64 * t64).sum(dim=1), t64.abs().sum(dim=1)))
    assert m["n_samples"] == S and np.all(m["n_outside"] == 0) and m["mean"].shape == (B, P)
    assert np.all(np.abs(m["mean"] - s1 / S) <= (S * U * a1 + U * np.abs(s1)) / S)
    assert np.all(np.abs(m["sd"] ** 2 + m["mean"] ** 2 - s2 / S) <= (S + 8) * U * s2 / S)
    box = _quantile_box(out)
    box_np = tuple(v.cpu().numpy() for v in box)
    torch.manual_seed(21)
    mb = am.posterior_moments(conf, S, box=box_np)
    inside = ((out.reshape(B, S, P) >= box[0]) & (out.reshape(B, S, P) <= box[1])).all(dim=-1)
    assert np.array_equal(mb["n_outside"], (~inside).sum(dim=1).cpu().numpy()) and 0.2 * S < mb["n_outside"].min()
    # rejection
    seen.clear()
    boxed = am.sample(conf, S, fused=True, to_numpy=False, reject_outside=box_np, max_redraws=64)
    assert boxed.shape == out.shape and bool(((boxed >= box[0]) & (boxed <= box[1])).all()) and am.last_redrawn > 0.2 * S and len(seen) == 1
    # the default never touches the new entry
    L = _train_lib.lib()

    def refuse(*a):
        raise AssertionError("nddm_train_flow_sample called")

    monkeypatch.setattr(L, "nddm_train_flow_sample", refuse)
    torch.manual_seed(21)
    again = am.sample(conf, S, to_numpy=False)
    assert torch.equal(again, plain)
    with pytest.raises(AssertionError, match="nddm_train_flow_sample called"):
        am.sample(conf, S, fused=True)


def test_uncovered_network_takes_the_pytorch_path():
    """A hidden-32 flow with fused=True: the PyTorch inverse, bit-equal to fused=False (no kernel of this library covers it)."""
    import torch
    from bayesflow_nddms_amd.amortizer import AmortizedPosterior, InvariantNetwork, InvertibleNetwork
    torch.manual_seed(1)
    am = AmortizedPosterior(InvertibleNetwork(num_params=5, hidden=32), InvariantNetwork()).cuda().eval()
    conf = {"summary_conditions": torch.randn(2, 40, 2, device="cuda"), "direct_conditions": torch.full((2, 1), float(np.log(40.0)), device="cuda")}
    assert am.inference_net._sample_lib(torch.zeros(2, 9, 5, device="cuda"), torch.zeros(2, 11, device="cuda")) is None
    torch.manual_seed(8)
    a = am.sample(conf, 100, to_numpy=False)
    torch.manual_seed(8)
    b = am.sample(conf, 100, to_numpy=False, fused=True)
    assert torch.equal(a, b)
    torch.manual_seed(8)
    m = am.posterior_moments(conf, 100)
    assert np.allclose(m["mean"], a.double().mean(dim=1).cpu().numpy(), rtol=0, atol=1e-12 * float(a.abs().max()))
