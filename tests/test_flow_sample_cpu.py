"""The fused posterior sampler (csrc/train_sample.hip, amortizer.py: inverse_per_set / sample(fused=True) / posterior_moments) as far
as a machine without a GPU can hold it: the library's exports and argument checks, and the Python paths' fallbacks, which must be the
PyTorch composition itself."""
import ctypes

import numpy as np
import pytest


def _amortizer(B, n=40, seed=0):
    import torch
    from bayesflow_nddms_amd.amortizer import AmortizedPosterior, InvariantNetwork, InvertibleNetwork
    torch.manual_seed(seed)
    am = AmortizedPosterior(InvertibleNetwork(num_params=5), InvariantNetwork()).eval()
    conf = {"summary_conditions": torch.randn(B, n, 2), "direct_conditions": torch.full((B, 1), float(np.log(n)))}
    return am, conf


def test_library_exports_the_sampler_and_refuses_bad_arguments_on_the_host():
    """libnddm_train.so cross-compiles with csrc/train_sample.hip in it and exports the entry and its work-size query; the entry
    answers 1 for every shape the gate refuses (hidden 64, no condition column, D = 9, no draws, no sets) and for a supported shape
    with null z / cond -- called with null pointers everywhere, on the host: had it read or launched anything, this would not return."""
    from bayesflow_nddms_amd import _train_lib, build
    raw = ctypes.CDLL(build.build_train())
    assert hasattr(raw, "nddm_train_flow_sample") and hasattr(raw, "nddm_train_flow_sample_work_bytes")
    L = _train_lib.lib()
    assert L is not None, "libnddm_train.so did not build / load"
    nulls = [None] * 11

    def rc(hidden=128, layers=6, B=1, S=100, D=5, d1=2, C=11):
        return L.nddm_train_flow_sample(hidden, layers, B, S, D, d1, C, 1.9, *nulls)

    assert rc() == 1                                        # supported shape, null params / perm / z / cond / work
    assert rc(hidden=64) == 1 and rc(C=0) == 1 and rc(D=9, d1=4) == 1 and rc(S=0) == 1 and rc(B=0) == 1 and rc(layers=9) == 1
    assert L.nddm_train_flow_supported(128, 6, 5, 2, 11) == 1                       # the gate is the training kernels', unchanged
    # one buffer at a time is given: everything else null still answers 1 (the pointers are only compared with null, never read)
    buf = (ctypes.c_char * 64)()
    a = ctypes.addressof(buf)
    perm = (ctypes.c_int * 30)(*([0, 1, 2, 3, 4] * 6))
    for missing in (2, 3):                                  # (params, perm, z, cond, theta, lo, hi, sums, n_outside, work, stream): z or cond null
        args = [a, ctypes.addressof(perm), a, a, a, None, None, None, None, a, None]
        args[missing] = None
        assert L.nddm_train_flow_sample(128, 6, 1, 100, 5, 2, 11, 1.9, *args) == 1, missing
    # the scratch: [B, 16, 128] floats of hoisted condition parts + per 128-draw tile 16 doubles and a count
    wb = L.nddm_train_flow_sample_work_bytes
    assert wb(1, 1, 5) == 16 * 128 * 4 + 136 and wb(3, 129, 5) == 3 * (16 * 128 * 4 + 2 * 136) and wb(1, 128, 8) == wb(1, 1, 8)
    assert wb(0, 10, 5) == 0 and wb(1, 0, 5) == 0 and wb(1, 10, 9) == 0
    assert wb(12000, 10000, 7) > 2 ** 27                    # (64-bit)


@pytest.mark.parametrize("B", [1, 3])
def test_fused_sample_on_cpu_tensors_is_the_default_bit_for_bit(B):
    """Without a device the fused option is the PyTorch composition on the same base normals: equal draws, bit for bit, under one
    seed -- with and without a rejection box (the generator is consumed identically: the redraws are the same too)."""
    import torch
    am, conf = _amortizer(B)
    torch.manual_seed(5)
    plain = am.sample(conf, 50)
    torch.manual_seed(5)
    fused = am.sample(conf, 50, fused=True)
    assert plain.shape == ((50, 5) if B == 1 else (B, 50, 5)) and plain.dtype == fused.dtype
    assert np.array_equal(plain, fused)
    box = ([-0.8] * 5, [0.8] * 5)
    torch.manual_seed(5)
    plain = am.sample(conf, 50, to_numpy=False, reject_outside=box)
    n_plain = am.last_redrawn
    torch.manual_seed(5)
    fused = am.sample(conf, 50, to_numpy=False, reject_outside=box, fused=True)
    assert torch.equal(plain, fused) and am.last_redrawn == n_plain > 0


def test_posterior_moments_fallback_is_a_float64_recomputation_of_the_draws():
    """posterior_moments on the CPU: the moments of sample()'s own draws (same seed: one launch holds all sets, so the base normals
    are the same) recomputed here in float64 with numpy.  Tolerances: the mean is a float64 sum of <= 400 float32 values in another
    order, relative error <= 400 x 2^-53 of sum|theta| -- 1e-12 of the largest |draw| is generous; the sd comes from sum(theta^2) /
    n - mean^2, whose cancellation loses (mean / sd)^2 ~ 10^2 at most here: 1e-10 relative.  With a box at the draws' own 10 % / 90 %
    column quantiles a draw is inside with probability ~0.8^5 = 0.33 (independent columns): the outside share is asserted to lie in
    (0.2, 0.9), n_outside equals the count, and the moments are those of the inside draws alone."""
    import torch
    B, S = 3, 400
    am, conf = _amortizer(B, seed=2)
    torch.manual_seed(9)
    draws = am.sample(conf, S).astype(np.float64)
    torch.manual_seed(9)
    m = am.posterior_moments(conf, S)
    assert set(m) == {"mean", "sd", "n_outside", "n_samples"} and m["n_samples"] == S
    assert m["mean"].shape == (B, 5) and m["sd"].shape == (B, 5) and m["n_outside"].shape == (B,)
    assert m["mean"].dtype == np.float64 and m["sd"].dtype == np.float64 and m["n_outside"].dtype == np.int64
    scale = np.abs(draws).max()
    assert np.all(m["n_outside"] == 0)
    assert np.abs(m["mean"] - draws.mean(axis=1)).max() <= 1e-12 * scale
    assert np.abs(m["sd"] / np.sqrt(np.var(draws, axis=1)) - 1.0).max() <= 1e-10
    lo, hi = np.quantile(draws.reshape(-1, 5), 0.1, axis=0), np.quantile(draws.reshape(-1, 5), 0.9, axis=0)
    lo32, hi32 = lo.astype(np.float32), hi.astype(np.float32)          # (the box is applied in float32, as sample's reject_outside)
    inside = ((draws >= lo32) & (draws <= hi32)).all(axis=-1)
    share = 1.0 - inside.mean()
    assert 0.2 < share < 0.9, share
    torch.manual_seed(9)
    mb = am.posterior_moments(conf, S, box=(lo, hi))
    assert np.array_equal(mb["n_outside"], (~inside).sum(axis=1))
    for b in range(B):
        d = draws[b][inside[b]]
        assert np.abs(mb["mean"][b] - d.mean(axis=0)).max() <= 1e-12 * scale
        assert np.abs(mb["sd"][b] / np.sqrt(np.var(d, axis=0)) - 1.0).max() <= 1e-10
    # sets are processed a launch at a time within a byte budget for z: one set per launch gives the same sets' numbers as sets
    # drawn one at a time (the same base normals; the networks run at batch 1 instead of 3, whose float32 GEMMs round otherwise:
    # 1e-5 of the draws' scale is float32's 6e-8 through ~50 layers with a wide margin, and far below any mix-up of sets or streams)
    torch.manual_seed(9)
    one = am.posterior_moments(conf, S, z_bytes=1)
    torch.manual_seed(9)
    ref = [am.sample({k: v[b:b + 1] for k, v in conf.items()}, S).astype(np.float64) for b in range(B)]
    assert np.abs(one["mean"] - np.array([r.mean(axis=0) for r in ref])).max() <= 1e-5 * scale
    with pytest.raises(ValueError):
        am.posterior_moments(conf, 10, box=([0.0] * 4, [1.0] * 4))


def test_inverse_per_set_falls_back_to_the_pytorch_inverse():
    """A hidden-32 network (the kernels are for width 128), and any network on CPU tensors: inverse_per_set is `inverse` on the
    condition repeated per draw, bit for bit; and it is the inverse of the forward."""
    import torch
    from bayesflow_nddms_amd.amortizer import InvertibleNetwork
    torch.manual_seed(4)
    for hidden in (32, 128):
        net = InvertibleNetwork(num_params=5, cond_dim=11, hidden=hidden).eval()
        z, cond = torch.randn(3, 7, 5), torch.randn(3, 11)
        assert net._sample_lib(z, cond) is None
        with torch.no_grad():
            got = net.inverse_per_set(z, cond)
            want = net.inverse(z.reshape(21, 5), cond.repeat_interleave(7, dim=0)).reshape(3, 7, 5)
            back, _ = net(got.reshape(21, 5), cond.repeat_interleave(7, dim=0))
        assert got.shape == (3, 7, 5) and torch.equal(got, want)
        assert float((back.reshape(3, 7, 5) - z).abs().max()) < 1e-4


def test_recovery_helpers_pass_the_fused_option_through():
    """posterior_estimates / posterior_recovery(fused=True) on the CPU: the same numbers as the default under the same seeds."""
    import torch
    from bayesflow_nddms_amd.amortizer import posterior_estimates, posterior_recovery
    am, _ = _amortizer(1)

    def gm(n):
        return {"parameters": torch.randn(n, 5), "summary_conditions": torch.randn(n, 30, 2), "direct_conditions": torch.full((n, 1), float(np.log(30.0)))}

    res = []
    for fused in (False, True):
        torch.manual_seed(11)
        est = posterior_estimates(am, gm, lambda d: d, n_datasets=4, n_samples=30, fused=fused)
        torch.manual_seed(11)
        res.append((est, posterior_recovery(am, gm, lambda d: d, n_datasets=4, n_samples=30, fused=fused)))
    for a, b in zip(res[0][0], res[1][0]):
        assert np.array_equal(a, b)
    assert np.array_equal(res[0][1], res[1][1])
