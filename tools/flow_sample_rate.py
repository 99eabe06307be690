#!/usr/bin/env python3
"""Rate of the fused posterior sampler (csrc/train_sample.hip) at the reference's inference shapes, beside the PyTorch composition of
the SAME commit: the default network (6 coupling layers, D = 5 parameters, C = 11 conditions) on basic_ddm_dc data sets, at
(B = 1, S = 10 000) -- the reference's call, amortizer.sample(data, n_samples=10000), basic_ddm_dc.py:223 -- and (B = 500, S = 10 000), its
recovery loop as one call.  Three legs per shape, each the whole public call (summary network, base normals, flow):
    sample(fused=False, to_numpy=False)      the PyTorch path (the default, untouched)
    sample(fused=True, to_numpy=False)       the fused kernel
    posterior_moments(...)                   the fused kernel, statistics only (no draws in memory; ends in a copy of [B, P] to the host)
Timing: device events around each call after a warm-up of every leg, the legs ALTERNATING, the median of --reps (>= 20) per leg.  The
fused and the PyTorch draws of one seed are compared at the timed size (float32 round-off apart, not bit for bit).  For the record only:
the share of the f32-MFMA peak (157.3 TFLOP/s) of the whole call's time, at draws x sum over the 12 half-layers of 2 x 128 x (128 + Dh +
2 Dt) FLOP -- a whole-call rate over peak, not a kernel's.

Usage: python tools/flow_sample_rate.py [--json profiles/r27_flow_sample_rate.json] [--reps 20]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((1, 10_000), (500, 10_000))
PEAK_F32_MFMA = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    import torch
    from bayesflow_nddms_amd import basic_ddm_dc, engine
    from bayesflow_nddms_amd.amortizer import AmortizedPosterior, InvariantNetwork, InvertibleNetwork
    engine.require_device()
    torch.manual_seed(0)
    np.random.seed(2023)
    P, H = 5, 128
    am = AmortizedPosterior(InvertibleNetwork(num_params=P), InvariantNetwork()).cuda().eval()
    net = am.inference_net
    d1 = net.layers[0].d1
    flop_per_draw = len(net.layers) * sum(2 * H * (H + dh + 2 * dt) for dh, dt in ((d1, P - d1), (P - d1, d1)))
    gm = basic_ddm_dc.make_generative_model(batched=True, device_prior=True, as_numpy=False)
    out = {"tool": "tools/flow_sample_rate.py", "device": torch.cuda.get_device_name(0), "network": {"layers": len(net.layers), "D": P, "C": 11, "hidden": H},
           "reps": a.reps, "timing": "device events around the whole public call, legs alternating, median", "flop_per_draw": flop_per_draw,
           "shapes": []}
    for B, S in SHAPES:
        conf = basic_ddm_dc.configurator(gm(B))
        with torch.no_grad():                                 # (as sample() runs: the kernel is no autograd node)
            assert net._sample_lib(torch.zeros(B, 1, P, device="cuda"), am._conditions(conf)) is not None, "the fused sampler does not cover this network"
        legs = {"pytorch_sample": lambda: am.sample(conf, S, to_numpy=False),
                "fused_sample": lambda: am.sample(conf, S, to_numpy=False, fused=True),
                "fused_posterior_moments": lambda: am.posterior_moments(conf, S)}
        torch.manual_seed(1)
        plain = legs["pytorch_sample"]()
        torch.manual_seed(1)
        fused = legs["fused_sample"]()
        torch.manual_seed(1)
        mom = am.posterior_moments(conf, S, z_bytes=4 * B * S * P)      # (all sets in ONE launch: then its base normals are sample()'s)
        agree = {"max_abs_difference_of_draws_over_max_abs_draw": float((plain - fused).abs().max() / plain.abs().max()),
                 "max_abs_difference_of_means_moments_vs_fused_draws": float(np.abs(mom["mean"] - fused.reshape(B, S, P).double().mean(dim=1).cpu().numpy()).max())}
        del plain, fused
        for fn in legs.values():                              # warm-up of every leg at the timed shape
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in legs}
        for _ in range(a.reps):                               # alternating
            for k, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        rec = {"B": B, "S": S, "draws": B * S, "results": agree, "legs": {}}
        for k, v in ms.items():
            med = float(np.median(v))
            rec["legs"][k] = {"ms": med, "ms_min": float(min(v)), "ms_max": float(max(v)), "draws_per_second": B * S / (med * 1e-3),
                              "whole_call_share_of_f32_mfma_peak": B * S * flop_per_draw / (med * 1e-3) / PEAK_F32_MFMA}
        base = rec["legs"]["pytorch_sample"]["ms"]
        rec["speedup_fused_sample_over_pytorch"] = base / rec["legs"]["fused_sample"]["ms"]
        rec["speedup_fused_posterior_moments_over_pytorch"] = base / rec["legs"]["fused_posterior_moments"]["ms"]
        out["shapes"].append(rec)
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
