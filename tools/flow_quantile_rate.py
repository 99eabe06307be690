#!/usr/bin/env python3
"""Price of the posterior quantiles (csrc/train_quantile.hip, amortizer.draw_quantiles / posterior_summary) at the reference's inference
shapes: the default network (6 coupling layers, D = 5 parameters, C = 11 conditions) on basic_ddm_dc data sets, at (B = 1, S = 10 000) --
the reference's call -- and (B = 500, S = 10 000), its recovery loop as one call.  Two groups of legs per shape:
  the kernel alone, on one buffer of fused draws [B, S, 5]
    draw_quantiles_kernel        the five default probabilities (one launch: B x 5 workgroups, a full LDS sort each)
    torch_sort_dim1              torch.sort(theta, dim=1) on the same buffer (values and int64 indices written back)
  whole public calls
    posterior_moments            the parent's call that does the same sampling: the difference is the price of the quantiles
    posterior_summary            mean, std and the five quantiles, nothing of size B x S x P leaving the device
    sample_sort_on_device        what a user could do before: sample(fused=True, to_numpy=False), torch.sort, the interpolation
    sample_numpy_quantile        the reference's way: sample(fused=True) to the host, np.quantile
Timing: device events around each leg after a warm-up of every leg, the legs of a group ALTERNATING in one process, the median of
--reps (>= 20) per leg.  At B = 1 every leg is a handful of launches of microseconds each: launch-bound, no ratio is claimed there.
The kernel's answer is compared with the sort-and-interpolate answer at the timed size (bit for bit).

Usage: python tools/flow_quantile_rate.py [--json profiles/r30_flow_quantile_rate.json] [--reps 20]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((1, 10_000), (500, 10_000))
PROBS = (.005, .025, .5, .975, .995)


def _time(legs, reps):
    import torch
    for fn in legs.values():                                  # warm-up of every leg at the timed shape
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(reps):                                     # alternating
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: {"ms": float(np.median(v)), "ms_min": float(min(v)), "ms_max": float(max(v))} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    import torch
    from bayesflow_nddms_amd import amortizer as A, basic_ddm_dc, engine
    engine.require_device()
    torch.manual_seed(0)
    np.random.seed(2023)
    P = 5
    am = A.AmortizedPosterior(A.InvertibleNetwork(num_params=P), A.InvariantNetwork()).cuda().eval()
    gm = basic_ddm_dc.make_generative_model(batched=True, device_prior=True, as_numpy=False)
    p_dev = torch.as_tensor(PROBS, dtype=torch.float64, device="cuda")
    out = {"tool": "tools/flow_quantile_rate.py", "device": torch.cuda.get_device_name(0), "network": {"layers": 6, "D": P, "C": 11, "hidden": 128},
           "probs": list(PROBS), "reps": a.reps, "timing": "device events around each leg, legs of a group alternating, median", "shapes": []}

    def sort_and_interpolate(theta):                          # every draw finite: n = S
        srt = torch.sort(theta, dim=1).values
        h = (theta.shape[1] - 1) * p_dev
        j = h.floor().long()
        g = (h - j.double())[None, :, None]
        lo, hi = srt[:, j].double(), srt[:, torch.clamp(j + 1, max=theta.shape[1] - 1)].double()
        return lo + (hi - lo) * g

    for B, S in SHAPES:
        conf = basic_ddm_dc.configurator(gm(B))
        torch.manual_seed(1)
        theta = am.sample(conf, S, to_numpy=False, fused=True).reshape(B, S, P).contiguous()
        assert A._quantile_lib(theta, len(PROBS)) is not None, "the selection kernel does not take this buffer"
        keep = theta.clone()
        got = A.draw_quantiles(theta, PROBS)
        finite = bool(torch.isfinite(theta).all())
        agree = {"every_draw_finite": finite, "theta_unchanged": bool(torch.equal(theta, keep)),
                 "kernel_equals_sort_and_interpolate_bit_for_bit": bool(torch.equal(got["quantiles"], sort_and_interpolate(theta))) if finite else None}
        del keep, got
        kernel = _time({"draw_quantiles_kernel": lambda: A.draw_quantiles(theta, PROBS), "torch_sort_dim1": lambda: torch.sort(theta, dim=1)}, a.reps)
        calls = _time({"posterior_moments": lambda: am.posterior_moments(conf, S),
                       "posterior_summary": lambda: am.posterior_summary(conf, S, probs=PROBS),
                       "sample_sort_on_device": lambda: sort_and_interpolate(am.sample(conf, S, to_numpy=False, fused=True).reshape(B, S, P)).cpu(),
                       "sample_numpy_quantile": lambda: np.quantile(am.sample(conf, S, fused=True).reshape(B, S, P), PROBS, axis=1)}, a.reps)
        rec = {"B": B, "S": S, "workgroups": B * P, "results": agree, "kernel_alone": kernel, "whole_calls": calls,
               "kernel_over_torch_sort": kernel["draw_quantiles_kernel"]["ms"] / kernel["torch_sort_dim1"]["ms"],
               "kernel_below_torch_sort": kernel["draw_quantiles_kernel"]["ms"] < kernel["torch_sort_dim1"]["ms"],
               "posterior_summary_over_posterior_moments": calls["posterior_summary"]["ms"] / calls["posterior_moments"]["ms"],
               "launch_bound": B == 1}
        out["shapes"].append(rec)
        del theta
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
