#!/usr/bin/env python3
"""Price of the importance-weighted posterior (AmortizedPosterior.posterior_importance: csrc/train_sample.hip with log q, the Wiener
likelihood launch, csrc/train_importance.hip) at the reference's inference shapes: the default network (6 coupling layers, D = 5
parameters, C = 11 conditions) on basic_ddm_dc data sets of 180 trials, at (B = 1, S = 10 000) -- the reference's call -- and (B = 500,
S = 10 000), its recovery loop as one call.  Legs per shape, whole public calls:
    posterior_moments       the unweighted moments: the same sampling, no density, no likelihood
    posterior_importance    the weighted moments, ESS and log evidence, nothing of size B x S leaving the device
    composition             what a user had before: sample(fused=True, to_numpy=False), the PyTorch FORWARD on the condition expanded to
                            every draw for log q, diagnostics.posterior_log_likelihood, torch ops for the prior and the weights
                            (importance_weights' torch evaluation, on float64 draws so that the kernel does not take them)
and the weight-and-reduce kernel alone on one buffer of draws against that torch evaluation.
Timing: device events around each leg after a warm-up of every leg, the legs ALTERNATING in one process, the median of --reps (>= 20)
per leg.  At B = 1 every leg is a handful of launches of microseconds each: launch-bound, no ratio is claimed there.  The two routes'
answers are compared at the timed size on the same draws (counts equal; log evidence and weighted means differ by the float32
round-off of two routes to log q, the kernel's inverse and the PyTorch forward -- recorded, not bit for bit).

Usage: python tools/flow_importance_rate.py [--json profiles/r31_flow_importance_rate.json] [--reps 20]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((1, 10_000), (500, 10_000))
N_TRIALS = 180


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
    from bayesflow_nddms_amd import amortizer as A, basic_ddm_dc, diagnostics, engine, priors
    engine.require_device()
    torch.manual_seed(0)
    P = 5
    am = A.AmortizedPosterior(A.InvertibleNetwork(num_params=P), A.InvariantNetwork()).cuda().eval()
    with torch.no_grad():                                     # untrained, but centred on the prior: most draws inside its support
        width = torch.tensor([1.0, 0.3, 0.15, 0.1, 0.3], device="cuda")
        am.inference_net.an_scale[0].copy_(-torch.log(width))
        am.inference_net.an_bias[0].copy_(-torch.tensor([0.0, 1.0, 0.5, 0.3, 1.0], device="cuda") / width)
    table = priors.prior_table("basic")
    out = {"tool": "tools/flow_importance_rate.py", "device": torch.cuda.get_device_name(0), "network": {"layers": 6, "D": P, "C": 11, "hidden": 128},
           "n_trials": N_TRIALS, "reps": a.reps, "timing": "device events around each leg, legs alternating, median", "shapes": []}

    def composition(conf, S):
        th = am.sample(conf, S, to_numpy=False, fused=True)
        th = th[None] if th.dim() == 2 else th
        lq = am.log_posterior(dict(conf, parameters=th), to_numpy=False)
        ll = diagnostics.posterior_log_likelihood(th, conf["summary_conditions"], engine.BASIC_DDM_DC)
        return {k: v.cpu() for k, v in A.importance_weights(th.double(), lq, ll, table).items()}

    for B, S in SHAPES:
        params = torch.as_tensor(priors.basic_prior_matrix(B, seed=5), device="cuda")
        sim = basic_ddm_dc.batch_simulate_trials(params, N_TRIALS, as_numpy=False, with_summary=False, seed=11)
        conf = basic_ddm_dc.configurator({"sim_data": sim["sim_data"], "sim_non_batchable_context": N_TRIALS, "prior_draws": params})
        torch.manual_seed(1)
        new = am.posterior_importance(conf, S, z_bytes=1 << 34)       # (one launch: the base normals of sample())
        torch.manual_seed(1)
        old = {k: v.numpy() for k, v in composition(conf, S).items()}
        ok = np.isfinite(new["log_evidence"]) & np.isfinite(old["log_evidence"])
        # (an UNTRAINED flow: the effective size is about 1, a set's numbers are its heaviest draw's.  The two routes share the draws and
        # differ in log q by float32 round-off of two evaluations.)
        agree = {"median_ess": float(np.median(new["ess"])), "sets_with_a_positive_weight": int(ok.sum()),
                 "n_zero_equal": bool(np.array_equal(new["n_zero"], old["n_zero"])), "n_nan_equal": bool(np.array_equal(new["n_nan"], old["n_nan"])),
                 "max_abs_log_evidence_difference": float(np.max(np.abs(new["log_evidence"][ok] - old["log_evidence"][ok]))) if ok.any() else None,
                 "max_abs_mean_difference": float(np.max(np.abs(new["mean"][ok] - old["mean"][ok]))) if ok.any() else None}
        calls = _time({"posterior_moments": lambda: am.posterior_moments(conf, S),
                       "posterior_importance": lambda: am.posterior_importance(conf, S),
                       "composition": lambda: composition(conf, S)}, a.reps)
        torch.manual_seed(2)
        with torch.no_grad():
            th, lq = am.inference_net.inverse_per_set(torch.randn(B, S, P, device="cuda"), am._conditions(conf), log_density=True)
        ll = diagnostics.posterior_log_likelihood(th, conf["summary_conditions"], engine.BASIC_DDM_DC)
        assert A._importance_lib(th, lq, ll) is not None, "the weight-and-reduce kernel does not take these buffers"
        th64 = th.double()
        kernel = _time({"importance_kernel": lambda: A.importance_weights(th, lq, ll, table),
                        "torch_float64": lambda: A.importance_weights(th64, lq, ll, table)}, a.reps)
        out["shapes"].append({"B": B, "S": S, "workgroups": B, "results": agree, "whole_calls": calls, "kernel_alone": kernel,
                              "composition_over_posterior_importance": calls["composition"]["ms"] / calls["posterior_importance"]["ms"],
                              "posterior_importance_over_posterior_moments": calls["posterior_importance"]["ms"] / calls["posterior_moments"]["ms"],
                              "torch_over_kernel": kernel["torch_float64"]["ms"] / kernel["importance_kernel"]["ms"],
                              "draws_per_s": B * S / (1e-3 * calls["posterior_importance"]["ms"]), "launch_bound": B == 1})
        del th, th64, lq, ll
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
