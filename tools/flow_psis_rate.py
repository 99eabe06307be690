#!/usr/bin/env python3
"""Price of the Pareto smoothing (csrc/train_psis.hip, amortizer.pareto_smooth / posterior_importance(smooth=True)) at the reference's
recovery shape, B = 500 data sets x S = 10 000 draws: the default network (6 coupling layers, D = 5 parameters, C = 11 conditions) on
basic_ddm_dc data sets of 180 trials.  Two groups of legs:
  the kernel alone, on one buffer of log weights [B, S]
    psis_kernel / torch_evaluation              that call's own log weights (an untrained flow's: every set fits, and its k-hat says
                                                what such weights are worth -- a median above 20)
    psis_kernel_broad / torch_evaluation_broad  log weights ~ N(0, 1): every set fits its M = 300 largest
    psis_kernel_diagnostic_broad                the same without the smoothed weights written (want_log_w=False)
    weighted_moments_broad                      the second weight-and-reduce launch on the smoothed weights
  whole public calls
    posterior_importance                        smooth=False: the parent's call
    posterior_importance_smooth                 smooth=True
    posterior_importance_probs / posterior_importance_probs_smooth   the same two with the five default probabilities
--control: only the first public leg, through calls the parent commit has as well; with --root it imports the package from another
checkout (the parent's, built): the control for "the default path is unchanged".
Timing: device events around each leg after a warm-up of every leg, the legs of a group ALTERNATING in one process, the median of
--reps (>= 20) per leg (--torch-reps for the torch evaluation).  The kernel's answer is compared with the torch
evaluation at the timed size.

Usage: python tools/flow_psis_rate.py [--json profiles/r34_flow_psis_rate.json] [--reps 20] [--control [--root DIR]]
"""
import argparse
import json
import os
import sys

import numpy as np

B, S, N_TRIALS = 500, 10_000, 180
PROBS = (.005, .025, .5, .975, .995)


def _time(legs, reps, slow=(), slow_reps=3):
    import torch
    for fn in legs.values():                                  # warm-up of every leg at the timed shape
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for rep in range(reps):                                   # alternating
        for k, fn in legs.items():
            if k in slow and rep >= slow_reps:
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: {"ms": float(np.median(v)), "ms_min": float(min(v)), "ms_max": float(max(v)), "reps": len(v)} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=20)
    ap.add_argument("--control", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from bayesflow_nddms_amd import amortizer as A, basic_ddm_dc, engine, priors
    engine.require_device()
    torch.manual_seed(0)
    P = 5
    am = A.AmortizedPosterior(A.InvertibleNetwork(num_params=P), A.InvariantNetwork()).cuda().eval()
    with torch.no_grad():                                     # untrained, but centred on the prior: most draws inside its support
        width = torch.tensor([1.0, 0.3, 0.15, 0.1, 0.3], device="cuda")
        am.inference_net.an_scale[0].copy_(-torch.log(width))
        am.inference_net.an_bias[0].copy_(-torch.tensor([0.0, 1.0, 0.5, 0.3, 1.0], device="cuda") / width)
    params = torch.as_tensor(priors.basic_prior_matrix(B, seed=5), device="cuda")
    sim = basic_ddm_dc.batch_simulate_trials(params, N_TRIALS, as_numpy=False, with_summary=False, seed=11)
    conf = basic_ddm_dc.configurator({"sim_data": sim["sim_data"], "sim_non_batchable_context": N_TRIALS, "prior_draws": params})
    out = {"tool": "tools/flow_psis_rate.py", "package": os.path.relpath(os.path.dirname(os.path.abspath(A.__file__))), "device": torch.cuda.get_device_name(0),
           "network": {"layers": 6, "D": P, "C": 11, "hidden": 128}, "B": B, "S": S, "n_trials": N_TRIALS, "probs": list(PROBS), "reps": a.reps,
           "timing": "device events around each leg, legs of a group alternating, median"}
    if a.control:
        out["whole_calls"] = _time({"posterior_importance": lambda: am.posterior_importance(conf, S)}, a.reps)
    else:
        torch.manual_seed(1)
        r = am.posterior_importance(conf, S, keep_draws=True, keep_weights=True)
        theta, log_w = torch.as_tensor(r["draws"], device="cuda"), torch.as_tensor(r["log_w"], device="cuda")
        del r
        broad = torch.randn(B, S, dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
        assert A._psis_lib(log_w) is not None, "the smoothing kernel does not take these buffers"
        gate = A._psis_lib

        def fallback(lw, **kw):
            A._psis_lib = lambda *x: None
            try:
                return A.pareto_smooth(lw, **kw)
            finally:
                A._psis_lib = gate

        res = {}
        for name, lw in (("own", log_w), ("broad", broad)):
            got, ref = A.pareto_smooth(lw), fallback(lw)
            fit = torch.isfinite(ref["pareto_k"])
            changed = got["log_w"] != lw
            res[name] = {"sets_with_a_finite_pareto_k": int(fit.sum()), "n_tail_median": float(got["n_tail"].double().median()),
                         "n_tail_and_cutoff_equal_torch": bool(torch.equal(got["n_tail"], ref["n_tail"]) and torch.equal(got["cutoff"], ref["cutoff"])),
                         "changed_rows_equal_torch": bool(torch.equal(changed, ref["log_w"] != lw)),
                         "non_finite_pareto_k_on_the_same_sets": bool(torch.equal(torch.isfinite(got["pareto_k"]), fit)),
                         "max_abs_pareto_k_difference": float((got["pareto_k"] - ref["pareto_k"])[fit].abs().max()) if bool(fit.any()) else 0.0,
                         "max_abs_smoothed_difference": float((got["log_w"] - ref["log_w"])[changed].abs().max()) if bool(changed.any()) else 0.0,
                         "pareto_k_median": float(got["pareto_k"][fit].median()) if bool(fit.any()) else None}
            del got, ref
        out["results"] = res
        smoothed = A.pareto_smooth(broad)["log_w"]
        kernel = _time({"psis_kernel": lambda: A.pareto_smooth(log_w),
                        "torch_evaluation": lambda: fallback(log_w),
                        "psis_kernel_broad": lambda: A.pareto_smooth(broad),
                        "torch_evaluation_broad": lambda: fallback(broad),
                        "psis_kernel_diagnostic_broad": lambda: A.pareto_smooth(broad, want_log_w=False),
                        "weighted_moments_broad": lambda: A.weighted_moments(theta, smoothed)}, a.reps,
                       slow=("torch_evaluation", "torch_evaluation_broad"), slow_reps=a.torch_reps)
        calls = _time({"posterior_importance": lambda: am.posterior_importance(conf, S),
                       "posterior_importance_smooth": lambda: am.posterior_importance(conf, S, smooth=True),
                       "posterior_importance_probs": lambda: am.posterior_importance(conf, S, probs=PROBS),
                       "posterior_importance_probs_smooth": lambda: am.posterior_importance(conf, S, probs=PROBS, smooth=True)}, a.reps)
        out.update(workgroups=B, kernel_alone=kernel, whole_calls=calls,
                   torch_evaluation_over_psis_kernel=kernel["torch_evaluation"]["ms"] / kernel["psis_kernel"]["ms"],
                   torch_evaluation_over_psis_kernel_broad=kernel["torch_evaluation_broad"]["ms"] / kernel["psis_kernel_broad"]["ms"],
                   psis_kernel_not_slower_than_torch=bool(kernel["psis_kernel"]["ms"] <= kernel["torch_evaluation"]["ms"]
                                                          and kernel["psis_kernel_broad"]["ms"] <= kernel["torch_evaluation_broad"]["ms"]),
                   smooth_over_default_call=calls["posterior_importance_smooth"]["ms"] / calls["posterior_importance"]["ms"],
                   probs_smooth_over_probs_call=calls["posterior_importance_probs_smooth"]["ms"] / calls["posterior_importance_probs"]["ms"])
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
