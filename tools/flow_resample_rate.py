#!/usr/bin/env python3
"""Price of sampling-importance-resampling (csrc/train_resample.hip, amortizer.resample_draws / posterior_importance(resample=M)) at the
reference's recovery shape, B = 500 data sets x S = 10 000 draws x D = 5, M = 10 000 outputs per set: the default network (6 coupling
layers, D = 5 parameters, C = 11 conditions) on basic_ddm_dc data sets of 180 trials.  Two groups of legs:
  the kernel alone, on that call's own draws and log weights
    resample_kernel / torch_evaluation          from the log weights (the kernel quantises them itself; torch: quantize_weights first)
    resample_kernel_weights / torch_evaluation_weights   from the kernel's integer weights: the two agree bit for bit (checked here)
    resample_kernel_broad / torch_evaluation_broad       the same draws with log weights ~ N(0, 1): every row weighs something and most
                                                are chosen (an untrained flow's own weights at 180 trials leave a handful of rows)
  whole public calls
    posterior_importance                        resample=None: the parent's call
    posterior_importance_resample               resample=10 000
    posterior_importance_smooth / posterior_importance_smooth_resample   the same two with smooth=True
--control: only the first public leg, through a call the parent commit has as well; with --root it imports the package from another
checkout (the parent's, built): the control for "the default path is unchanged".
Timing: device events around each leg after a warm-up of every leg, the legs of a group ALTERNATING in one process, the median of
--reps (>= 20) per leg.

Usage: python tools/flow_resample_rate.py [--json profiles/r35_flow_resample_rate.json] [--reps 20] [--control [--root DIR]]
"""
import argparse
import json
import os
import sys

import numpy as np

B, S, M, N_TRIALS = 500, 10_000, 10_000, 180


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
    return {k: {"ms": float(np.median(v)), "ms_min": float(min(v)), "ms_max": float(max(v)), "reps": len(v)} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--reps", type=int, default=20)
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
    out = {"tool": "tools/flow_resample_rate.py", "package": os.path.relpath(os.path.dirname(os.path.abspath(A.__file__))), "device": torch.cuda.get_device_name(0),
           "network": {"layers": 6, "D": P, "C": 11, "hidden": 128}, "B": B, "S": S, "M": M, "n_trials": N_TRIALS, "reps": a.reps,
           "timing": "device events around each leg, legs of a group alternating, median"}
    if a.control:
        out["whole_calls"] = _time({"posterior_importance": lambda: am.posterior_importance(conf, S)}, a.reps)
    else:
        torch.manual_seed(1)
        r = am.posterior_importance(conf, S, keep_draws=True, keep_weights=True)
        theta, log_w = torch.as_tensor(r["draws"], device="cuda"), torch.as_tensor(r["log_w"], device="cuda")
        del r
        words = torch.from_numpy(A.resample_words(B, seed=2).view(np.int64)).cuda()
        assert A._resample_lib(theta, M, log_w) is not None, "the resampling kernel does not take these buffers"
        gate = A._resample_lib

        broad = torch.randn(B, S, dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(3))

        def fallback(**kw):
            A._resample_lib = lambda *x: None
            try:
                return A.resample_draws(theta, M, words=words, **kw)
            finally:
                A._resample_lib = gate

        got = A.resample_draws(theta, M, log_w=log_w, words=words, want_weights=True)
        W = got["weights"]
        ref, ref_lw = fallback(weights=W), fallback(log_w=log_w, want_weights=True)
        same = lambda x, y: bool(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y))   # noqa: E731
        out["results"] = {"kernel_equals_torch_on_the_kernels_weights": all(same(got[k], ref[k]) for k in ("draws", "ancestors", "n_unique", "n_positive")),
                          "weights_differing_from_torchs": int((W != ref_lw["weights"]).sum()),
                          "largest_weight_difference": int((W - ref_lw["weights"]).abs().max()),
                          "ancestors_differing_from_log_w_route": int((got["ancestors"] != ref_lw["ancestors"]).sum()),
                          "n_unique_median": float(got["n_unique"].double().median()), "n_positive_median": float(got["n_positive"].double().median()),
                          "sets_with_no_weight": int((got["n_positive"] == 0).sum())}
        got_b = A.resample_draws(theta, M, log_w=broad, words=words, want_weights=True)
        ref_b = fallback(weights=got_b["weights"])
        out["results_broad"] = {"kernel_equals_torch_on_the_kernels_weights": all(same(got_b[k], ref_b[k]) for k in ("draws", "ancestors", "n_unique", "n_positive")),
                                "n_unique_median": float(got_b["n_unique"].double().median()), "n_positive_median": float(got_b["n_positive"].double().median())}
        del got, ref, ref_lw, got_b, ref_b
        kernel = _time({"resample_kernel": lambda: A.resample_draws(theta, M, log_w=log_w, words=words),
                        "torch_evaluation": lambda: fallback(log_w=log_w),
                        "resample_kernel_weights": lambda: A.resample_draws(theta, M, weights=W, words=words),
                        "torch_evaluation_weights": lambda: fallback(weights=W),
                        "resample_kernel_broad": lambda: A.resample_draws(theta, M, log_w=broad, words=words),
                        "torch_evaluation_broad": lambda: fallback(log_w=broad)}, a.reps)
        calls = _time({"posterior_importance": lambda: am.posterior_importance(conf, S),
                       "posterior_importance_resample": lambda: am.posterior_importance(conf, S, resample=M),
                       "posterior_importance_smooth": lambda: am.posterior_importance(conf, S, smooth=True),
                       "posterior_importance_smooth_resample": lambda: am.posterior_importance(conf, S, smooth=True, resample=M)}, a.reps)
        out.update(workgroups=B, kernel_alone=kernel, whole_calls=calls,
                   torch_evaluation_over_resample_kernel=kernel["torch_evaluation"]["ms"] / kernel["resample_kernel"]["ms"],
                   torch_evaluation_over_resample_kernel_weights=kernel["torch_evaluation_weights"]["ms"] / kernel["resample_kernel_weights"]["ms"],
                   torch_evaluation_over_resample_kernel_broad=kernel["torch_evaluation_broad"]["ms"] / kernel["resample_kernel_broad"]["ms"],
                   resample_kernel_not_slower_than_torch=bool(kernel["resample_kernel"]["ms"] <= kernel["torch_evaluation"]["ms"]
                                                              and kernel["resample_kernel_broad"]["ms"] <= kernel["torch_evaluation_broad"]["ms"]
                                                              and kernel["resample_kernel_weights"]["ms"] <= kernel["torch_evaluation_weights"]["ms"]),
                   resample_over_default_call=calls["posterior_importance_resample"]["ms"] / calls["posterior_importance"]["ms"],
                   smooth_resample_over_smooth_call=calls["posterior_importance_smooth_resample"]["ms"] / calls["posterior_importance_smooth"]["ms"])
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
