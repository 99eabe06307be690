#!/usr/bin/env python3
"""Price of the weighted posterior quantiles (csrc/train_wquantile.hip, amortizer.weighted_draw_quantiles /
posterior_importance(probs=...)) at the reference's recovery shape, B = 500 data sets x S = 10 000 draws x D = 5: the default network
(6 coupling layers, D = 5 parameters, C = 11 conditions) on basic_ddm_dc data sets of 180 trials.  Two groups of legs:
  the kernel alone, on one buffer of fused draws [B, S, 5] and that call's own log weights [B, S]
    weighted_kernel_log_w        the five default probabilities from log weights (one launch: B x 5 workgroups, a max sweep, a full
                                 LDS sort of 8-byte items, the weights recomputed in sorted order)
    weighted_kernel_weights      the same from integer weights passed in
    torch_fallback_log_w         the PyTorch evaluation of the same definition on the same device tensors (the gate patched off)
    torch_fallback_weights       the same from integer weights
    weighted_kernel_broad / torch_fallback_broad   the same two routes on the same draws with log weights ~ N(0, 1): EVERY row inside
                                 (an untrained flow's own weights leave a handful of rows: a sort of padding, a scan of nothing)
    draw_quantiles_kernel        the UNWEIGHTED kernel on the same draws: 4-byte keys, half the LDS traffic (reported, not gated)
  whole public calls
    posterior_importance         probs=None: the parent's call
    posterior_importance_probs   probs = the five default probabilities
--control: only the first public leg, through calls the parent commit has as well; with --root it imports the package from another
checkout (the parent's, built): the control for "the default path is unchanged".
Timing: device events around each leg after a warm-up of every leg, the legs of a group ALTERNATING in one process, the median of
--reps (>= 20) per leg.  The kernel's answer is compared with the PyTorch evaluation at the timed size (bit for bit, on the kernel's
own integer weights).

Usage: python tools/flow_wquantile_rate.py [--json profiles/r33_flow_wquantile_rate.json] [--reps 20] [--control [--root DIR]]
"""
import argparse
import json
import os
import sys

import numpy as np

B, S, N_TRIALS = 500, 10_000, 180
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
    out = {"tool": "tools/flow_wquantile_rate.py", "package": os.path.dirname(os.path.abspath(A.__file__)), "device": torch.cuda.get_device_name(0),
           "network": {"layers": 6, "D": P, "C": 11, "hidden": 128}, "B": B, "S": S, "n_trials": N_TRIALS, "probs": list(PROBS), "reps": a.reps,
           "timing": "device events around each leg, legs of a group alternating, median"}
    if a.control:
        out["whole_calls"] = _time({"posterior_importance": lambda: am.posterior_importance(conf, S)}, a.reps)
    else:
        torch.manual_seed(1)
        r = am.posterior_importance(conf, S, keep_draws=True, keep_weights=True)
        theta, log_w = torch.as_tensor(r["draws"], device="cuda"), torch.as_tensor(r["log_w"], device="cuda")
        del r
        assert A._wquantile_lib(theta, len(PROBS), log_w) is not None, "the weighted selection kernel does not take these buffers"
        gate = A._wquantile_lib

        def fallback(**kw):
            A._wquantile_lib = lambda *x: None
            try:
                return A.weighted_draw_quantiles(theta, PROBS, **kw)
            finally:
                A._wquantile_lib = gate

        got = A.weighted_draw_quantiles(theta, PROBS, log_w=log_w, want_weights=True)
        W = got["weights"]
        ref, given = fallback(weights=W), A.weighted_draw_quantiles(theta, PROBS, weights=W)
        same = lambda x, y: bool(torch.equal(x.view(torch.int64), y.view(torch.int64)))      # noqa: E731
        out["results"] = {"kernel_equals_torch_on_its_own_weights_bit_for_bit": same(got["quantiles"], ref["quantiles"]),
                          "kernel_from_weights_equals_kernel_from_log_w": same(got["quantiles"], given["quantiles"]),
                          "max_abs_weight_difference_kernel_torch": int((W - A.quantize_weights(log_w)).abs().max()),
                          "n_positive_median": float(got["n_positive"].double().median()), "sets_without_a_positive_weight": int((got["n_positive"] == 0).sum())}
        del got, ref, given
        broad = torch.randn(B, S, dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
        nb = A.weighted_draw_quantiles(theta, PROBS, log_w=broad, want_weights=True)
        out["results"]["broad_n_positive_median"] = float(nb["n_positive"].double().median())
        out["results"]["broad_kernel_equals_torch_on_its_own_weights_bit_for_bit"] = same(nb["quantiles"], fallback(weights=nb["weights"])["quantiles"])
        del nb
        kernel = _time({"weighted_kernel_log_w": lambda: A.weighted_draw_quantiles(theta, PROBS, log_w=log_w),
                        "weighted_kernel_weights": lambda: A.weighted_draw_quantiles(theta, PROBS, weights=W),
                        "torch_fallback_log_w": lambda: fallback(log_w=log_w),
                        "torch_fallback_weights": lambda: fallback(weights=W),
                        "weighted_kernel_broad": lambda: A.weighted_draw_quantiles(theta, PROBS, log_w=broad),
                        "torch_fallback_broad": lambda: fallback(log_w=broad),
                        "draw_quantiles_kernel": lambda: A.draw_quantiles(theta, PROBS)}, a.reps)
        calls = _time({"posterior_importance": lambda: am.posterior_importance(conf, S),
                       "posterior_importance_probs": lambda: am.posterior_importance(conf, S, probs=PROBS)}, a.reps)
        out.update(workgroups=B * P, kernel_alone=kernel, whole_calls=calls,
                   torch_fallback_over_weighted_kernel=kernel["torch_fallback_log_w"]["ms"] / kernel["weighted_kernel_log_w"]["ms"],
                   weighted_kernel_not_slower_than_torch=kernel["weighted_kernel_log_w"]["ms"] <= kernel["torch_fallback_log_w"]["ms"],
                   torch_fallback_over_weighted_kernel_broad=kernel["torch_fallback_broad"]["ms"] / kernel["weighted_kernel_broad"]["ms"],
                   weighted_broad_over_unweighted_kernel=kernel["weighted_kernel_broad"]["ms"] / kernel["draw_quantiles_kernel"]["ms"],
                   weighted_over_unweighted_kernel=kernel["weighted_kernel_log_w"]["ms"] / kernel["draw_quantiles_kernel"]["ms"],
                   probs_over_default_call=calls["posterior_importance_probs"]["ms"] / calls["posterior_importance"]["ms"])
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
