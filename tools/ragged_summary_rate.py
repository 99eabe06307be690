#!/usr/bin/env python3
"""Rate of ONE amortizer call on participants of different trial counts (amortizer.observed_batch, the summary network's inference
kernels: csrc/train_deepset.hip, nddm_deepset_summary) beside the loop it replaces, all legs on the SAME commit: 100 basic_ddm_dc data
sets whose trial counts are drawn once, under a fixed seed, uniformly from 60 to 300, and 1000 posterior draws of each, from the default
networks.  Legs, each the whole public call(s):
    loop_sample             the reference's participant loop (fitting_stahl_data.py:196-211): 100 x sample(configurator(one set), 1000)
    loop_sample_fused       the same loop with sample(..., fused=True)
    ragged_sample_fused     sample(observed_batch(all sets), 1000, fused=True): one call
and the summary step alone, the kernels (InvariantNetwork.summarize) against the PyTorch definition (forward(x, counts=...) under
no_grad), at B = 100 ragged and at B = 1 x 300 trials.
Timing: device events around each leg after a warm-up of every leg, the legs ALTERNATING, the median of --reps (>= 20) per leg.  The
ragged call's draws are compared with the loop's conditions fed the same base normals.

Usage: python tools/ragged_summary_rate.py [--json profiles/r32_ragged_summary_rate.json] [--reps 20]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS, DRAWS, N_MIN, N_MAX = 100, 1000, 60, 300


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    import torch
    from bayesflow_nddms_amd import basic_ddm_dc, engine
    from bayesflow_nddms_amd.amortizer import AmortizedPosterior, InvariantNetwork, InvertibleNetwork, observed_batch
    engine.require_device()
    torch.manual_seed(0)
    rng = np.random.default_rng(2023)
    P = 5
    am = AmortizedPosterior(InvertibleNetwork(num_params=P), InvariantNetwork()).cuda().eval()
    net = am.summary_net
    counts = rng.integers(N_MIN, N_MAX + 1, SETS)
    theta = np.stack([rng.normal(0.5, 1.0, SETS), rng.uniform(0.9, 1.6, SETS), rng.uniform(0.4, 0.6, SETS), rng.uniform(0.2, 0.4, SETS),
                      rng.uniform(0.8, 1.2, SETS)], axis=1).astype(np.float32)
    sim = basic_ddm_dc.batch_simulate_trials(theta, N_MAX, seed=2023, set_offset=0, with_summary=False)["sim_data"]
    sets = [np.asarray(sim[b, :n], dtype=np.float32) for b, n in enumerate(counts)]
    ob = observed_batch(sets, device="cuda")
    # the loop's inputs, configured once (as the reference's loop configures each participant before its call): device tensors
    confs = [basic_ddm_dc.configurator({"sim_data": torch.as_tensor(s, device="cuda")[None], "sim_non_batchable_context": len(s),
                                        "prior_draws": np.zeros((1, P), np.float32)}) for s in sets]
    x, cnt = ob["summary_conditions"], ob["summary_counts"]
    one = torch.as_tensor(np.asarray(sim[:1], dtype=np.float32), device="cuda").contiguous()          # one set of all N_MAX simulated trials
    with torch.no_grad():
        assert net._summary_lib(x, ob["direct_conditions"]) is not None, "the inference kernels do not cover this network"

    def loop(fused):
        return [am.sample(c, DRAWS, to_numpy=False, fused=fused) for c in confs]

    def plain_summary(xx, c):
        with torch.no_grad():
            return net(xx, counts=c) if c is not None else net(xx)

    legs = {"loop_sample": lambda: loop(False), "loop_sample_fused": lambda: loop(True),
            "ragged_sample_fused": lambda: am.sample(ob, DRAWS, to_numpy=False, fused=True),
            "summary_kernels_B100_ragged": lambda: net.summarize(x, cnt), "summary_pytorch_B100_ragged": lambda: plain_summary(x, cnt),
            "summary_kernels_B1_x_%d" % one.shape[1]: lambda: net.summarize(one), "summary_pytorch_B1_x_%d" % one.shape[1]: lambda: plain_summary(one, None)}
    # the ragged call's draws against the loop's conditions fed the same base normals
    torch.manual_seed(1)
    ragged = legs["ragged_sample_fused"]()
    torch.manual_seed(1)
    z = torch.randn(SETS * DRAWS, P, device="cuda").view(SETS, DRAWS, P)
    with torch.no_grad():
        cond = torch.cat([am._conditions(c) for c in confs])
        want = am.inference_net.inverse_per_set(z, cond)
        agree = {"max_abs_difference_of_draws_over_max_abs_draw": float((ragged - want).abs().max() / want.abs().max()),
                 "max_abs_difference_of_conditions": float((am._conditions(ob) - cond).abs().max())}
    del ragged, want, z
    for fn in legs.values():                                  # warm-up of every leg at the timed shape
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(a.reps):                                   # alternating
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    out = {"tool": "tools/ragged_summary_rate.py", "device": torch.cuda.get_device_name(0), "sets": SETS, "draws_per_set": DRAWS,
           "trial_counts": {"min": int(counts.min()), "max": int(counts.max()), "sum": int(counts.sum()), "seed": 2023}, "reps": a.reps,
           "timing": "device events around the whole leg, legs alternating, median", "results": agree,
           "legs": {k: {"ms": float(np.median(v)), "ms_min": float(min(v)), "ms_max": float(max(v))} for k, v in ms.items()}}
    t = {k: v["ms"] for k, v in out["legs"].items()}
    n1 = one.shape[1]
    out["speedup_ragged_call_over_loop"] = t["loop_sample"] / t["ragged_sample_fused"]
    out["speedup_ragged_call_over_fused_loop"] = t["loop_sample_fused"] / t["ragged_sample_fused"]
    out["speedup_summary_kernels_over_pytorch_B100_ragged"] = t["summary_pytorch_B100_ragged"] / t["summary_kernels_B100_ragged"]
    out["speedup_summary_kernels_over_pytorch_B1"] = t["summary_pytorch_B1_x_%d" % n1] / t["summary_kernels_B1_x_%d" % n1]
    out["ragged_call_not_slower_than_the_loop"] = bool(t["ragged_sample_fused"] <= min(t["loop_sample"], t["loop_sample_fused"]))
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
