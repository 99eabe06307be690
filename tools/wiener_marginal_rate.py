#!/usr/bin/env python3
"""Rate of nddm_wiener_marginal_log_likelihood (csrc/nddm_wiener_marginal.h) on the MI355X, timed with HIP events beside the forward kernel
(nddm_wiener_log_likelihood, basic_ddm_dc, sums only) on rows of the same shape in the same run.  Prints one JSON line.

  marginal_paired / fwd_paired              100 000 rows x 300 trials, each row against its own data set
  marginal_broadcast / fwd_broadcast        100 data sets x 1 000 draws x 300 trials

The marginal's rows are the forward rows' (drift, boundary -> mu_alpha, beta, tau -> ter, dc) with std_alpha in [0.1, 0.5], sigma1 in [0.2, 1]
and gamma = 1; its data the forward data's response times with z1 = mu_alpha + N(0, 0.3^2) per trial; no timeouts (the censored branch is
the rare one).  Every shape is warmed up (3 calls), then timed `--reps` times; the median is reported.  Per shape: trial marginals per
second, and the time per NODE evaluation (WMARG_PASSES x WMARG_K = 96 per trial) over the forward kernel's time per trial -- the price of a
node in units of one forward evaluation.  Each shape runs in a child process of its own under `timeout` (a step that faults or hangs ends
the tool; nothing further starts).
Usage: python tools/wiener_marginal_rate.py [--json OUT] [--reps 20]        (one shape: --only NAME)
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wiener_rate as WR  # noqa: E402  (the shapes' inputs)

SHAPES = ("marginal_paired", "fwd_paired", "marginal_broadcast", "fwd_broadcast")
NODES_PER_TRIAL = 96


def run_one(name, reps):
    sys.path.insert(0, ROOT)
    import torch
    from bayesflow_nddms_amd import _lib, engine
    L = _lib.lib()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    st = lambda: torch.cuda.current_stream().cuda_stream
    N = 300
    D, S = (100_000, 1) if "paired" in name else (100, 1_000)
    R = D * S
    p, d = WR._basic_params(torch, R, gen), WR._data(torch, D, N, gen)
    out_s = torch.empty(R, dtype=torch.float64, device="cuda")
    res = {}
    if name.startswith("marginal"):
        u = lambda lo, hi: torch.rand(R, generator=gen, device="cuda") * (hi - lo) + lo
        pm = torch.stack([p[:, 0], p[:, 1], p[:, 2], p[:, 3], u(0.1, 0.5), p[:, 4], u(0.2, 1.0), torch.ones(R, device="cuda")], 1).contiguous()
        mu_set = pm[::S, 1]
        z = mu_set[:, None] + 0.3 * torch.randn((D, N), generator=gen, device="cuda")
        dm = torch.stack([d[..., 0] * d[..., 1], z], -1).contiguous()
        fn = lambda: _lib.check(L.nddm_wiener_marginal_log_likelihood(engine.SINGLE_TRIAL, pm.data_ptr(), R, S, dm.data_ptr(), N, 4.0, 0, None,
                                                                      out_s.data_ptr(), st()))
        fn()
        res["finite_fraction"] = torch.isfinite(out_s).float().mean().item()
    else:
        fn = lambda: _lib.check(L.nddm_wiener_log_likelihood(0, p.data_ptr(), R, S, d.data_ptr(), N, 0, None, out_s.data_ptr(), st()))
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    med, best = WR._time(torch, fn, reps)
    print(json.dumps({"shape": name, "trials": R * N, "reps": reps, "ms_median": round(med, 4), "ms_best": round(best, 4),
                      "trials_per_s": R * N / (med * 1e-3), **res}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only")
    ap.add_argument("--json")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=240)
    a = ap.parse_args()
    if a.only:
        run_one(a.only, a.reps)
        return
    sys.path.insert(0, ROOT)
    from bayesflow_nddms_amd import build
    out = {"tool": "tools/wiener_marginal_rate.py", "library_source_hash": build.source_hash(), "nodes_per_trial": NODES_PER_TRIAL, "shapes": {}}
    for name in SHAPES:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--only", name, "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(f"{name}: exit status {r.returncode}; nothing further is started")
        out["shapes"][name] = json.loads(r.stdout.strip().splitlines()[-1])
    for name in ("marginal_paired", "marginal_broadcast"):
        s, f = out["shapes"][name], out["shapes"]["fwd" + name[8:]]
        s["time_over_forward_kernel"] = s["ms_median"] / f["ms_median"]
        s["node_time_over_forward_evaluation"] = s["time_over_forward_kernel"] / NODES_PER_TRIAL
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
