#!/usr/bin/env python3
"""Rate of nddm_wiener_marginal_log_likelihood_grad (csrc/nddm_wiener_marginal_grad.h) on the MI355X, timed with HIP events beside the forward
marginal kernel (nddm_wiener_marginal_log_likelihood, sums only) on the same rows and data in the same run.  Prints one JSON line.

  grad_paired / marginal_paired                 100 000 rows x 300 trials, each row against its own data set
  grad_broadcast / marginal_broadcast           100 data sets x 1 000 draws x 300 trials
  grad_paired_timeouts / marginal_paired_timeouts, grad_broadcast_timeouts / marginal_broadcast_timeouts
                                                the same with 10 % of every data set's trials timeouts (choicert 0, t_censor 4 s)

Rows and data are tools/wiener_marginal_rate.py's (its method: 3 warm-up calls, the median of `--reps` timed ones).  Per gradient shape:
trial gradients per second and the time over the forward marginal kernel's.  Each shape runs in a child process of its own under `timeout`
(a step that faults or hangs ends the tool; nothing further starts).
Usage: python tools/wiener_marginal_grad_rate.py [--json OUT] [--reps 20]        (one shape: --only NAME)
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wiener_rate as WR  # noqa: E402  (the shapes' inputs)

SHAPES = tuple(k + "_" + lay + suf for suf in ("", "_timeouts") for lay in ("paired", "broadcast") for k in ("grad", "marginal"))
TIMEOUT_FRACTION = 0.1


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
    u = lambda lo, hi: torch.rand(R, generator=gen, device="cuda") * (hi - lo) + lo
    pm = torch.stack([p[:, 0], p[:, 1], p[:, 2], p[:, 3], u(0.1, 0.5), p[:, 4], u(0.2, 1.0), torch.ones(R, device="cuda")], 1).contiguous()
    z = pm[::S, 1][:, None] + 0.3 * torch.randn((D, N), generator=gen, device="cuda")
    y = d[..., 0] * d[..., 1]
    if name.endswith("_timeouts"):
        y = torch.where(torch.rand((D, N), generator=gen, device="cuda") < TIMEOUT_FRACTION, torch.zeros_like(y), y)
    dm = torch.stack([y, z], -1).contiguous()
    out_s = torch.empty(R, dtype=torch.float64, device="cuda")
    out_g = torch.empty((R, 8), dtype=torch.float64, device="cuda")
    if name.startswith("grad"):
        fn = lambda: _lib.check(L.nddm_wiener_marginal_log_likelihood_grad(engine.SINGLE_TRIAL, pm.data_ptr(), R, S, dm.data_ptr(), N, 4.0, 0,
                                                                           out_s.data_ptr(), out_g.data_ptr(), st()))
    else:
        fn = lambda: _lib.check(L.nddm_wiener_marginal_log_likelihood(engine.SINGLE_TRIAL, pm.data_ptr(), R, S, dm.data_ptr(), N, 4.0, 0, None,
                                                                      out_s.data_ptr(), st()))
    fn()
    res = {"finite_fraction": torch.isfinite(out_s).float().mean().item(), "timeout_fraction": (y == 0).float().mean().item()}
    if name.startswith("grad"):
        res["finite_gradient_fraction"] = torch.isfinite(out_g).all(1).float().mean().item()
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
    out = {"tool": "tools/wiener_marginal_grad_rate.py", "library_source_hash": build.source_hash(), "timeout_fraction": TIMEOUT_FRACTION, "shapes": {}}
    for name in SHAPES:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--only", name, "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(f"{name}: exit status {r.returncode}; nothing further is started")
        out["shapes"][name] = json.loads(r.stdout.strip().splitlines()[-1])
    for name in SHAPES:
        if name.startswith("grad"):
            s, f = out["shapes"][name], out["shapes"]["marginal" + name[4:]]
            s["trial_gradients_per_s"] = s.pop("trials_per_s")
            s["time_over_forward_marginal_kernel"] = s["ms_median"] / f["ms_median"]
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
