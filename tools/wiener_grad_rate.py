#!/usr/bin/env python3
"""Rate of nddm_wiener_log_likelihood_grad (csrc/nddm_wiener_grad.h), the fused value-and-gradient kernel, at the shapes of
tools/wiener_rate.py, timed with HIP events beside the forward kernel (nddm_wiener_log_likelihood, sums only) at the same shapes and inputs
and beside PyTorch autograd -- forward plus backward -- through the composed formula (tools/wiener_rate.py: torch_logpdf), all in one run.
Prints one JSON line.

  grad_paired / fwd_paired                  basic_ddm_dc, 1M rows x 300 trials, each row against its own data set
  grad_broadcast / fwd_broadcast            500 data sets x 10 000 draws x 300 trials, basic_ddm_dc
  grad_broadcast_ans / fwd_broadcast_ans    the same for alpha_not_scaled (Eta in (0, 1.5))
  torch_autograd                            torch_logpdf(...).sum().backward() on 100 000 rows x 300 trials (basic, eta = 0); its gradient is
                                            compared with the kernel's on the first 1 000 rows

Every shape is warmed up (3 calls), then timed `--reps` times; the median is reported.  Each shape runs in a child process of its own under
`timeout` (a step that faults or hangs ends the tool; nothing further starts).
Usage: python tools/wiener_grad_rate.py [--json OUT] [--reps 20]        (one shape: --only NAME)
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wiener_rate as WR  # noqa: E402  (the shapes' inputs and the composed formula)

SHAPES = ("grad_paired", "fwd_paired", "grad_broadcast", "fwd_broadcast", "grad_broadcast_ans", "fwd_broadcast_ans", "torch_autograd")


def _time(torch, fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return WR._time(torch, fn, reps)


def run_one(name, reps):
    sys.path.insert(0, ROOT)
    import torch
    from bayesflow_nddms_amd import _lib, engine
    L = _lib.lib()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    st = lambda: torch.cuda.current_stream().cuda_stream
    N = 300
    res = {}
    if name == "torch_autograd":
        R = 100_000
        p, d = WR._basic_params(torch, R, gen), WR._data(torch, R, N, gen)
        k = engine.wiener_log_likelihood_grad(0, p[:1000], d[:1000])
        q = p[:1000].clone().requires_grad_(True)
        WR.torch_logpdf(torch, q, d[:1000]).sum(dtype=torch.float64).backward()
        ok = torch.isfinite(q.grad).all(1)                              # (autograd through torch.where gives NaN where the unselected series overflows)
        res["torch_grad_finite_row_fraction_first_1000_rows"] = ok.float().mean().item()
        res["max_abs_grad_diff_vs_kernel_over_max_abs_grad_first_1000_rows"] = ((q.grad.double() - k["grad"])[ok].abs().max() / k["grad"][ok].abs().max()).item()
        pg = p.clone().requires_grad_(True)

        def fn():
            pg.grad = None
            WR.torch_logpdf(torch, pg, d).sum(1, dtype=torch.float64).sum().backward()
        reps = min(reps, 5)
    else:
        D, S = (1_000_000, 1) if "paired" in name else (500, 10_000)
        R = D * S
        ans = name.endswith("_ans")
        p, model = WR._basic_params(torch, R, gen), 0
        if ans:
            eta = torch.rand(R, generator=gen, device="cuda") * 1.5
            p, model = torch.stack([p[:, 0], p[:, 1], p[:, 2], p[:, 3], eta, p[:, 4]], 1).contiguous(), engine.ALPHA_NOT_SCALED
        d = WR._data(torch, D, N, gen, signed=ans)
        out_s = torch.empty(R, dtype=torch.float64, device="cuda")
        if name.startswith("grad"):
            out_g = torch.empty((R, p.shape[1]), dtype=torch.float64, device="cuda")
            fn = lambda: _lib.check(L.nddm_wiener_log_likelihood_grad(model, p.data_ptr(), R, S, d.data_ptr(), N, 0, out_s.data_ptr(), out_g.data_ptr(), st()))
            fn()
            res["finite_fraction"] = torch.isfinite(out_g).all(1).float().mean().item()
        else:
            fn = lambda: _lib.check(L.nddm_wiener_log_likelihood(model, p.data_ptr(), R, S, d.data_ptr(), N, 0, None, out_s.data_ptr(), st()))
    evals = R * N
    med, best = _time(torch, fn, reps)
    print(json.dumps({"shape": name, "evals": evals, "reps": reps, "ms_median": round(med, 4), "ms_best": round(best, 4),
                      "evals_per_s": evals / (med * 1e-3), **res}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only")
    ap.add_argument("--json")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    if a.only:
        run_one(a.only, a.reps)
        return
    sys.path.insert(0, ROOT)
    from bayesflow_nddms_amd import build
    out = {"tool": "tools/wiener_grad_rate.py", "library_source_hash": build.source_hash(), "shapes": {}}
    for name in SHAPES:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--only", name, "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(f"{name}: exit status {r.returncode}; nothing further is started")
        out["shapes"][name] = json.loads(r.stdout.strip().splitlines()[-1])
    tc = out["shapes"]["torch_autograd"]["evals_per_s"]
    for name in ("grad_paired", "grad_broadcast", "grad_broadcast_ans"):
        s = out["shapes"][name]
        s["time_over_forward_kernel"] = s["ms_median"] / out["shapes"]["fwd" + name[4:]]["ms_median"]
        s["x_torch_autograd"] = s["evals_per_s"] / tc
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
