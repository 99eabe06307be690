#!/usr/bin/env python3
"""Rate of nddm_wiener_log_likelihood (csrc/nddm_wiener.h) at the shapes of its users, timed with HIP events, beside the same formula
composed from PyTorch elementwise ops in the same process (the yardstick).  Prints one JSON line.

  paired_sums       basic_ddm_dc, 1M rows x 300 trials, each row against its own data set, sums only   (8 B of data per evaluation)
  paired_trials     the same with the per-trial output as well                                         (12 B per evaluation)
  broadcast_sums    500 data sets x 10 000 draws x 300 trials, sums only: the recovery loop's shape (basic_ddm_dc.py:211-223)
  broadcast_ans     the same for alpha_not_scaled (drift variability integrated out: one more v_rcp / v_log per evaluation)
  torch_composed    the fixed-trip formula of the kernel as PyTorch elementwise ops on 100 000 rows x 300 trials (basic, eta = 0)

With --cdf: nddm_wiener_cdf (csrc/nddm_wiener_cdf.h) instead, every shape writing its [R, 300] float32 output (8 + 4 B per evaluation):
  cdf_paired_eta0      basic_ddm_dc, 200 000 rows x 300 trials, each row against its own data set
  cdf_paired_eta       alpha_not_scaled with Eta in (0, 1.5): the large-time form's 16-node rule, the small-time form's closed one
  cdf_broadcast_eta0   100 data sets x 2 000 draws x 300 trials, basic_ddm_dc
  cdf_broadcast_eta    the same for alpha_not_scaled with Eta in (0, 1.5)
  cdf_torch_composed   the eta = 0 formula of the kernel as PyTorch elementwise ops (torch.special.erfcx) on 100 000 rows x 300 trials

With --quantile: nddm_wiener_quantile (csrc/nddm_wiener_quantile.h), the .1 / .3 / .5 / .7 / .9 quantiles of each boundary's own responses
(conditional, Q = 5 per boundary: 10 requests per row), beside what a user did before it existed -- a 32-step bisection of
engine.wiener_cdf from Python on the bit pattern of t (32 launches and one more for the limit P(boundary), on the paired layout: every row has its
own times):
  q_paired_eta0        basic_ddm_dc, 200 000 rows, each with its own request set
  q_paired_eta         alpha_not_scaled with Eta in (0, 1.5)
  q_broadcast_eta0     100 request sets x 2 000 draws, basic_ddm_dc
  q_broadcast_eta      the same for alpha_not_scaled with Eta in (0, 1.5)
  q_bisect_eta0        the composed bisection on q_paired_eta0's rows and requests
  q_bisect_eta         the composed bisection on q_paired_eta's rows and requests
Every kernel shape also reports the largest |wiener_cdf(q) - target| over its first 20 000 rows.

Each shape runs in a child process of its own under `timeout` (a step that faults or hangs ends the tool; nothing further starts).
Usage: python tools/wiener_rate.py [--cdf | --quantile] [--json OUT] [--reps 10]        (one shape: --only NAME)
"""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ("paired_sums", "paired_trials", "broadcast_sums", "broadcast_ans", "torch_composed")
CDF_SHAPES = ("cdf_paired_eta0", "cdf_paired_eta", "cdf_broadcast_eta0", "cdf_broadcast_eta", "cdf_torch_composed")
Q_SHAPES = ("q_paired_eta0", "q_paired_eta", "q_broadcast_eta0", "q_broadcast_eta", "q_bisect_eta0", "q_bisect_eta")
Q_PROBS = (.1, .3, .5, .7, .9)
HBM_BPS = 8e12


def _time(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], ms[0]


def _basic_params(torch, n, gen):
    u = lambda lo, hi: torch.rand(n, generator=gen, device="cuda") * (hi - lo) + lo
    return torch.stack([u(-3, 3), u(0.6, 2.0), u(0.3, 0.7), u(0.1, 0.5), u(0.8, 1.3)], 1).contiguous()


def _data(torch, D, N, gen, signed=False):
    rt = 0.5 + torch.rand((D, N), generator=gen, device="cuda") * 1.5
    ch = torch.where(torch.rand((D, N), generator=gen, device="cuda") < 0.6, 1.0, -1.0)
    if signed:
        return torch.stack([rt * ch, (ch + 1) / 2], -1).contiguous()
    return torch.stack([rt, ch], -1).contiguous()


def torch_logpdf(torch, p, d):
    """The kernel's formula (basic, eta = 0) from PyTorch elementwise ops: p [R, 5] against d [R, N, 2]."""
    v, a, beta, tau, s = (p[:, i:i + 1] for i in range(5))
    rt, ch = d[..., 0], d[..., 1]
    up = ch > 0
    ap, vp = a / s, v / s
    w = torch.where(up, 1 - beta, beta)
    nu = torch.where(up, -vp, vp)
    t = rt - tau
    u = t / (ap * ap)
    A, B = torch.exp(-2 * (1 - w) / u), torch.exp(-2 * (1 + w) / u)
    ss = w + (w - 2) * A + (w + 2) * B + (w - 4) * A ** 3 * B + (w + 4) * A * B ** 3
    small = -0.5 * math.log(2 * math.pi) - 1.5 * torch.log(u) - w * w / (2 * u) + torch.log(ss)
    q = torch.exp(-math.pi ** 2 * u / 2)
    c = torch.cos(math.pi * w)
    large = math.log(math.pi) + torch.log(torch.sin(math.pi * w)) - math.pi ** 2 * u / 2 + torch.log(1 + 4 * c * q ** 3 + 3 * (4 * c * c - 1) * q ** 8)
    lg = torch.where(u < 0.375, small, large)
    lf = lg - 2 * torch.log(ap) - ap * nu * w - nu * nu * t / 2
    return torch.where(t > 0, lf, torch.full_like(lf, -math.inf))


def torch_cdf(torch, p, d):
    """The kernel's distribution function (basic, eta = 0) from PyTorch elementwise ops: p [R, 5] against d [R, N, 2]."""
    v, a, beta, tau, s = (p[:, i:i + 1] for i in range(5))
    rt, ch = d[..., 0], d[..., 1]
    up = ch > 0
    ap, vp = a / s, v / s
    w = torch.where(up, 1 - beta, beta)
    nu = torch.where(up, -vp, vp)
    t = (rt - tau).clamp(min=1e-30)
    aw = ap * w
    d0 = -nu * aw - nu * nu * t / 2
    rs = torch.rsqrt(2 * t)
    small = torch.zeros_like(t)
    for j in range(4):
        r = ap * (j + 1 - w) if j & 1 else ap * (j + w)
        eg = torch.exp(d0 - r * r / (2 * t))
        xa, xb = (r - nu * t) * rs, (r + nu * t) * rs
        ta, tb = eg * torch.special.erfcx(xa.abs()), eg * torch.special.erfcx(xb.abs())
        term = torch.where(xa < 0, 2 * torch.exp(-(aw + r) * nu) - ta, ta) + torch.where(xb < 0, 2 * torch.exp(-(aw - r) * nu) - tb, tb)
        small = small - term / 2 if j & 1 else small + term / 2
    m = 2 * nu.abs() * ap
    ms = m.clamp(min=1e-6)
    ratio = torch.expm1(-ms * (1 - w)) / torch.expm1(-ms)
    P = torch.where(m < 1e-6, 1 - w, torch.where(nu > 0, torch.exp(-ms * w) * ratio, ratio))
    q = torch.exp(-math.pi ** 2 * t / (2 * ap * ap))
    lam = math.pi ** 2 / (ap * ap)
    tail = sum(k * torch.sin(k * math.pi * w) * q ** (k * k) / (nu * nu + k * k * lam) for k in range(1, 5))
    large = P - 2 * math.pi / (ap * ap) * torch.exp(d0) * tail
    F = torch.where(t < 0.375 * ap * ap, small, large)
    return torch.where(rt - tau > 0, torch.minimum(F.clamp(min=0), P), torch.zeros_like(F))


def run_cdf(name, reps):
    sys.path.insert(0, ROOT)
    import torch
    from bayesflow_nddms_amd import _lib, engine
    L = _lib.lib()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    st = lambda: torch.cuda.current_stream().cuda_stream
    N = 300
    ans = name.endswith("_eta")

    def params(R):
        b = _basic_params(torch, R, gen)
        if not ans:
            return b, 0
        eta = torch.rand(R, generator=gen, device="cuda") * 1.5
        return torch.stack([b[:, 0], b[:, 1], b[:, 2], b[:, 3], eta, b[:, 4]], 1).contiguous(), engine.ALPHA_NOT_SCALED

    res = {}
    if name == "cdf_torch_composed":
        R = 100_000
        p, d = _basic_params(torch, R, gen), _data(torch, R, N, gen)
        k = engine.wiener_cdf(0, p[:1000], d[:1000], want_p_upper=False)["cdf"]
        res["max_abs_diff_vs_kernel_first_1000_rows"] = (torch_cdf(torch, p[:1000], d[:1000]) - k).abs().max().item()
        fn = lambda: torch_cdf(torch, p, d)
    else:
        D, S = (200_000, 1) if "paired" in name else (100, 2_000)
        R = D * S
        (p, model), d = params(R), _data(torch, D, N, gen, signed=ans)
        out = torch.empty((R, N), dtype=torch.float32, device="cuda")
        fn = lambda: _lib.check(L.nddm_wiener_cdf(model, p.data_ptr(), R, S, d.data_ptr(), N, 0, out.data_ptr(), None, st()))
        res["small_time_fraction"] = ((d[..., 0].abs()[:, None, :] - p.reshape(D, S, -1)[..., 3:4])
                                      < 0.375 * (p.reshape(D, S, -1)[..., 1:2] / p.reshape(D, S, -1)[..., -1:]) ** 2)[:, :8].float().mean().item()
    evals = R * N
    nbytes = d.numel() * 4 + p.numel() * 4 + evals * 4
    med, best = _time(torch, fn, reps)
    res = {"shape": name, "evals": evals, "ms_median": round(med, 4), "ms_best": round(best, 4), "evals_per_s": evals / (med * 1e-3),
           "GB_per_s": nbytes / (med * 1e-3) / 1e9, "frac_of_8TBps": nbytes / (med * 1e-3) / HBM_BPS, **res}
    print(json.dumps(res), flush=True)


def _signed_data(torch, model, rt, code):
    """Response times and boundary codes [R, n] as trials of the model's format [R, n, 2]."""
    if model == 0:
        return torch.stack([rt, code], -1).contiguous()
    return torch.stack([rt * code, (code + 1) / 2], -1).contiguous()


def bisect_quantile(torch, engine, model, p, req, steps=32):
    """What a user does without the kernel: conditional quantiles by `steps` bisections of engine.wiener_cdf on the bit pattern of t
    between 0 and 1e15 (positive floats order as their integers: it ends on adjacent floats).  p [R, P], req [R, n, 2] -> rt [R, n]."""
    R, n = req.shape[0], req.shape[1]
    code, tau = req[..., 1], p[:, 3:4]
    inf = torch.full((R, n), float("inf"), device=p.device)
    target = req[..., 0] * engine.wiener_cdf(model, p, _signed_data(torch, model, inf, code), want_p_upper=False)["cdf"]
    lo = torch.zeros((R, n), dtype=torch.int32, device=p.device)
    hi = torch.full((R, n), 1.0e15, dtype=torch.float32, device=p.device).view(torch.int32)
    for _ in range(steps):
        mid = lo + (hi - lo) // 2
        F = engine.wiener_cdf(model, p, _signed_data(torch, model, tau + mid.view(torch.float32), code), want_p_upper=False)["cdf"]
        below = F < target
        lo, hi = torch.where(below, mid, lo), torch.where(below, hi, mid)
    return tau + hi.view(torch.float32)


def run_quantile(name, reps):
    sys.path.insert(0, ROOT)
    import torch
    from bayesflow_nddms_amd import _lib, engine
    L = _lib.lib()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    st = lambda: torch.cuda.current_stream().cuda_stream
    ans = name.endswith("_eta")
    Q = len(Q_PROBS)
    n = 2 * Q
    D, S = (100, 2_000) if "broadcast" in name else (200_000, 1)
    R = D * S
    b = _basic_params(torch, R, gen)
    if ans:
        eta = torch.rand(R, generator=gen, device="cuda") * 1.5
        p, model = torch.stack([b[:, 0], b[:, 1], b[:, 2], b[:, 3], eta, b[:, 4]], 1).contiguous(), engine.ALPHA_NOT_SCALED
    else:
        p, model = b, 0
    pr = torch.tensor(Q_PROBS + Q_PROBS, device="cuda")
    code = torch.tensor([-1.0] * Q + [1.0] * Q, device="cuda")
    req = torch.stack([pr, code], -1)[None].repeat(D, 1, 1).contiguous()
    res = {}
    if "bisect" in name:
        fn = lambda: bisect_quantile(torch, engine, model, p, req)
        k = engine.wiener_quantile(model, p[:20_000], req[:20_000], conditional=True)["quantile"]
        d = (bisect_quantile(torch, engine, model, p[:20_000], req[:20_000]) - k).abs()
        res["max_abs_rt_diff_vs_kernel_first_20000_rows"] = d[torch.isfinite(d)].max().item()
    else:
        out = torch.empty((R, n), dtype=torch.float32, device="cuda")
        fn = lambda: _lib.check(L.nddm_wiener_quantile(model, p.data_ptr(), R, S, req.data_ptr(), n, _lib.QUANTILE_CONDITIONAL, out.data_ptr(), st()))
        fn()
        m = min(R, 20_000)
        pm, qm = p[:m], out[:m]
        cm = code[None].expand(m, n)
        inf = torch.full((m, n), float("inf"), device="cuda")
        lim = engine.wiener_cdf(model, pm, _signed_data(torch, model, inf, cm), want_p_upper=False)["cdf"]
        F = engine.wiener_cdf(model, pm, _signed_data(torch, model, qm, cm), want_p_upper=False)["cdf"]
        res["finite_fraction_first_rows"] = torch.isfinite(qm).float().mean().item()
        res["max_abs_cdf_residual_first_rows"] = (F - pr[None] * lim)[torch.isfinite(qm)].abs().max().item()
    evals = R * n
    med, best = _time(torch, fn, reps)
    res = {"shape": name, "requests": evals, "ms_median": round(med, 4), "ms_best": round(best, 4), "requests_per_s": evals / (med * 1e-3), **res}
    print(json.dumps(res), flush=True)


def run_one(name, reps):
    if name in CDF_SHAPES:
        return run_cdf(name, reps)
    if name in Q_SHAPES:
        return run_quantile(name, reps)
    sys.path.insert(0, ROOT)
    import torch
    from bayesflow_nddms_amd import _lib, engine
    L = _lib.lib()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    st = lambda: torch.cuda.current_stream().cuda_stream
    N = 300
    if name in ("paired_sums", "paired_trials"):
        R = 1_000_000
        p, d = _basic_params(torch, R, gen), _data(torch, R, N, gen)
        out_s = torch.empty(R, dtype=torch.float64, device="cuda")
        out_t = torch.empty((R, N), dtype=torch.float32, device="cuda") if name == "paired_trials" else None
        fn = lambda: _lib.check(L.nddm_wiener_log_likelihood(0, p.data_ptr(), R, 1, d.data_ptr(), N, 0,
                                                             None if out_t is None else out_t.data_ptr(), out_s.data_ptr(), st()))
        nbytes = d.numel() * 4 + p.numel() * 4 + R * 8 + (R * N * 4 if out_t is not None else 0)
        evals = R * N
    elif name in ("broadcast_sums", "broadcast_ans"):
        D, S = 500, 10_000
        R = D * S
        if name == "broadcast_sums":
            p, model = _basic_params(torch, R, gen), 0
        else:
            b = _basic_params(torch, R, gen)
            eta = torch.rand(R, generator=gen, device="cuda") * 1.5
            p, model = torch.stack([b[:, 0], b[:, 1], b[:, 2], b[:, 3], eta, b[:, 4]], 1).contiguous(), engine.ALPHA_NOT_SCALED
        d = _data(torch, D, N, gen, signed=name == "broadcast_ans")
        out_s = torch.empty(R, dtype=torch.float64, device="cuda")
        fn = lambda: _lib.check(L.nddm_wiener_log_likelihood(model, p.data_ptr(), R, S, d.data_ptr(), N, 0, None, out_s.data_ptr(), st()))
        nbytes = d.numel() * 4 + p.numel() * 4 + R * 8
        evals = R * N
    else:
        R = 100_000
        p = _basic_params(torch, R, gen)
        d = _data(torch, R, N, gen)
        # the same values as the kernel, to the tolerance of f32 (a check that the yardstick computes the same thing)
        k = engine.wiener_log_likelihood(0, p[:1000], d[:1000], per_trial=True)["trial_logp"]
        dev = (torch_logpdf(torch, p[:1000], d[:1000]) - k).abs().max().item()
        fn = lambda: torch_logpdf(torch, p, d).sum(1, dtype=torch.float64)
        nbytes = d.numel() * 4 + p.numel() * 4 + R * 8
        evals = R * N
    med, best = _time(torch, fn, reps)
    res = {"shape": name, "evals": evals, "ms_median": round(med, 4), "ms_best": round(best, 4),
           "evals_per_s": evals / (med * 1e-3), "GB_per_s": nbytes / (med * 1e-3) / 1e9, "frac_of_8TBps": nbytes / (med * 1e-3) / HBM_BPS}
    if name == "torch_composed":
        res["max_abs_diff_vs_kernel_first_1000_rows"] = dev
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only")
    ap.add_argument("--cdf", action="store_true", help="the shapes of nddm_wiener_cdf instead of the log-likelihood's")
    ap.add_argument("--quantile", action="store_true", help="the shapes of nddm_wiener_quantile, beside a composed bisection of wiener_cdf")
    ap.add_argument("--json")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    if a.only:
        run_one(a.only, a.reps)
        return
    sys.path.insert(0, ROOT)
    from bayesflow_nddms_amd import build
    out = {"tool": "tools/wiener_rate.py", "library_source_hash": build.source_hash(), "shapes": {}}
    for name in (Q_SHAPES if a.quantile else CDF_SHAPES if a.cdf else SHAPES):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--only", name, "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(f"{name}: exit status {r.returncode}; nothing further is started")
        out["shapes"][name] = json.loads(r.stdout.strip().splitlines()[-1])
    if a.quantile:                              # each kernel shape against the composed bisection of the same model
        for name in Q_SHAPES[:4]:
            yard = out["shapes"]["q_bisect_eta" if name.endswith("_eta") else "q_bisect_eta0"]["requests_per_s"]
            out["shapes"][name]["x_composed_bisection"] = out["shapes"][name]["requests_per_s"] / yard
    else:
        yard = "cdf_torch_composed" if a.cdf else "torch_composed"
        tc = out["shapes"][yard]["evals_per_s"]
        for name in (CDF_SHAPES[:-1] if a.cdf else ("broadcast_sums", "broadcast_ans", "paired_sums")):
            out["shapes"][name]["x_torch_composed"] = out["shapes"][name]["evals_per_s"] / tc
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
