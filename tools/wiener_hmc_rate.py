#!/usr/bin/env python3
"""Rate of the batched HMC sampler (nddm_wiener_hmc; csrc/nddm_wiener_hmc.h) at the shape of the reference's fit -- 100 participants x 6
chains = 600 chains x 100 trials, 16 leapfrog steps (basic_ddm_dc_pyjags.py) -- beside the route the library offered before it: the SAME
algorithm (the same coordinates, priors, jittered step, leapfrog and accept rule) as a PyTorch loop over likelihood.wiener_loglik with all
600 chains batched, one gradient launch per leapfrog step plus PyTorch's elementwise ops around it.  Both run in this process, alternating,
after a warm-up of each; the figure of each is the MEDIAN of three timed runs (a host clock around work that ends in a device synchronise).

Prints one JSON line: seconds per iteration of both, their ratio, the device loop's time per leapfrog step and per trial round (64 trials of
one chain), leapfrog x trials per second, the time of one full bounded launch (WHMC_MAX_ROUNDS rounds), and the projected wall time of the
reference's 2000 + 10 000 iterations cut into bounded launches.

Usage: python tools/wiener_hmc_rate.py [--json OUT] [--iters 8000] [--baseline-iters 60]
       python tools/wiener_hmc_rate.py --censored [--unflagged-only] [--json OUT] [--iters 4000]
--censored: NDDM_WIENER_CENSORED's cost at the same shape -- seconds per iteration of the unflagged entry, of the flagged entry on the same
data (0 % timeouts) and on data with 3 % timeouts, and the gradient kernel at 100 000 rows x 300 trials unflagged, flagged with 0 % and with
10 % timeouts; every figure the median of three alternating runs.  --unflagged-only: the unflagged legs alone (what a library from before
the flag can run: point NDDM_HIP_LIB at it to compare the two in one session).
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

D, CHAINS, N, LEAPFROG = 100, 6, 100, 16
EPS = 0.05


def torch_hmc(torch, engine, likelihood, data, q, T, n_iter, eps, gen):
    """n_iter iterations of the kernel's algorithm for all chains at once in PyTorch float64: unit mass, all five columns free, one
    likelihood.wiener_loglik launch (value and gradient) per leapfrog step -> (q, the mean acceptance probability)."""
    C = q.shape[0]
    lo = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.05], dtype=torch.float64, device=q.device)
    wd = torch.stack([torch.ones_like(T), torch.full_like(T, 10.0), torch.ones_like(T), T, torch.full_like(T, 9.95)], 1)

    def log_post(x):
        sg = torch.sigmoid(x)
        th = torch.cat([x[:, :1], lo[1:] + wd[:, 1:] * sg[:, 1:]], 1).detach().requires_grad_(True)
        ll = likelihood.wiener_loglik(engine.BASIC_DDM_DC, th, data, draws_per_dataset=CHAINS)
        (gl,) = torch.autograd.grad(ll.sum(), th)
        v, a, b, ta, s = th.detach().unbind(1)
        lp = ll.detach() - 0.125 * v * v - 2.0 * (a - 1.0) ** 2 + torch.log(b) + torch.log1p(-b) - 8.0 * (ta - 0.5) ** 2 - 2.0 * (s - 1.0) ** 2
        gl = gl + torch.stack([-0.25 * v, -4.0 * (a - 1.0), 1.0 / b - 1.0 / (1.0 - b), -16.0 * (ta - 0.5), -4.0 * (s - 1.0)], 1)
        jac = wd[:, 1:] * sg[:, 1:] * (1.0 - sg[:, 1:])
        lp = lp + (torch.log(wd[:, 1:]) + torch.nn.functional.logsigmoid(x[:, 1:]) + torch.nn.functional.logsigmoid(-x[:, 1:])).sum(1)
        return lp, torch.cat([gl[:, :1], gl[:, 1:] * jac + (1.0 - 2.0 * sg[:, 1:])], 1)
    lp, g = log_post(q)
    acc = torch.zeros((), dtype=torch.float64, device=q.device)
    for _ in range(n_iter):
        p = torch.randn(C, 5, dtype=torch.float64, device=q.device, generator=gen)
        u = torch.rand(C, 2, dtype=torch.float64, device=q.device, generator=gen)
        e = (eps * (0.8 + 0.2 * u[:, 0]))[:, None]
        H0 = -lp + 0.5 * (p * p).sum(1)
        qn, gn = q, g
        for _ in range(LEAPFROG):
            p = p + 0.5 * e * gn
            qn = qn + e * p
            lpn, gn = log_post(qn)
            p = p + 0.5 * e * gn
        d = H0 - (-lpn + 0.5 * (p * p).sum(1))
        ok = torch.isfinite(d) & (d > -1000.0)
        take = ok & (torch.log(u[:, 1]) < d)
        acc = acc + torch.where(ok, torch.exp(d.clamp(max=0.0)), torch.zeros_like(d)).mean()
        q = torch.where(take[:, None], qn, q)
        g = torch.where(take[:, None], gn, g)
        lp = torch.where(take, lpn, lp)
    return q, acc / n_iter


def censored_legs(a):
    import torch
    import wiener_hmc_host as H
    from bayesflow_nddms_amd import engine, mcmc
    engine.require_device()
    dev = torch.device("cuda")
    iters = min(a.iters, 4000)
    data_np = H.example_data(D, N, 41)
    with3 = H.censor(data_np, share=0.03)
    legs = {"unflagged": (data_np, False)}
    if not a.unflagged_only:
        legs.update({"flagged_0pct_timeouts": (data_np, True), "flagged_3pct_timeouts": (with3, True)})
    kw = dict(chains_per_dataset=CHAINS, n_leapfrog=LEAPFROG, seed=3)
    runs = {}
    for name, (d_np, cens) in legs.items():
        ck = {"censored": True} if cens else {}
        theta = mcmc.hmc_init(d_np, CHAINS, 1, **ck).reshape(-1, 5)
        st = torch.as_tensor(mcmc.make_state(theta, np.repeat(d_np, CHAINS, 0), eps0=EPS, **ck)).to(dev)
        d = torch.as_tensor(d_np).to(dev)
        engine.wiener_hmc(engine.BASIC_DDM_DC, d, st, n_iter=300, n_adapt=300, want_draws=False, want_log_post=False, **kw, **ck)
        torch.cuda.synchronize()

        def loop(d=d, st=st, ck=ck):
            r = engine.wiener_hmc(engine.BASIC_DDM_DC, d, st.clone(), n_iter=iters, n_adapt=0, iter_offset=300, thin=10, **kw, **ck)
            return float(r["accept"].mean()), int(r["flagged"].sum())
        runs[name] = loop
    # the gradient kernel: 100 000 rows x 300 trials, paired layout
    R_, N_ = 100_000, 300
    rng = np.random.default_rng(7)
    p = torch.as_tensor(np.stack([rng.uniform(-1, 1, R_), rng.uniform(1.2, 1.8, R_), rng.uniform(0.2, 0.8, R_), rng.uniform(0.2, 0.22, R_),
                                  rng.uniform(0.9, 1.1, R_)], 1).astype(np.float32)).to(dev)
    rt = torch.rand(R_, N_, device=dev) * 1.65 + 0.35
    ch = torch.where(torch.rand(R_, N_, device=dev) < 0.5, 1.0, -1.0)
    g0 = torch.stack([rt, ch], -1).contiguous()
    to = torch.rand(R_, N_, device=dev) < 0.10
    g10 = torch.stack([torch.where(to, torch.rand(R_, N_, device=dev) * 0.6 + 0.5, rt), torch.where(to, 0.0, ch)], -1).contiguous()
    del rt, ch, to
    glegs = {"grad_unflagged": (g0, False)}
    if not a.unflagged_only:
        glegs.update({"grad_flagged_0pct_timeouts": (g0, True), "grad_flagged_10pct_timeouts": (g10, True)})
    REPS = 5
    for name, (g, cens) in glegs.items():
        def loop(g=g, ck=({"censored": True} if cens else {})):
            for _ in range(REPS):
                r = engine.wiener_log_likelihood_grad(engine.BASIC_DDM_DC, p, g, **ck)
            return float(torch.isfinite(r["grad"]).all()), 0
        runs[name] = loop

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, x
    for fn in runs.values():
        timed(fn)                                                       # warm-up of every shape the timed windows use
    t = {k: [] for k in runs}
    seen = {}
    for _ in range(3):                                                  # alternating
        for k, fn in runs.items():
            dt, seen[k] = timed(fn)
            t[k].append(dt / (REPS if k.startswith("grad") else iters))
    out = {"tool": "tools/wiener_hmc_rate.py --censored", "device": torch.cuda.get_device_name(0), "library": os.environ.get("NDDM_HIP_LIB", "in-tree"),
           "sampler": {"chains": D * CHAINS, "n_trials": N, "n_leapfrog": LEAPFROG, "timed_iterations": iters, "timeouts_per_set_at_3pct": 3},
           "gradient": {"rows": R_, "n_trials": N_, "layout": "paired", "launches_per_run": REPS}, "runs": 3, "legs": {}}
    for k in runs:
        unit = "seconds_per_launch" if k.startswith("grad") else "seconds_per_iteration"
        out["legs"][k] = {unit + "_runs": t[k], unit: float(np.median(t[k])), "spread_of_runs": float((max(t[k]) - min(t[k])) / np.median(t[k])),
                          "mean_accept_or_all_finite": seen[k][0], "flagged_chains": seen[k][1]}
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--iters", type=int, default=8000)
    ap.add_argument("--baseline-iters", type=int, default=60)
    ap.add_argument("--censored", action="store_true")
    ap.add_argument("--unflagged-only", action="store_true")
    a = ap.parse_args()
    if a.censored:
        return censored_legs(a)
    import torch
    import wiener_hmc_host as H
    from bayesflow_nddms_amd import engine, likelihood, mcmc
    engine.require_device()
    data_np = H.example_data(D, N, 41)
    theta = mcmc.hmc_init(data_np, CHAINS, 1).reshape(-1, 5)
    per = np.repeat(data_np, CHAINS, 0)
    dev = torch.device("cuda")
    data = torch.as_tensor(data_np).to(dev)
    kw = dict(chains_per_dataset=CHAINS, n_leapfrog=LEAPFROG, seed=3)
    # both routes start from chains that have found the posterior: 300 adapting iterations of the device loop (not timed)
    st = torch.as_tensor(mcmc.make_state(theta, per, eps0=EPS)).to(dev)
    engine.wiener_hmc(engine.BASIC_DDM_DC, data, st, n_iter=300, n_adapt=300, want_draws=False, want_log_post=False, **kw)
    torch.cuda.synchronize()
    eps = float(torch.exp(st[:, 5]).median())
    T = torch.as_tensor(np.minimum(1.5, per[..., 0].min(1).astype(np.float64))).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)

    def device_loop():
        s = st.clone()
        r = engine.wiener_hmc(engine.BASIC_DDM_DC, data, s, n_iter=a.iters, n_adapt=0, iter_offset=300, thin=10, **kw)
        return r["accept"].mean()

    def baseline():
        return torch_hmc(torch, engine, likelihood, data, st[:, :5].clone(), T, a.baseline_iters, eps, gen)[1]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        acc = float(fn())                                               # (reading the value back is the synchronise)
        return time.perf_counter() - t0, acc
    timed(device_loop)
    timed(baseline)                                                     # warm-up of every shape the timed windows use
    dev_t, base_t, dev_acc, base_acc = [], [], [], []
    for _ in range(3):                                                  # alternating
        t, x = timed(device_loop)
        dev_t.append(t / a.iters)
        dev_acc.append(x)
        t, x = timed(baseline)
        base_t.append(t / a.baseline_iters)
        base_acc.append(x)
    dev_it, base_it = float(np.median(dev_t)), float(np.median(base_t))
    rounds = (N + 63) // 64
    per_launch = engine.wiener_hmc_max_iter(N, LEAPFROG)
    total = 12_000
    out = {"tool": "tools/wiener_hmc_rate.py", "device": torch.cuda.get_device_name(0), "chains": D * CHAINS, "n_trials": N, "n_leapfrog": LEAPFROG,
           "step_size": eps, "timed_iterations": {"device_loop": a.iters, "torch_loop": a.baseline_iters}, "runs": 3,
           "device_loop": {"seconds_per_iteration_runs": dev_t, "seconds_per_iteration": dev_it, "mean_accept": float(np.mean(dev_acc)),
                           "seconds_per_leapfrog_step": dev_it / LEAPFROG, "seconds_per_trial_round": dev_it / (LEAPFROG * rounds),
                           "leapfrog_trials_per_second": D * CHAINS * LEAPFROG * N / dev_it},
           "torch_loop": {"seconds_per_iteration_runs": base_t, "seconds_per_iteration": base_it, "mean_accept": float(np.mean(base_acc)),
                          "launches_per_iteration": LEAPFROG, "leapfrog_trials_per_second": D * CHAINS * LEAPFROG * N / base_it},
           "speedup_device_loop_over_torch_loop": base_it / dev_it,
           "bounded_launch": {"max_rounds": engine.WHMC_MAX_ROUNDS, "max_iterations_at_this_shape": per_launch,
                              "seconds_of_a_full_launch": per_launch * dev_it},
           "projected_fit_2000_plus_10000": {"launches": math.ceil(total / per_launch) + 2, "device_loop_seconds": total * dev_it,
                                             "torch_loop_seconds": total * base_it}}
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
