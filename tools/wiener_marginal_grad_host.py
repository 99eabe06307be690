#!/usr/bin/env python3
"""The per-trial code and the chain rule of csrc/nddm_wiener_marginal_grad.h run on the HOST, without a GPU: the header's own
wiener_marginal_grad_trial, wiener_marginal_grad_fold and wiener_marginal_grad_finish (over nddm_wiener_marginal.h's row constants and node, nddm_wiener_grad.h's row
constants and the header's own partials of log S) compiled by the host compiler as a stand-alone program with its own main against the
stand-in for <hip/hip_runtime.h> of tools/host_build.py (the hardware's rcp / exp / log become the C library's), optionally under
AddressSanitizer and UndefinedBehaviorSanitizer.  Nothing is loaded into Python.  A pass's node values live in a local array here, in LDS in the
kernel, and a row's trials are summed in one sequence (one lane), not in the kernel's 64 interleaved ones; nothing else differs.

evaluate(exe, td, params [n, 8], data [n, N, 2], t_censor) -> float64 (loglik [n], grad [n, 8]) as the header gives them.
survival(exe, td, a', w, v', t) -> float32 [n, 4] = wiener_log_survival_grad's (log S, d/da', d/dw, d/dv').

Usage: python tools/wiener_marginal_grad_host.py [--sanitize] [--rows N] [--json OUT]      prints one JSON line: per row set of
tests/wiener_marginal_ref.py (prior_rows, box; one trial per row) and parameter column, the largest and the 99th-percentile
|gradient - yardstick| / scale_j (tests/wiener_marginal_grad_ref.py is the float64 yardstick; with one trial per row scale_j is
|yardstick_j|), and the set's device bar, 4 x the largest of them rounded up to one significant digit.
"""
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_build as B  # noqa: E402  (the stand-in header, the compiler call, the command line)

MAIN = r"""// usage: wiener_marginal_grad_host grad T_CENSOR in.bin out.bin ; in: int32 n, int32 N, then n * (8 + 2N) floats (params, N trials); out: n * 9 doubles
//        wiener_marginal_grad_host surv 0 in.bin out.bin        ; in: int32 n, int32 0, then n * 4 floats (a', w, v', t); out: n * 4 floats
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
inline double erfcx(double x) {                         // (the device library's; x >= 0 here)
    if (x < 25.0) return exp(x * x) * erfc(x);
    const double i2 = 1.0 / (x * x);
    return 0.5641895835477563 / x * (1.0 - 0.5 * i2 + 0.75 * i2 * i2 - 1.875 * i2 * i2 * i2);
}
#include "nddm_wiener_marginal_grad.h"
using namespace nddm;
int main(int argc, char **argv) {
    if (argc != 5) return 1;
    const bool surv = !strcmp(argv[1], "surv");
    const float t_censor = (float)atof(argv[2]);
    FILE *f = fopen(argv[3], "rb"); int hdr[2]; if (!f || fread(hdr, 4, 2, f) != 2) return 2;
    const int n = hdr[0], N = hdr[1];
    std::vector<float> in((size_t)n * (surv ? 4 : 8 + 2 * N));
    if (fread(in.data(), 4, in.size(), f) != in.size()) return 3;
    fclose(f);
    f = fopen(argv[4], "wb"); if (!f) return 4;
    if (surv) {
        std::vector<float> out((size_t)n * 4);
        for (int i = 0; i < n; ++i) {
            const float *q = in.data() + (size_t)i * 4;
            const float pb[5] = {q[2], q[0], q[1], 0.0f, 1.0f};
            const WienerSurvivalGrad g = wiener_log_survival_grad(wiener_row<NDDM_BASIC_DDM_DC>(pb), q[3]);
            out[4 * i] = g.ls; out[4 * i + 1] = g.da; out[4 * i + 2] = g.dw; out[4 * i + 3] = g.dv;
        }
        fwrite(out.data(), 4, out.size(), f);
    } else {
        std::vector<double> out((size_t)n * 9);
        float buf[WMARG_K];
        for (int i = 0; i < n; ++i) {
            const float *p = in.data() + (size_t)i * (8 + 2 * N), *d = p + 8;
            const WienerRow b = wiener_marginal_base(p);
            const WienerMarginalRow r = wiener_marginal_row(p);
            const float pb[5] = {p[0], p[5], p[2], 0.0f, p[5]};
            const WienerGradRow g = wiener_grad_row<NDDM_BASIC_DDM_DC>(pb, b);
            WienerMarginalGradAcc s = wiener_marginal_grad_zero();
            for (int j = 0; j < N; ++j) wiener_marginal_grad_trial(b, r, g, (double)p[7] * (double)p[1], d[2 * j], d[2 * j + 1], t_censor, buf, 1, s);
            wiener_marginal_grad_fold(s);
            wiener_marginal_grad_finish(p, r.valid * b.valid, N, s, &out[(size_t)i * 9], &out[(size_t)i * 9 + 1]);
        }
        fwrite(out.data(), 8, out.size(), f);
    }
    fclose(f);
    return 0;
}
"""


def build(td, sanitize=False):
    return B.build(td, MAIN, "wiener_marginal_grad_host", sanitize)


def evaluate(exe, td, params, data, t_censor):
    """params [n, 8], data [n, N, 2] = (choicert, z1) -> float64 (loglik [n], grad [n, 8]) as the header gives them."""
    params, data = np.asarray(params, np.float32), np.asarray(data, np.float32)
    n, N = params.shape[0], data.shape[1]
    with open(os.path.join(td, "in.bin"), "wb") as f:
        f.write(np.array([n, N], np.int32).tobytes())
        f.write(np.concatenate([params, data.reshape(n, 2 * N)], 1).astype(np.float32).tobytes())
    subprocess.check_call([exe, "grad", repr(float(t_censor)), os.path.join(td, "in.bin"), os.path.join(td, "out.bin")])
    o = np.fromfile(os.path.join(td, "out.bin"), np.float64).reshape(n, 9)
    return o[:, 0], o[:, 1:]


def survival(exe, td, ap, w, vp, t):
    """wiener_log_survival_grad on rows of (a', w, v', t) -> float32 [n, 4] = (log S, d/da', d/dw, d/dv')."""
    q = np.stack(np.broadcast_arrays(ap, w, vp, t), -1).astype(np.float32)
    with open(os.path.join(td, "sin.bin"), "wb") as f:
        f.write(np.array([q.shape[0], 0], np.int32).tobytes())
        f.write(q.tobytes())
    subprocess.check_call([exe, "surv", "0", os.path.join(td, "sin.bin"), os.path.join(td, "sout.bin")])
    return np.fromfile(os.path.join(td, "sout.bin"), np.float32).reshape(-1, 4)


def round_up_1sd(x):
    """x rounded UP to one significant digit."""
    e = math.floor(math.log10(x))
    return math.ceil(x / 10.0 ** e - 1e-12) * 10.0 ** e


def errors_over_scale(grad, ref, scale):
    """|grad - ref| / scale per element; where scale is 0 the two must be equal."""
    with np.errstate(all="ignore"):
        return np.where(scale > 0, np.abs(grad - ref) / scale, np.where(grad == ref, 0.0, np.inf))


def survey(sanitize=False, n=1500):
    sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT]
    import wiener_marginal_grad_ref as MG
    import wiener_marginal_ref as M
    out = {"tool": "tools/wiener_marginal_grad_host.py", "sanitized": bool(sanitize), "rows_per_set": int(n), "trials_per_row": 1, "cases": {}}
    with tempfile.TemporaryDirectory() as td:
        exe = build(td, sanitize)
        for name, rows in (("prior_rows", M.prior_rows), ("box", M.box)):
            p32, y32, z32, tc = rows(n)
            ll, grad = evaluate(exe, td, p32, np.stack([y32, z32], 1)[:, None, :], tc)
            ref = MG.grad_log_lik(*M.as_f64(p32, y32, z32), tc)
            rel = errors_over_scale(grad, ref, np.abs(ref))
            w = np.unravel_index(int(np.argmax(rel)), rel.shape)
            out["cases"][name] = {
                "rows": int(n), "censored": int((y32 == 0).sum()), "t_censor": float(tc), "yardstick_finite_rows": int(np.isfinite(ref).all(1).sum()),
                "header_finite_rows": int(np.isfinite(grad).all(1).sum()), "max_abs_gradient": float(np.abs(ref).max()),
                "max_err_over_scale": {c: float(rel[:, j].max()) for j, c in enumerate(MG.COLUMNS)},
                "p99_err_over_scale": {c: float(np.percentile(rel[:, j], 99)) for j, c in enumerate(MG.COLUMNS)},
                "worst": {"row": int(w[0]), "column": MG.COLUMNS[w[1]], "params": [float(v) for v in p32[w[0]]], "y": float(y32[w[0]]),
                          "z": float(z32[w[0]]), "yardstick": float(ref[w]), "float32": float(grad[w]), "err_over_scale": float(rel[w])},
                "device_bar": round_up_1sd(4.0 * float(rel.max()))}
    out["bar_rule"] = "per set, 4 x the largest error over scale on the host, rounded up to one significant digit (the hardware transcendentals' last ulp)"
    return out


if __name__ == "__main__":
    B.cli(survey, rows=1500)
