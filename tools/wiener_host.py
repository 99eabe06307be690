#!/usr/bin/env python3
"""The per-trial code of csrc/nddm_wiener.h and csrc/nddm_wiener_cdf.h run on the HOST, without a GPU: the headers' own wiener_row,
wiener_trial (a censored choice 0 included), wiener_cdf_side and wiener_cdf_trial compiled by the host compiler as a stand-alone program
against the stand-in for <hip/hip_runtime.h> of tools/host_build.py (the hardware's rcp / rsq / exp / log become the C
library's), optionally under AddressSanitizer and UndefinedBehaviorSanitizer.  The device's numbers differ by the hardware
transcendentals' last ulp; what float32 cannot hold on the host it cannot hold on the device either.

evaluate(exe, td, model, params [n, P], data [n, 2]) -> (log f or log S [n], F [n], P(upper) [n]), one trial per row.

Usage: python tools/wiener_host.py [--sanitize] [--json OUT]      prints one JSON line: the largest errors against the float64 yardsticks
(tests/wiener_ref.py, tests/wiener_cdf_ref.py) over the rows of tests/test_wiener_host.py.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_build as B  # noqa: E402  (the stand-in header, the compiler call, the command line)

MAIN = r"""// usage: wiener_host MODEL(0|3) in.bin out.bin ; in: int32 n, then n*(P+2) floats (params, x0, x1); out: n * (log f | log S, F, P(upper))
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "nddm_wiener_cdf.h"
using namespace nddm;
template <int MODEL> void run(int n, int P, const float *in, float *out) {
    for (int i = 0; i < n; ++i) {
        const float *p = in + (size_t)i * (P + 2);
        WienerRow wr = wiener_row<MODEL>(p);
        WienerCdfSide cs[2];
        for (int s = 0; s < 2; ++s) cs[s] = wiener_cdf_side<MODEL>(wr, p, s);
        out[3 * i] = wiener_trial<MODEL>(wr, p[P], p[P + 1]);
        out[3 * i + 1] = wiener_cdf_trial<MODEL>(cs, &wr, p[P], p[P + 1]);
        out[3 * i + 2] = cs[1].P;
    }
}
int main(int argc, char **argv) {
    if (argc != 4) return 1;
    int model = atoi(argv[1]);
    FILE *f = fopen(argv[2], "rb"); int n; if (!f || fread(&n, 4, 1, f) != 1) return 2;
    int P = model == 0 ? 5 : 6;
    std::vector<float> in((size_t)n * (P + 2)), out((size_t)n * 3);
    if (fread(in.data(), 4, in.size(), f) != in.size()) return 3;
    fclose(f);
    if (model == 0) run<NDDM_BASIC_DDM_DC>(n, P, in.data(), out.data()); else run<NDDM_ALPHA_NOT_SCALED>(n, P, in.data(), out.data());
    f = fopen(argv[3], "wb"); if (!f) return 4;
    fwrite(out.data(), 4, out.size(), f); fclose(f);
    return 0;
}
"""


def build(td, sanitize=False):
    return B.build(td, MAIN, "wiener_host", sanitize)


def evaluate(exe, td, model, params, data):
    """params [n, P] and data [n, 2] in the model's trial format, one trial per row -> float64 (log f, or log S on choice 0; the
    distribution function; P(upper)), each [n], as the float32 the headers give."""
    params, data = np.asarray(params, np.float32), np.asarray(data, np.float32)
    n = params.shape[0]
    with open(os.path.join(td, "in.bin"), "wb") as f:
        f.write(np.int32(n).tobytes())
        f.write(np.concatenate([params, data], 1).astype(np.float32).tobytes())
    subprocess.check_call([exe, str(model), os.path.join(td, "in.bin"), os.path.join(td, "out.bin")])
    o = np.fromfile(os.path.join(td, "out.bin"), np.float32).reshape(n, 3).astype(np.float64)
    return o[:, 0], o[:, 1], o[:, 2]


def trial_data(basic, rt32, up):
    """(rt, boundary) as one trial per row in the model's format, float32 [n, 2]."""
    if basic:
        return np.stack([rt32, np.where(up, 1.0, -1.0)], 1).astype(np.float32)
    y = np.where(up, rt32, -rt32).astype(np.float32)
    return np.stack([y, (np.sign(y) + 1) / 2], 1).astype(np.float32)


def survey(sanitize=False, n=20_000):
    sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT]
    import wiener_cdf_ref as C
    import wiener_ref as W
    out = {"tool": "tools/wiener_host.py", "sanitized": bool(sanitize), "cases": {}}
    with tempfile.TemporaryDirectory() as td:
        exe = build(td, sanitize)
        for name, basic, (p32, rt32, up, t) in (("basic_prior", True, C.prior_rows(n, True)), ("alpha_ns_prior_and_box", False, C.prior_rows(n, False))):
            lf, F, pu = evaluate(exe, td, 0 if basic else 3, p32, trial_data(basic, rt32, up))
            a, v, beta, _, s, eta = C.row_columns(p32, basic)
            ref = W.log_f(t, up, a, v, beta, s, eta)
            err, inner = np.abs(lf - ref), np.abs(ref) <= 20
            out["cases"][name] = {"rows": int(n), "max_abs_dlogf_inner": float(err[inner].max()),
                                  "max_rel_dlogf_beyond": float(np.max(err[~inner] / np.abs(ref[~inner]))) if np.any(~inner) else 0.0,
                                  "max_abs_dF": float(np.max(np.abs(F - C.cdf(t, up, a, v, beta, s, eta)))),
                                  "max_abs_dp_upper": float(np.max(np.abs(pu - C.p_upper(a, v, beta, s, eta))))}
        for name, (p32, rt32, t) in C.censor_sets().items():
            a, v, beta, _, s, _ = C.row_columns(p32, True)
            ref, ok = C.log_survival(t, a[:, None], v[:, None], beta[:, None], s[:, None])
            m = t.shape[1]
            lp, F, _ = evaluate(exe, td, 0, np.repeat(p32, m, 0), np.stack([rt32.ravel(), np.zeros(rt32.size)], 1))
            lp, F = lp.reshape(t.shape), F.reshape(t.shape)
            case = {"rows": int(p32.shape[0]), "points_S_ge_1e-3": int(ok.sum()), "nan": int(np.isnan(lp).sum()), "above_0": int((lp > 0).sum()),
                    "increasing_pairs": int((np.diff(lp, axis=1) > 0).sum()),
                    "max_err_over_bar": float(np.max((np.abs(lp - ref) / (2e-5 + 1e-5 * np.abs(ref)))[ok])),
                    "max_abs_dcdf": float(np.max(np.abs(F - (-np.expm1(ref)))[ok]))}
            if name == "fixture":                       # the file's own values: below S = 1e-3 they are the high-precision series'
                g = np.load(os.path.join(ROOT, "tests", "golden", "wiener_survival.npz"))
                deep = g["mp"]
                case["points_S_lt_1e-3"] = int(deep.sum())
                case["max_rel_err_S_lt_1e-3"] = float(np.max((np.abs(lp - g["log_s"]) / np.abs(g["log_s"]))[deep]))
                case["max_abs_dcdf_S_lt_1e-3"] = float(np.max(np.abs(F - (-np.expm1(g["log_s"])))[deep]))
                case["reported_rows_log_S"] = [float(x) for x in lp[:4, -1]]
            out["cases"]["censored_" + name] = case
    return out


if __name__ == "__main__":
    B.cli(survey)
