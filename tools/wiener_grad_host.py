#!/usr/bin/env python3
"""The per-trial code and the chain rule of csrc/nddm_wiener_grad.h run on the HOST, without a GPU: the header's own wiener_grad_row,
wiener_grad_trial, wiener_grad_fold and wiener_grad_finish (over nddm_wiener.h's wiener_row and wiener_trial) compiled by the host compiler as a stand-alone
program against the stand-in for <hip/hip_runtime.h> of tools/host_build.py (the hardware's rcp / exp / log become the C
library's), optionally under AddressSanitizer and UndefinedBehaviorSanitizer.  A row's trials are summed in one sequence here (one lane), not
in the kernel's 64 interleaved ones: the float64 sums differ in their last bits, nothing more.

evaluate(exe, td, model, params [n, P], data [n, N, 2]) -> (loglik [n], grad [n, P]) in float64.

Usage: python tools/wiener_grad_host.py [--sanitize] [--json OUT]      prints one JSON line: per model and parameter column, the largest
|gradient - yardstick| / scale_j over tests/wiener_cdf_ref.prior_rows (20 000 rows each, one trial per row; tests/wiener_grad_ref.py is the
float64 yardstick and defines scale_j), and the bar B = 4 x the largest of them, rounded up to one significant digit.
With --censored: the same for NDDM_WIENER_CENSORED's instantiation on rows with 10 % timeouts (censored_survey).
"""
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wiener_host as H  # noqa: E402  (trial_data)
import host_build as B  # noqa: E402  (the stand-in header, the compiler call, the command line)

MAIN = r"""// usage: wiener_grad_host MODEL(0|3) in.bin out.bin [censored] ; in: int32 n, int32 N, then n * (P + 2N) floats (params, N trials); out: n * (1 + P) doubles
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "nddm_wiener_grad.h"
using namespace nddm;
template <int MODEL, bool CENSORED = false> void run(int n, int N, int P, const float *in, double *out) {
    for (int i = 0; i < n; ++i) {
        const float *p = in + (size_t)i * (P + 2 * N), *d = p + P;
        const WienerRow c = wiener_row<MODEL>(p);
        const WienerGradRow g = wiener_grad_row<MODEL>(p, c);
        WienerGradAcc s = wiener_grad_zero();
        for (int j = 0; j < N; ++j) wiener_grad_trial<MODEL, CENSORED>(c, g, d[2 * j], d[2 * j + 1], s);
        wiener_grad_fold<MODEL>(s);
        wiener_grad_finish<MODEL>(p, c.valid, s, out + (size_t)i * (1 + P), out + (size_t)i * (1 + P) + 1);
    }
}
int main(int argc, char **argv) {
    if (argc != 4 && argc != 5) return 1;
    int model = atoi(argv[1]);
    const bool censored = argc == 5;                                    // NDDM_WIENER_CENSORED's instantiation (basic_ddm_dc)
    if (censored && model != 0) return 5;
    FILE *f = fopen(argv[2], "rb"); int hdr[2]; if (!f || fread(hdr, 4, 2, f) != 2) return 2;
    int n = hdr[0], N = hdr[1], P = model == 0 ? 5 : 6;
    std::vector<float> in((size_t)n * (P + 2 * N));
    std::vector<double> out((size_t)n * (1 + P));
    if (fread(in.data(), 4, in.size(), f) != in.size()) return 3;
    fclose(f);
    if (censored) run<NDDM_BASIC_DDM_DC, true>(n, N, P, in.data(), out.data());
    else if (model == 0) run<NDDM_BASIC_DDM_DC>(n, N, P, in.data(), out.data()); else run<NDDM_ALPHA_NOT_SCALED>(n, N, P, in.data(), out.data());
    f = fopen(argv[3], "wb"); if (!f) return 4;
    fwrite(out.data(), 8, out.size(), f); fclose(f);
    return 0;
}
"""


def build(td, sanitize=False):
    return B.build(td, MAIN, "wiener_grad_host", sanitize)


def evaluate(exe, td, model, params, data, censored=False):
    """params [n, P], data [n, N, 2] in the model's trial format -> float64 (loglik [n], grad [n, P]) as the header gives them.
    censored: the NDDM_WIENER_CENSORED instantiation (model 0)."""
    params, data = np.asarray(params, np.float32), np.asarray(data, np.float32)
    n, P = params.shape
    N = data.shape[1]
    with open(os.path.join(td, "in.bin"), "wb") as f:
        f.write(np.array([n, N], np.int32).tobytes())
        f.write(np.concatenate([params, data.reshape(n, 2 * N)], 1).astype(np.float32).tobytes())
    subprocess.check_call([exe, str(model), os.path.join(td, "in.bin"), os.path.join(td, "out.bin")] + (["censored"] if censored else []))
    o = np.fromfile(os.path.join(td, "out.bin"), np.float64).reshape(n, 1 + P)
    return o[:, 0], o[:, 1:]


def round_up_1sd(x):
    """x rounded UP to one significant digit."""
    e = math.floor(math.log10(x))
    return math.ceil(x / 10.0 ** e - 1e-12) * 10.0 ** e


def survey(sanitize=False, n=20_000):
    sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT]
    import wiener_cdf_ref as C
    import wiener_grad_ref as G
    out = {"tool": "tools/wiener_grad_host.py", "sanitized": bool(sanitize), "rows_per_model": int(n), "trials_per_row": 1, "cases": {}}
    worst = 0.0
    with tempfile.TemporaryDirectory() as td:
        exe = build(td, sanitize)
        for name, basic in (("basic_ddm_dc", True), ("alpha_not_scaled", False)):
            p32, rt32, up, t = C.prior_rows(n, basic)
            ll, grad = evaluate(exe, td, 0 if basic else 3, p32, H.trial_data(basic, rt32, up)[:, None, :])
            ref, scale = G.row_grad(basic, p32.astype(np.float64), t[:, None], up[:, None])
            finite = np.isfinite(ref).all(1) & (scale > 0).any(1)
            with np.errstate(all="ignore"):
                rel = np.where(scale > 0, np.abs(grad - ref) / scale, np.where(grad == ref, 0.0, np.inf))
            out["cases"][name] = {"rows": int(n), "yardstick_finite_rows": int(finite.sum()), "header_finite_rows": int(np.isfinite(grad).all(1).sum()),
                                  "max_err_over_scale": {c: float(rel[:, j].max()) for j, c in enumerate(G.COLUMNS[basic])},
                                  "p99_err_over_scale": {c: float(np.percentile(rel[:, j], 99)) for j, c in enumerate(G.COLUMNS[basic])}}
            worst = max(worst, float(rel.max()))
    out["max_err_over_scale"] = worst
    out["bar_B"] = round_up_1sd(4.0 * worst)
    out["bar_rule"] = "4 x the largest error on the host, rounded up to one significant digit (the hardware transcendentals' last ulp)"
    return out


def censored_survey(sanitize=False, n_prior=5000, n_box=2000):
    """NDDM_WIENER_CENSORED's instantiation over wiener_cdf_ref.censor_sets()'s prior_1s, prior_4s and box rows, 160 trials per row of
    which 16 (10 %) are timeouts at the set's times (tests/wiener_censored_ref.py: censored_rows, the float64 yardstick and scale_j)."""
    sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT]
    import wiener_cdf_ref as C
    import wiener_censored_ref as R
    import wiener_grad_ref as G
    out = {"tool": "tools/wiener_grad_host.py --censored", "sanitized": bool(sanitize), "trials_per_row": R.TRIALS_PER_ROW,
           "censored_per_row": R.CENSORED_PER_ROW, "cases": {}}
    worst = 0.0
    sets = C.censor_sets(n_prior=n_prior, n_box=n_box, with_fixture=False)
    with tempfile.TemporaryDirectory() as td:
        exe = build(td, sanitize)
        for name in ("prior_1s", "prior_4s", "box"):
            p32, rt32, _ = sets[name]
            rows, data, t, code = R.censored_rows(p32, rt32)
            ll, grad = evaluate(exe, td, 0, p32[rows], data, censored=True)
            ref, scale = R.row_grad(p32[rows].astype(np.float64), t, code)
            assert np.all(np.isfinite(ref)) and np.all(scale > 0)
            rel = np.abs(grad - ref) / scale
            out["cases"][name] = {"rows_of_the_set": int(p32.shape[0]), "rows": int(rows.size), "header_finite_rows": int(np.isfinite(grad).all(1).sum()),
                                  "max_err_over_scale": {c: float(rel[:, j].max()) for j, c in enumerate(R.COLUMNS)},
                                  "p99_err_over_scale": {c: float(np.percentile(rel[:, j], 99)) for j, c in enumerate(R.COLUMNS)}}
            worst = max(worst, float(np.nanmax(rel)))
            # the timeouts alone (a row of 16 timeouts, no response to lend its scale): reported, not part of the bar's rule
            cens = code[0] == 0
            ll, grad = evaluate(exe, td, 0, p32[rows], data[:, cens], censored=True)
            ref, scale = R.row_grad(p32[rows].astype(np.float64), t[:, cens], code[:, cens])
            with np.errstate(all="ignore"):
                rel = np.where(scale > 1e-12, np.abs(grad - ref) / scale, np.abs(grad - ref))   # (S = 1 to the last bit: absolute)
            out["cases"][name]["timeouts_alone_max_err_over_scale"] = {c: float(rel[:, j].max()) for j, c in enumerate(R.COLUMNS)}
            out["cases"][name]["timeouts_alone_p99_err_over_scale"] = {c: float(np.percentile(rel[:, j], 99)) for j, c in enumerate(R.COLUMNS)}
    out["max_err_over_scale"] = worst
    out["bar"] = G.BAR_B if worst <= G.BAR_B else round_up_1sd(4.0 * worst)
    out["bar_rule"] = ("wiener_grad_ref.BAR_B where the largest error on the host is within it; otherwise 4 x that error, rounded up to one "
                       "significant digit (the hardware transcendentals' last ulp)")
    return out


if __name__ == "__main__":
    if "--censored" in sys.argv:
        sys.argv.remove("--censored")
        B.cli(censored_survey)
    else:
        B.cli(survey)
