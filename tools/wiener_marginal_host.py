#!/usr/bin/env python3
"""The per-trial code of csrc/nddm_wiener_marginal.h run on the HOST, without a GPU: the header's own wiener_marginal_base,
wiener_marginal_row and wiener_marginal_trial (over nddm_wiener.h's wiener_row, wiener_logpdf and wiener_log_survival) compiled by the host
compiler as a stand-alone program against the stand-in for <hip/hip_runtime.h> of tools/host_build.py (the hardware's rcp / exp /
log become the C library's), optionally under AddressSanitizer and UndefinedBehaviorSanitizer.  A pass's node values live in a local array
here, in LDS in the kernel; nothing else differs.

evaluate(exe, td, params [n, 8], data [n, N, 2], t_censor) -> float32 trial log-likelihoods [n, N] as the header gives them.

Usage: python tools/wiener_marginal_host.py [--sanitize] [--rows N] [--json OUT]      prints one JSON line: per row set of
tests/wiener_marginal_ref.py (prior_rows, box; one trial per row) the largest |log L - yardstick| of the header's float32 and of the
scheme restated in float64 (the quadrature's own share), and the device bar 4 x the float32 figure rounded up to one significant digit.
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

MAIN = r"""// usage: wiener_marginal_host T_CENSOR in.bin out.bin ; in: int32 n, int32 N, then n * (8 + 2N) floats (params, N trials); out: n * N floats
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "nddm_wiener_marginal.h"
using namespace nddm;
int main(int argc, char **argv) {
    if (argc != 4) return 1;
    const float t_censor = (float)atof(argv[1]);
    FILE *f = fopen(argv[2], "rb"); int hdr[2]; if (!f || fread(hdr, 4, 2, f) != 2) return 2;
    const int n = hdr[0], N = hdr[1];
    std::vector<float> in((size_t)n * (8 + 2 * N)), out((size_t)n * N);
    if (fread(in.data(), 4, in.size(), f) != in.size()) return 3;
    fclose(f);
    float buf[WMARG_K];
    for (int i = 0; i < n; ++i) {
        const float *p = in.data() + (size_t)i * (8 + 2 * N), *d = p + 8;
        const WienerRow b = wiener_marginal_base(p);
        const WienerMarginalRow r = wiener_marginal_row(p);
        for (int j = 0; j < N; ++j) out[(size_t)i * N + j] = wiener_marginal_trial(b, r, d[2 * j], d[2 * j + 1], t_censor, buf, 1);
    }
    f = fopen(argv[3], "wb"); if (!f) return 4;
    fwrite(out.data(), 4, out.size(), f); fclose(f);
    return 0;
}
"""


def build(td, sanitize=False):
    return B.build(td, MAIN, "wiener_marginal_host", sanitize)


def evaluate(exe, td, params, data, t_censor):
    """params [n, 8], data [n, N, 2] = (choicert, z1) -> float32 [n, N] as the header gives them."""
    params, data = np.asarray(params, np.float32), np.asarray(data, np.float32)
    n, N = params.shape[0], data.shape[1]
    with open(os.path.join(td, "in.bin"), "wb") as f:
        f.write(np.array([n, N], np.int32).tobytes())
        f.write(np.concatenate([params, data.reshape(n, 2 * N)], 1).astype(np.float32).tobytes())
    subprocess.check_call([exe, repr(float(t_censor)), os.path.join(td, "in.bin"), os.path.join(td, "out.bin")])
    return np.fromfile(os.path.join(td, "out.bin"), np.float32).reshape(n, N)


def round_up_1sd(x):
    """x rounded UP to one significant digit."""
    e = math.floor(math.log10(x))
    return math.ceil(x / 10.0 ** e - 1e-12) * 10.0 ** e


def survey(sanitize=False, n=1500):
    sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT]
    import wiener_marginal_ref as M
    out = {"tool": "tools/wiener_marginal_host.py", "sanitized": bool(sanitize), "rows_per_set": int(n), "trials_per_row": 1, "cases": {}}
    with tempfile.TemporaryDirectory() as td:
        exe = build(td, sanitize)
        for name, rows in (("prior_rows", M.prior_rows), ("box", M.box)):
            p32, y32, z32, tc = rows(n)
            got = evaluate(exe, td, p32, np.stack([y32, z32], 1)[:, None, :], tc)[:, 0].astype(np.float64)
            p, y, z = M.as_f64(p32, y32, z32)
            ref, sch = M.log_lik(p, y, z, tc), M.scheme_log_lik(p, y, z, tc)
            err, e64 = np.abs(got - ref), np.abs(sch - ref)
            w = int(np.argmax(err))
            out["cases"][name] = {"rows": int(n), "censored": int((y32 == 0).sum()), "t_censor": float(tc), "finite": int(np.isfinite(got).sum()),
                                  "max_abs_err_float32": float(err.max()), "p99_abs_err_float32": float(np.percentile(err, 99)),
                                  "median_abs_err_float32": float(np.median(err)), "max_abs_err_scheme_float64": float(e64.max()),
                                  "worst_row": {"index": w, "params": [float(v) for v in p32[w]], "y": float(y32[w]), "z": float(z32[w]),
                                                "yardstick": float(ref[w]), "float32": float(got[w])},
                                  "device_bar": round_up_1sd(4.0 * float(err.max()))}
    out["bar_rule"] = "per set, 4 x the largest float32 error on the host, rounded up to one significant digit (the hardware transcendentals' last ulp)"
    return out


if __name__ == "__main__":
    B.cli(survey, rows=1500)
