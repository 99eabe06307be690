#!/usr/bin/env python3
"""The quantile solver of csrc/nddm_wiener_quantile.h run on the HOST, without a GPU: the header's own per-request code (wiener_row,
wiener_cdf_side, wiener_quantile_request and the two forms of the distribution function under them) compiled by the host compiler
against a small stand-in for <hip/hip_runtime.h> -- the hardware's rcp / rsq / exp / log become the C library's, erfcx is exp(x^2) erfc(x)
in float64.  It answers what the kernel cannot tell from outside: HOW MANY evaluations of G a request takes.  Over the rows of the
accuracy tests (tests/wiener_cdf_ref.py: accuracy_rows with tau = 0, conditional p ~ U(0.001, 0.999) on the drawn boundary) it prints one
JSON line.  Per model and mode (conditional, defective, either boundary): the mean / 99th percentile / largest number of evaluations per
request; `max_abs_residual`, the largest |F(q) - target| with F the HEADER'S OWN distribution function and the target as the solver had it
(the solver's residual, bar (i) of the device test); and `max_abs_yardstick_minus_target`, the float64 yardstick at q against p P_float64
(conditional: bar (ii), 6e-5) or against the float32 target (defective: bar (iii), 4e-5).  Then the four extreme rows of the distribution
function's tests, and the reference sampler's tables (tests/golden/ratcliff.npz) in ranks, with the next set's row as control.

Usage: python tools/wiener_quantile_host.py [--sanitize] [--json OUT]      (--sanitize: -fsanitize=address,undefined)
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_build as B  # noqa: E402  (the stand-in header, the compiler call, the command line)

MAIN = r"""// usage: wiener_quantile_host MODEL(0|3) FLAGS in.bin out.bin ; in: int32 n, then n*(P+2) floats (params, p, code); out: n * (rt, evaluations, F(rt), P(boundary))
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "nddm_wiener_quantile.h"
using namespace nddm;
template <int MODEL> void run(int n, int P, const float *in, unsigned flags, float *out) {
    for (int i = 0; i < n; ++i) {
        const float *p = in + (size_t)i * (P + 2);
        WienerRow wr = wiener_row<MODEL>(p);
        WienerCdfSide cs[2]; WienerQuantileSide qs[2];
        for (int s = 0; s < 2; ++s) { cs[s] = wiener_cdf_side<MODEL>(wr, p, s); qs[s] = wiener_quantile_side(cs[s]); }
        int ev;
        float q = wiener_quantile_request(cs, qs, p[P], p[P + 1], flags, ev);
        out[4 * i] = q; out[4 * i + 1] = (float)ev;
        float F = 0;
        if (p[P + 1] == 0.0f) F = wiener_cdf_value(cs[0], q) + wiener_cdf_value(cs[1], q);
        else F = wiener_cdf_value(cs[p[P + 1] > 0 ? 1 : 0], q);
        out[4 * i + 2] = F;
        out[4 * i + 3] = p[P + 1] == 0.0f ? cs[0].P + cs[1].P : cs[p[P + 1] > 0 ? 1 : 0].P;
    }
}
int main(int argc, char **argv) {
    int model = atoi(argv[1]); unsigned flags = (unsigned)atoi(argv[2]);
    FILE *f = fopen(argv[3], "rb"); int n; if (fread(&n, 4, 1, f) != 1) return 2;
    int P = model == 0 ? 5 : 6;
    std::vector<float> in((size_t)n * (P + 2)), out((size_t)n * 4);
    if (fread(in.data(), 4, in.size(), f) != in.size()) return 3;
    fclose(f);
    if (model == 0) run<NDDM_BASIC_DDM_DC>(n, P, in.data(), flags, out.data()); else run<NDDM_ALPHA_NOT_SCALED>(n, P, in.data(), flags, out.data());
    f = fopen(argv[4], "wb"); fwrite(out.data(), 4, out.size(), f); fclose(f);
    return 0;
}
"""


def build(td, sanitize=False, main=None, name="wiener_quantile_host"):
    """Compile `main` (this tool's own program by default) against the stand-in header."""
    return B.build(td, MAIN if main is None else main, name, sanitize)


def solve(exe, td, model, flags, params, probs):
    """params [n, P], probs [n, 2] = (p, code), one request per row -> (rt [n], evaluations [n], the header's F at rt [n], its
    P(boundary) [n])."""
    n = params.shape[0]
    with open(os.path.join(td, "in.bin"), "wb") as f:
        f.write(np.int32(n).tobytes())
        f.write(np.concatenate([params, probs], 1).astype(np.float32).tobytes())
    subprocess.check_call([exe, str(model), str(flags), os.path.join(td, "in.bin"), os.path.join(td, "out.bin")])
    o = np.fromfile(os.path.join(td, "out.bin"), np.float32).reshape(n, 4)
    return o[:, 0], o[:, 1].astype(np.int64), o[:, 2], o[:, 3]


def survey(sanitize=False):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import wiener_cdf_ref as C
    out = {"tool": "tools/wiener_quantile_host.py", "sanitized": bool(sanitize), "cases": {}}
    with tempfile.TemporaryDirectory() as td:
        exe = build(td, sanitize)
        for basic, n in ((False, 20_000), (True, 2_000)):
            p32, _, up, _ = C.accuracy_rows(n, basic)
            p32 = p32.copy()
            p32[:, 3] = 0.0
            a, v, beta, _, s, eta = C.row_columns(p32, basic)
            pu = C.p_upper(a, v, beta, s, eta)
            P64 = np.where(up, pu, 1.0 - pu)
            keep = P64 >= 0.01
            pc = np.random.default_rng(21).uniform(0.001, 0.999, n).astype(np.float32)
            code = np.where(up, 1.0, -1.0)
            model = 0 if basic else 3
            name = "basic_ddm_dc" if basic else "alpha_not_scaled"
            for mode, flags, p, cd, sel in (("conditional", 1, pc, code, keep), ("defective", 0, (pc * P64).astype(np.float32), code, keep),
                                            ("either_boundary", 0, pc, np.zeros(n), np.ones(n, bool))):
                q, ev, F, lim = solve(exe, td, model, flags, p32, np.stack([p, cd], 1))
                fin = sel & np.isfinite(q)
                tgt = p.astype(np.float64) * lim if flags else p.astype(np.float64)        # the target as the solver had it
                out["cases"][f"{name}_{mode}"] = {
                    "requests": int(sel.sum()), "finite": int(fin.sum()), "evals_mean": float(ev[sel].mean()),
                    "evals_p99": float(np.percentile(ev[sel], 99)), "evals_max": int(ev[sel].max()),
                    "max_abs_residual": float(np.max(np.abs(F[fin] - tgt[fin])))}
                # the float64 yardstick at the answer: against p P_float64 (conditional) or against the float32 target (defective)
                if mode != "either_boundary":
                    ref = pc.astype(np.float64) * P64 if flags else p.astype(np.float64)
                    out["cases"][f"{name}_{mode}"]["max_abs_yardstick_minus_target"] = float(
                        np.max(np.abs(C.cdf(q.astype(np.float64), up, a, v, beta, s, eta) - ref)[fin]))
        out["cases"]["extreme_rows_conditional"] = _extreme_rows(exe, td)
        out["cases"]["golden_tables_defective"] = _golden_tables(exe, td)
    return out


def _extreme_rows(exe, td):
    """The four extreme rows of the distribution function's tests (|Nu| = 5, Eta = 3, beta .02 / .98): conditional p on a grid of 200 values
    in [1e-6, 1 - 1e-6] on both boundaries; the residual is against the header's own F at rt - tau as the solver had it."""
    rows = np.array([[5.0, 2.5, 0.5, 0.0, 3.0, 0.8], [5.0, 2.5, 0.98, 0.0, 3.0, 0.8], [-5.0, 2.5, 0.02, 0.0, 3.0, 0.8],
                     [-5.0, 2.5, 0.98, 0.0, 3.0, 0.8]], np.float32)
    grid = np.concatenate([np.geomspace(1e-6, 0.5, 100), 1.0 - np.geomspace(0.5, 1e-6, 100)]).astype(np.float32)
    m = grid.size
    params = np.repeat(rows, 2 * m, 0)
    probs = np.tile(np.stack([np.r_[grid, grid], np.r_[np.ones(m), -np.ones(m)]], 1), (4, 1))
    q, ev, F, lim = solve(exe, td, 3, 1, params, probs)
    fin = np.isfinite(q)
    return {"requests": int(q.size), "finite": int(fin.sum()), "nan": int(np.isnan(q).sum()), "evals_mean": float(ev.mean()), "evals_max": int(ev.max()),
            "max_abs_residual": float(np.max(np.abs(F - probs[:, 0].astype(np.float32).astype(np.float64) * lim)[fin]))}


def _golden_tables(exe, td):
    """tests/golden/ratcliff.npz as tests/test_gpu_wiener_quantile.py reads it: every level k / 4000, k = 40 .. 3960, not within 0.01 of
    P(lower), as a defective request on its boundary; the rank of the returned signed time in the set's 4001-point quantile table, and in
    the next set's (the control)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "ratcliff.npz"))
    sets = g["sets"].astype(np.float32)
    B = sets.shape[0]
    ks = np.arange(40, 3961, 40)
    lev = ks / 4000.0

    def signed(rows):
        _, _, _, pu = solve(exe, td, 3, 0, rows, np.stack([np.zeros(B), np.ones(B)], 1))      # (p = 0 on the upper boundary: its P comes back)
        plo = 1.0 - pu.astype(np.float64)
        upper = lev[None, :] > plo[:, None]
        p = np.where(upper, lev[None, :] - plo[:, None], plo[:, None] - lev[None, :])
        use = np.abs(lev[None, :] - plo[:, None]) > 0.01
        q, _, _, _ = solve(exe, td, 3, 0, np.repeat(rows, ks.size, 0), np.stack([p.ravel(), np.where(upper, 1.0, -1.0).ravel()], 1))
        q = q.reshape(B, ks.size).astype(np.float64)
        return np.where(upper, q, -q), use

    y, use = signed(sets)
    yx, usex = signed(np.roll(sets, -1, 0))
    own, other = [], []
    for i in range(B):
        yq = g[f"yq_s{i}"].astype(np.float64)
        own.append(int(np.max(np.abs(np.searchsorted(yq, y[i][use[i]]) - ks[use[i]]))))
        other.append(int(np.max(np.abs(np.searchsorted(yq, yx[i][usex[i]]) - ks[usex[i]]))))
    return {"sets": B, "max_rank_distance_per_set": own, "max_rank_distance": max(own), "control_next_sets_row_per_set": other,
            "control_min": min(other)}


if __name__ == "__main__":
    B.cli(survey)
