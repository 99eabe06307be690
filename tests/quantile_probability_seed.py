#!/usr/bin/env python3
"""How the seed of tests/test_gpu_wiener_quantile.py::test_quantile_probability_on_the_exact_sampler (QP_SEED) was chosen, without a GPU
and with the quantile kernel out of the loop.  That test draws 4 sets x 20 000 trials from the exact sampler and asks that the share of a
boundary's observed response times at or below each predicted quantile be within 0.005 N / n of its level.  At that trial count the bar
is about two standard deviations of the SAMPLE's own noise, so a sample drawn blindly misses it about every other time whatever
produced the quantiles.  This script makes that statement checkable: for each seed it draws the sample with the sampler's CPU
restatement (oracle.philox_ratcliff, which nddm_simulratcliff with fast=False equals bit for bit), takes the quantiles from the FLOAT64
YARDSTICK (tests/wiener_cdf_ref.py, bisected in log t), and prints the worst deviation as a share of its bar, per boundary.  The seed
used is the first of 1, 2, 3, ... whose worst share is at most 0.7.

Usage: python tests/quantile_probability_seed.py [--seeds 12]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PROBS = np.array((.1, .3, .5, .7, .9))
# the test's four parameter sets (Nu, Alpha, Beta, Tau, Eta, Varsigma) and trial count
SETS = np.array([[0.3, 1.2, 0.5, 0.3, 0.5, 1.0], [-0.2, 1.5, 0.5, 0.2, 0.0, 1.1], [0.1, 0.9, 0.55, 0.4, 1.0, 0.9], [-0.4, 1.1, 0.55, 0.25, 0.3, 1.0]],
                np.float32)
N = 20_000
MARGIN = 0.7


def yardstick_quantiles():
    """float64 response-time quantiles of each boundary's own responses, [4, 2, Q]: lower, upper."""
    import wiener_cdf_ref as C
    a, v, beta, tau, s, eta = C.row_columns(SETS)
    pu = C.p_upper(a, v, beta, s, eta)
    out = np.zeros((SETS.shape[0], 2, PROBS.size))
    for side in (0, 1):
        up = np.full(SETS.shape[0], bool(side))
        Pb = np.where(up, pu, 1.0 - pu)
        for j, p in enumerate(PROBS):
            lo, hi = np.full(SETS.shape[0], 1e-8), np.full(SETS.shape[0], 1e4)
            for _ in range(80):
                mid = np.sqrt(lo * hi)
                below = C.cdf(mid, up, a, v, beta, s, eta) < p * Pb
                lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
            out[:, side, j] = tau + np.sqrt(lo * hi)
    return out


def shares_of_the_bar(seed, yard):
    """Worst |m / n - p| over the five levels as a share of 0.005 N / n, for the eight (set, boundary) pairs."""
    import oracle
    y = oracle.philox_ratcliff(SETS, N, seed=seed, set_offset=0, want_summary=False, threads=8)["trials"][..., 0].astype(np.float64)
    out = []
    for b in range(SETS.shape[0]):
        for side, rts in ((0, -y[b][y[b] < 0]), (1, y[b][y[b] > 0])):
            n = len(rts)
            out.append(max(abs((rts <= yard[b, side, j]).sum() / n - PROBS[j]) for j in range(PROBS.size)) / (0.005 * N / n))
    return np.array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=12)
    a = ap.parse_args()
    yard = yardstick_quantiles()
    chosen, misses = None, 0
    for seed in range(1, a.seeds + 1):
        sh = shares_of_the_bar(seed, yard)
        misses += sh.max() > 1.0
        if chosen is None and sh.max() <= MARGIN:
            chosen = seed
        print(f"seed {seed}: worst deviation / bar {sh.max():.3f}   per boundary {np.round(sh, 2)}", flush=True)
    print(f"{misses} of {a.seeds} seeds miss the bar against the yardstick's own quantiles; first seed within {MARGIN} of it: {chosen}")


if __name__ == "__main__":
    main()
