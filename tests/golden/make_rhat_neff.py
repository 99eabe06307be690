#!/usr/bin/env python3
"""Writes tests/golden/rhat_neff.npz: a small recorded array of chains in the reference's JAGS-sample layout and what the reference's own
`diagnostic` (pyhddmjagsutils.py) reports for it -- the known answers of diagnostics.rhat_neff.  The input is made here (autoregressive
chains of several strengths, one variable with a chain offset so that Rhat is well above 1); the reference module is imported from the
directory NDDM_REFERENCE names and only called.  Run once where the reference is mounted; the tests read the file."""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def make_input():
    rng = np.random.default_rng(2024)
    n, m = 120, 4
    phi = np.array([[0.0, 0.5], [0.9, -0.3], [0.7, 0.2]])              # a [3, 2] variable
    x = np.zeros((3, 2, n, m))
    e = rng.standard_normal((3, 2, n, m))
    for t in range(n):
        x[:, :, t, :] = (phi[..., None] * x[:, :, t - 1, :] if t else 0.0) + e[:, :, t, :]
    x[2, 1] += np.arange(m) * 0.8                                       # chains that disagree
    return {"theta": x, "vector": x[0, :1] * 2.0 + 1.0}      # (the reference needs a leading dimension)


def main():
    sys.path.insert(0, os.environ.get("NDDM_REFERENCE", ""))
    import pyhddmjagsutils as phju
    inp = make_input()
    with contextlib.redirect_stdout(io.StringIO()):
        res = phju.diagnostic(inp)
    out = {}
    for k, v in inp.items():
        out[f"in_{k}"] = v
        for stat in ("rhat", "neff", "mean", "std"):
            out[f"{stat}_{k}"] = np.asarray(res[k][stat], dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "rhat_neff.npz"), **out)


if __name__ == "__main__":
    main()
