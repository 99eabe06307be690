#!/usr/bin/env python3
"""A/B of nddm::ratcliff_kernel at the bench leg's shape (1M sets x 300 trials): ANOTHER build of the library -- the parent commit's,
say -- against this tree's, both modes, 16 timed launches each, interleaved launch by launch in one process so that both see the
same clocks.  Prints each side's median and launch-to-launch spread.
Usage: python tools/ratcliff_ab.py --other /path/to/other/libnddm_hip.so [--json profiles/NAME.json]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from bayesflow_nddms_amd import _lib, priors  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--other", required=True, help="the library to compare with (built from another commit)")
ap.add_argument("--json", default=None)
args = ap.parse_args()
new = _lib.lib()
par = ctypes.CDLL(os.path.abspath(args.other))
_lib._declare(par)
print("# this tree", new.nddm_source_hash().decode()[:16], "other", par.nddm_source_hash().decode()[:16], flush=True)
B, N = 1_000_000, 300
p = torch.as_tensor(priors.alpha_ns_prior_matrix(B, 2023)).cuda()
tr = torch.empty((B, N, 2), dtype=torch.float32, device="cuda")
sm = torch.empty((B, 10), dtype=torch.float32, device="cuda")
st = torch.cuda.current_stream().cuda_stream
res = {"shape": [B, N], "launches": 16, "this_tree": new.nddm_source_hash().decode()[:16], "other": par.nddm_source_hash().decode()[:16]}
for fast in (True, False):
    def run(L, i):
        rc = L.nddm_simulratcliff(p.data_ptr(), B, N, 2023, i * B, 1 if fast else 0, 0.0, 0, tr.data_ptr(), sm.data_ptr(), None, st)
        assert rc == 0, rc
    for i in range(4):
        run(par, i); run(new, i)
    torch.cuda.synchronize()
    ms = {"other": [], "this_tree": []}
    for i in range(16):
        for name, L in (("other", par), ("this_tree", new)) if i % 2 == 0 else (("this_tree", new), ("other", par)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); run(L, 10 + i); e1.record(); torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    s = sm.cpu().numpy()
    out = {}
    for name, v in ms.items():
        v = np.array(v)
        out[name] = {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max()),
                     "q25_ms": float(np.percentile(v, 25)), "q75_ms": float(np.percentile(v, 75)), "all_ms": [round(float(x), 4) for x in v]}
        print("fast " if fast else "exact", name, {k: round(x, 4) for k, x in out[name].items() if k != "all_ms"}, flush=True)
    out["n_missing_total_last_launch"] = float(s[:, 2].sum())
    res["fast" if fast else "exact"] = out
if args.json:
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)
