#!/usr/bin/env python3
"""What the flow's log density costs the fused sampler (csrc/train_sample.hip), against another build of libnddm_train.so -- the parent
commit's -- in ONE process, the legs alternating, at the default network (6 layers, D = 5, C = 11) and (B = 1, S = 10 000), (B = 20,
S = 10 000):
    parent       nddm_train_flow_sample of --parent (draws only)
    control      the same library again: what two sets of calls of ONE code differ by
    new_off      this tree's nddm_train_flow_sample: log_q not asked for (flow_sample_kernel)
    new_on       this tree's nddm_train_flow_sample_logq: draws and log_q (flow_sample_logq_kernel)
Timing: device events around each call (the prologue kernel, a few microseconds, included) after a warm-up of every leg, the median,
minimum and maximum of --reps calls per leg.  The bar: new_off's median inside the control's min .. max.
Bit equality: sha256 of theta, sums and n_outside on one seeded input (B = 3, S = 1000, a box at +-1) from the parent, from new_off and
from new_on.

Usage: python tools/flow_importance_ab.py --parent /path/to/parent/libnddm_train.so [--out profiles/r31_flow_importance_ab.txt] [--reps 40]
"""
import argparse
import ctypes
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=40)
    a = ap.parse_args()
    import torch
    from bayesflow_nddms_amd import _train_lib, engine
    from bayesflow_nddms_amd.amortizer import InvertibleNetwork
    engine.require_device()
    new = _train_lib.lib()
    assert new is not None, "libnddm_train.so did not build or load"
    old = ctypes.CDLL(os.path.abspath(a.parent))
    old.nddm_train_flow_sample.argtypes, old.nddm_train_flow_sample.restype = new.nddm_train_flow_sample.argtypes, ctypes.c_int
    torch.manual_seed(0)
    net = InvertibleNetwork(num_params=5).cuda().eval()
    params = net._flow_params()
    ptrs = (ctypes.c_void_p * (14 * 6))(*[p.data_ptr() for p in params])
    perm = (ctypes.c_int * 30)(*[int(v) for p in net._perm_host for v in p])
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda v: None if v is None else v.data_ptr()       # noqa: E731

    works = {(B, S): torch.empty(int(new.nddm_train_flow_sample_work_bytes(B, S, 5)), dtype=torch.uint8, device="cuda")
             for B, S in ((1, 10_000), (20, 10_000), (3, 1000))}

    def call(lib, z, cond, theta, box, sums, n_out, log_q):
        B, S, D = z.shape
        work = works[(B, S)]
        head = (128, 6, B, S, D, 2, 11, 1.9, ptrs, perm, z.data_ptr(), cond.data_ptr(), ptr(theta), ptr(box and box[0]), ptr(box and box[1]),
                ptr(sums), ptr(n_out))
        rc = lib.nddm_train_flow_sample_logq(*head, log_q.data_ptr(), work.data_ptr(), st) if log_q is not None else \
            lib.nddm_train_flow_sample(*head, work.data_ptr(), st)
        assert rc == 0, rc

    lines = ["tools/flow_importance_ab.py: the fused sampler with and without log_q against the parent's library, one process, legs "
             f"alternating, device events, {a.reps} calls per leg; microseconds: median  min .. max", f"device: {torch.cuda.get_device_name(0)}"]
    for B, S in ((1, 10_000), (20, 10_000)):
        z, cond = torch.randn(B, S, 5, device="cuda"), torch.randn(B, 11, device="cuda")
        theta, log_q = torch.empty(B, S, 5, device="cuda"), torch.empty(B, S, device="cuda")
        legs = {"parent": lambda: call(old, z, cond, theta, None, None, None, None), "control": lambda: call(old, z, cond, theta, None, None, None, None),
                "new_off": lambda: call(new, z, cond, theta, None, None, None, None), "new_on": lambda: call(new, z, cond, theta, None, None, None, log_q)}
        for fn in legs.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in legs}
        for _ in range(a.reps):
            for k, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                us[k].append(1e3 * e0.elapsed_time(e1))
        med = {k: float(np.median(v)) for k, v in us.items()}
        for k, v in us.items():
            lines.append(f"B={B:3d} S={S} {k:8s} {med[k]:9.2f}  {min(v):9.2f} .. {max(v):9.2f}   / parent {med[k] / med['parent']:.4f}")
        inside = min(us["control"]) <= med["new_off"] <= max(us["control"])
        lines.append(f"B={B:3d} S={S} new_off's median inside the control's min .. max: {'yes' if inside else 'NO'};  "
                     f"control / parent {med['control'] / med['parent']:.4f}, new_off / parent {med['new_off'] / med['parent']:.4f}, "
                     f"new_on / new_off {med['new_on'] / med['new_off']:.4f}")
    torch.manual_seed(1)
    B, S = 3, 1000
    z, cond = torch.randn(B, S, 5, device="cuda"), torch.randn(B, 11, device="cuda")
    box = (torch.full((5,), -1.0, device="cuda"), torch.full((5,), 1.0, device="cuda"))
    digests = {}
    for k, lib, on in (("parent", old, False), ("new_off", new, False), ("new_on", new, True)):
        theta, sums, n_out = torch.empty(B, S, 5, device="cuda"), torch.empty(B, 10, dtype=torch.float64, device="cuda"), torch.empty(B, dtype=torch.int64, device="cuda")
        call(lib, z, cond, theta, box, sums, n_out, torch.empty(B, S, device="cuda") if on else None)
        torch.cuda.synchronize()
        digests[k] = {n: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for n, t in (("theta", theta), ("sums", sums), ("n_outside", n_out))}
        lines.append(f"sha256 {k:8s} " + "  ".join(f"{n} {h}" for n, h in digests[k].items()))
    lines.append(f"the three agree: {'yes' if digests['parent'] == digests['new_off'] == digests['new_on'] else 'NO'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
