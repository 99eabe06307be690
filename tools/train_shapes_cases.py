#!/usr/bin/env python
"""Per-case figures of the batteries in tests/test_gpu_training_shapes.py: the test's own code with a yardstick whose add() prints,
per case and group, the relative rms error of the fused kernels and of PyTorch's float32 composition against float64, and their
ratio, before it asserts.  The pooled figures the tests print say which group is close to the bound; these say which case put it there.

    python tools/train_shapes_cases.py flow | deepset          (needs the GPU)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_gpu_training_shapes as shapes          # noqa: E402
import train_yardstick                             # noqa: E402


class PrintingYardstick(train_yardstick._F64Yardstick):
    def add(self, label, case, fused, plain, exact, groups):
        acc = {}
        for a, b, e, grp in zip(fused, plain, exact, groups):
            mag = float(e.pow(2).mean().sqrt()) + 1e-30
            fa, fb, n = acc.get(grp, (0.0, 0.0, 0))
            acc[grp] = (fa + float(((a.double() - e) / mag).pow(2).sum()), fb + float(((b.double() - e) / mag).pow(2).sum()), n + e.numel())
        print(label, case, {g: (f"{(fa / n) ** 0.5:.2e}", f"{(fb / n) ** 0.5:.2e}", round((fa / max(fb, 1e-300)) ** 0.5, 2))
                            for g, (fa, fb, n) in acc.items()}, flush=True)
        super().add(label, case, fused, plain, exact, groups)


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "flow"
    shapes._F64Yardstick = PrintingYardstick
    {"flow": shapes.test_fused_flow_at_every_shape_the_gate_admits, "deepset": shapes.test_fused_deepset_at_every_shape_the_gate_admits}[which]()
