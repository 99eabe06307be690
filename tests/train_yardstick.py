"""The yardstick of the fused training kernels' tests (tests/test_gpu_training.py, tests/test_gpu_training_shapes.py): a float64
evaluation of the same network is the reference, PyTorch's float32 composition the measure of what float32 can give."""


class _F64Yardstick:
    """The bound of the fused-kernel tests: an f64 evaluation of the SAME network is the reference, PyTorch's own f32 composition the
    yardstick.  Two f32 evaluations of one function differ from f64 by round-off of the same size but not of the same VALUE, and the
    error of a 5-element gradient of ONE random network is a noisy statistic (a ratio of two chi variables with 5 degrees of freedom);
    so errors are pooled: per GROUP of tensors (an output of its own; all weight-matrix / all bias / all ActNorm gradients; each
    tensor's error divided by its own f64 RMS magnitude, so that layers and cases of different scale pool sensibly) over ALL cases of
    the test's battery,

        rms(fused - f64) <= 2 * rms(pytorch f32 - f64) + 32 * 2^-24        at finish()

    and within each single case no group may be off by more than `outlier` x (+ the same few ulps): add() asserts it."""

    def __init__(self, factor=2.0, outlier=8.0, ulps=32.0):
        self.factor, self.outlier, self.tiny, self.pool = factor, outlier, ulps * 2.0 ** -24, {}

    def add(self, label, case, fused, plain, exact, groups):
        acc = {}
        for a, b, e, grp in zip(fused, plain, exact, groups):
            mag = float(e.pow(2).mean().sqrt()) + 1e-30
            fa, fb, n = acc.get(grp, (0.0, 0.0, 0))
            acc[grp] = (fa + float(((a.double() - e) / mag).pow(2).sum()), fb + float(((b.double() - e) / mag).pow(2).sum()), n + e.numel())
        for grp, (fa, fb, n) in acc.items():
            ra, rb = (fa / n) ** 0.5, (fb / n) ** 0.5
            assert ra <= self.outlier * rb + self.tiny, (label, case, grp, "relative rms fused - f64", ra, "pytorch f32 - f64", rb)
            pa, pb, pn = self.pool.get((label, grp), (0.0, 0.0, 0))
            self.pool[(label, grp)] = (pa + fa, pb + fb, pn + n)

    def finish(self):
        """-> {label: group: ratio of the pooled rms errors fused / pytorch}; asserts the 2 x bound on every group."""
        out = {}
        for (label, grp), (fa, fb, n) in self.pool.items():
            ra, rb = (fa / n) ** 0.5, (fb / n) ** 0.5
            out[f"{label}: {grp}"] = round(ra / max(rb, 1e-30), 3)
            assert ra <= self.factor * rb + self.tiny, (label, grp, "pooled relative rms fused - f64", ra, "pytorch f32 - f64", rb)
        return out


def _flow_groups(net):
    """Group names of [theta, cond] + net.parameters() gradients: weight matrices, biases and the ActNorm's pooled over the layers."""
    return ["d theta", "d cond"] + [("d ActNorm" if n.startswith("an_") else "d weights" if n.endswith("weight") else "d biases")
                                    for n, _ in net.named_parameters()]
