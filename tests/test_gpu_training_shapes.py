"""The three training libraries (csrc/train_kernels.hip, csrc/train_deepset.hip, csrc/train_update.hip) at the shapes their gates
admit beyond the one configuration the training loop uses: every comparison against a float64 evaluation of the same operation, with
PyTorch's float32 composition as the yardstick (tests/train_yardstick.py, the constants of tests/test_gpu_training.py)."""
import copy
import math

import numpy as np
import pytest

from train_yardstick import _F64Yardstick, _flow_groups

pytestmark = pytest.mark.gpu


def _lib():
    from bayesflow_nddms_amd import _train_lib
    L = _train_lib.lib()
    assert L is not None, "libnddm_train.so did not build / load"
    return L


def _prepared_flow(D, C, layers, gen_scale=1.5):
    """An InvertibleNetwork made ill-conditioned as tests/test_gpu_training.py makes its own: weights x 1.5, ActNorms at 0.3 x randn."""
    import torch
    from bayesflow_nddms_amd.amortizer import InvertibleNetwork
    net = InvertibleNetwork(num_params=D, cond_dim=C, num_coupling_layers=layers, seed=layers).cuda()
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(gen_scale)
        for p in list(net.an_scale) + list(net.an_bias):
            p.copy_(0.3 * torch.randn_like(p))
    return net, copy.deepcopy(net).double()


def _flow_forms(wz, wl):
    import torch

    def flow(n, th, cd):
        z, ld = n(th, cd)
        g = torch.autograd.grad((z * wz.to(z.dtype)).sum() + (ld * wl.to(z.dtype)).sum(), [th, cd] + list(n.parameters()))
        return [z.detach(), ld.detach()] + [t.detach() for t in g]

    def nll(n, th, cd):                              # the loss form: gradients of z and log|det| derived inside the kernel
        loss = n.nll(th, cd)
        return [loss.detach()] + [t.detach() for t in torch.autograd.grad(3.0 * loss, [th, cd] + list(n.parameters()))]

    return flow, nll


def test_unconditional_flow_takes_the_pytorch_path():
    """InvertibleNetwork(cond_dim=0) on the device: the gate refuses it (asked on the host, before anything runs), so forward, loss and
    every gradient are PyTorch's composition -- held to the float64 copy at float32's own accuracy.  The bound: a chain of 36 small
    GEMMs (6 layers x 2 halves x 3, K <= 128) whose worst-case relative error is K u = 128 x 2^-24 = 8e-6 each, accumulating as a
    random walk: sqrt(36) x 8e-6 = 5e-5, so 1e-4 relative rms per tensor.  No fused kernel is launched with C = 0."""
    import torch
    L = _lib()
    assert L.nddm_train_flow_supported(128, 6, 5, 2, 0) == 0 and L.nddm_train_flow_supported(128, 6, 5, 2, 1) == 1
    torch.manual_seed(17)
    net, net64 = _prepared_flow(5, 0, 6)
    R = 40
    theta = torch.randn(R, 5, device="cuda", requires_grad=True)
    cond = torch.zeros(R, 0, device="cuda", requires_grad=True)
    assert net.fused and net._fused_lib(theta, cond) is None
    theta64, cond64 = theta.detach().double().requires_grad_(True), cond.detach().double().requires_grad_(True)
    flow, nll = _flow_forms(torch.randn(R, 5, device="cuda"), torch.randn(R, device="cuda"))
    for form in (flow, nll):
        for a, e in zip(form(net, theta, cond), form(net64, theta64, cond64)):
            assert a.shape == e.shape and a.dtype == torch.float32
            if e.numel():
                err = float((a.double() - e).pow(2).mean().sqrt()) / (float(e.pow(2).mean().sqrt()) + 1e-30)
                assert err <= 1e-4, (form.__name__, tuple(e.shape), err)


FLOW_CASES = ((8, 32, 8, 28), (8, 32, 8, 24), (7, 15, 8, 27), (1, 17, 2, 1), (2, 33, 5, 4), (2, 31, 5, 8), (3, 16, 6, 16), (2, 48, 7, 25),
              (4, 9, 3, 13), (5, 64, 4, 2), (1, 4096, 5, 11))


def test_fused_flow_at_every_shape_the_gate_admits():
    """csrc/train_kernels.hip beyond condition width 11 and layers {1, 2, 3, 6}: (layers, rows, D, C) with every maximum at once
    (L = 8 = L_MAX, D = 8, C = 28: DI = 32, the whole in_s tile and one weight-gradient input element per thread), DI = 31, 28 / 29 (the two
    halves differ), the smallest of everything (one layer, D = 2, C = 1), C a multiple of 4 with rows around the 16- and 32-row tiles,
    L = 4, 5, 7, and FUSED_MAX_ROWS rows (one more row falls back); one case with theta x 20 (the soft clamp's flat part, ELU's deep
    negative branch) and one with theta and the condition as column slices of wider tensors (the gradients come back in the views'
    shapes).  Both forms (z, log|det| and every gradient; the loss and every gradient) and the float64 round trip, on the yardstick of
    tests/test_gpu_training.py with its constants.
    Measured on the MI355X, pooled rms error fused / pytorch (profiles/r24_train_shapes_yardstick.txt, the same figures on two
    machines): flow form z 1.37, log|det| 0.88, d theta 1.92, d cond 1.90, d weights 1.85, d biases 1.87, d ActNorm 1.90; loss form
    1.13 / 1.93 / 1.94 / 1.88 / 1.96 / 1.97 (loss, d theta, d cond, d weights, d biases, d ActNorm); round trip 0.50.
    The gradient figures are those of ONE case, theta x 20, whose relative errors (4e-5 .. 8e-5 fused, 2e-5 .. 4e-5 PyTorch) are
    twenty to a hundred times everybody else's and so carry the pool: every gradient group of that case sits at 1.90 .. 2.01 x PyTorch,
    uniformly, while the other twelve cases are at 0.2 .. 1.8 (python tools/train_shapes_cases.py flow).  A common factor: on
    saturated log-scales the backward derives the clamp's derivative from the SAVED s = clamp * tanh(o / clamp), which carries
    the product's rounding on top of tanh's own, where PyTorch keeps tanh's output -- about twice the error of a difference,
    clamp - s, that is itself a few ulps wide.  Within the bound, close to it, and the place to look first if this test ever fails."""
    import torch
    _lib()
    torch.manual_seed(23)
    yard = _F64Yardstick()
    battery = [(c, 1.0, False) for c in FLOW_CASES] + [((2, 40, 5, 11), 20.0, False), ((2, 40, 5, 11), 1.0, True)]
    for (layers, R, D, C), theta_scale, sliced in battery:
        case = (layers, R, D, C) + (("theta x 20",) if theta_scale != 1.0 else ()) + (("views",) if sliced else ())
        net, net64 = _prepared_flow(D, C, layers)
        if sliced:                                   # non-contiguous views: a column slice of a wider tensor each
            wide_t = torch.randn(R, D + 3, device="cuda", requires_grad=True)
            wide_c = torch.randn(R, C + 5, device="cuda", requires_grad=True)
            theta, cond = wide_t[:, 1:1 + D], wide_c[:, 2:2 + C]
            assert not theta.is_contiguous() and not cond.is_contiguous()
        else:
            theta = (theta_scale * torch.randn(R, D, device="cuda")).requires_grad_(True)
            cond = torch.randn(R, C, device="cuda", requires_grad=True)
        theta64, cond64 = theta.detach().double().requires_grad_(True), cond.detach().double().requires_grad_(True)
        flow, nll = _flow_forms(torch.randn(R, D, device="cuda"), torch.randn(R, device="cuda"))
        res, nl = {}, {}
        for fused in (True, False):
            net.fused = fused
            assert (net._fused_lib(theta, cond) is not None) == fused, case
            res[fused], nl[fused] = flow(net, theta, cond), nll(net, theta, cond)
        assert net64._fused_lib(theta64, cond64) is None
        exact, exact_nl = flow(net64, theta64, cond64), nll(net64, theta64, cond64)
        for got in (res[True], nl[True]):
            assert all(bool(torch.isfinite(t).all()) for t in got), case
        assert res[True][2].shape == (R, D) and res[True][3].shape == (R, C) and nl[True][1].shape == (R, D) and nl[True][2].shape == (R, C)
        grp = _flow_groups(net)
        yard.add("flow", case, res[True], res[False], exact, ["z", "log|det|"] + grp)
        yard.add("nll", case, nl[True], nl[False], exact_nl, ["loss"] + grp)
        with torch.no_grad():                        # both f32 forwards' z through the f64 inverse: what comes back is the forward's own round-off
            back = [[net64.inverse(res[f][0].double(), cond64.detach())] for f in (True, False)]
        yard.add("round trip", case, back[0], back[1], [theta64.detach()], ["theta"])
    print("fused flow at the gate's shapes, pooled rms error fused / pytorch-f32 against f64:", yard.finish())
    # one row beyond FUSED_MAX_ROWS: the PyTorch composition
    net, _ = _prepared_flow(5, 11, 1)
    cap = net.FUSED_MAX_ROWS
    assert cap == 4096
    th, cd = torch.randn(cap + 1, 5, device="cuda"), torch.randn(cap + 1, 11, device="cuda")
    assert net._fused_lib(th, cd) is None and net._fused_lib(th[:cap], cd[:cap]) is not None
    z, ld = net(th, cd)
    assert z.shape == (cap + 1, 5) and ld.shape == (cap + 1,)


#               blocks, B, N, n_real, input_dim, summary_dim
DEEPSET_CASES = ((1, 3, 70, None, 1, 10), (2, 3, 65, 40, 3, 10), (0, 2, 5, None, 4, 10), (1, 2, 130, 129, 64, 10), (2, 3, 64, None, 64, 10),
                 (2, 65, 3, None, 2, 10), (2, 130, 70, 5, 2, 1), (1, 7, 66, 3, 2, 64), (3, 2, 65, 64, 2, 54))


def test_fused_deepset_at_every_shape_the_gate_admits():
    """csrc/train_deepset.hip beyond 2 input columns, summary width 10 and B <= 32: the small-input widths 1, 3, 4 (3: a W1 leading
    dimension of 67 in the equivariant half), 64 raw input columns (layer 1 of the first MLPs as an MFMA product), more than 64 sets
    (the post-pooling MLP over two and three workgroups, whose weight-gradient rows reduce_partials_kernel sums in its tail branch),
    B > n_real in the count form (the post-pooling launch receives the TRIAL count while its rows are the SETS), summary widths 1, 54
    and 64, a tile that is all padding, three blocks.  Mask form and count form (the fused count form equals the fused mask form bit
    for bit), both `direct` forms where summary_dim + k <= 64; at summary width 54 a 10-column `direct` stays fused and an 11-column
    one takes forward()'s concatenation.  The yardstick and constants of tests/test_gpu_training.py.
    Measured on the MI355X, pooled rms error fused / pytorch (profiles/r24_train_shapes_yardstick.txt): summary 0.81, d weights 1.04,
    d biases 1.23; with direct conditions 0.85 / 0.94 / 1.08."""
    import torch
    from bayesflow_nddms_amd.amortizer import InvariantNetwork
    _lib()
    torch.manual_seed(29)
    yard = _F64Yardstick()
    for blocks, B, N, n_real, d_in, d_sum in DEEPSET_CASES:
        case = (blocks, B, N, n_real, d_in, d_sum)
        net = InvariantNetwork(input_dim=d_in, summary_dim=d_sum, num_equiv=blocks).cuda()
        with torch.no_grad():
            for p in net.parameters():
                if p.dim() == 1:
                    p.copy_(0.1 * torch.randn_like(p))                  # non-zero biases
        net64 = copy.deepcopy(net).double()
        cols = [0.3 + torch.rand(B, N, 1, device="cuda") * 2.0]
        if d_in > 1:
            cols.append((torch.rand(B, N, 1, device="cuda") < 0.7).float())
        if d_in > 2:
            cols.append(torch.randn(B, N, d_in - 2, device="cuda"))
        x = torch.cat(cols, dim=-1).contiguous()
        assert x.shape == (B, N, d_in)
        mask = inv_n = mask64 = inv_n64 = None
        if n_real is not None:
            mask = (torch.arange(N, device="cuda") < n_real).float().view(1, N, 1)
            inv_n = torch.tensor(1.0 / n_real, device="cuda")
            mask64, inv_n64 = mask.double(), torch.tensor(1.0 / n_real, device="cuda", dtype=torch.float64)
        w = torch.randn(B, d_sum, device="cuda")

        def summary(n, xx, *a, wt=w, **kw):
            out = n(xx, *a, **kw)
            return [out.detach()] + [t.detach() for t in torch.autograd.grad((out * wt.to(out.dtype)).sum(), list(n.parameters()))]

        res = {}
        for fused in (True, False):
            net.fused = fused
            assert (net._fused_lib(x) is not None) == fused, case
            res[fused] = summary(net, x, mask, inv_n)
        assert res[True][0].shape == (B, d_sum) and all(bool(torch.isfinite(t).all()) for t in res[True]), case
        grp = ["summary"] + [("d weights" if n.endswith("weight") else "d biases") for n, _ in net.named_parameters()]
        yard.add("summary", case, res[True], res[False], summary(net64, x.double(), mask64, inv_n64), grp)
        if n_real is not None:                               # the count form of the mask (a device scalar: what the graph trainer passes)
            nv = torch.tensor([float(n_real)], device="cuda")
            for fused in (True, False):
                net.fused = fused
                out = net(x, n_valid=nv)
                g = torch.autograd.grad((out * w).sum(), list(net.parameters()))
                for a, b in zip([out.detach()] + list(g), res[fused]):
                    assert torch.equal(a, b) if fused else torch.allclose(a, b, rtol=1e-5, atol=1e-6), case
        directs = [torch.tensor([5.25], device="cuda").view(1, 1).expand(B, 1), torch.randn(B, 3, device="cuda")]
        if d_sum == 54:
            directs += [torch.randn(B, 10, device="cuda"), torch.randn(B, 11, device="cuda")]   # 54 + 10 = 64: fused; 65: forward()'s concatenation
        for direct in directs:
            k = direct.shape[1]
            if d_sum + k > 64 and d_sum != 54:
                continue
            wd = torch.randn(B, d_sum + k, device="cuda")
            got = {}
            for fused in (True, False):
                net.fused = fused
                got[fused] = summary(net, x, mask, inv_n, wt=wd, direct=direct)
                assert got[fused][0].shape == (B, d_sum + k) and torch.equal(got[fused][0][:, d_sum:], direct), (case, k)
            yard.add("direct", case + (k,), got[True], got[False], summary(net64, x.double(), mask64, inv_n64, wt=wd, direct=direct.double()), grp)
    print("fused DeepSet at the gate's shapes, pooled rms error fused / pytorch-f32 against f64:", yard.finish())


def _f32(v):
    return float(np.float32(v))


class _AdamRun:
    """nddm_train_adam_step beside a float64 Adam written out here (the reference) and clip_grad_norm_ + torch.optim.Adam in float32
    (the yardstick), all three on the same numbers: the hyper-parameters are float32 values, which is what the entry point receives."""

    def __init__(self, n, T, start=0, lr0=2e-3, clip=5.0, scale=0.5, cap=4):
        import torch
        self.L, self.n, self.T, self.lr0, self.clip, self.scale, self.cap = _lib(), n, T, _f32(lr0), clip, scale, cap
        self.b1, self.b2, self.eps, self.step = _f32(0.9), _f32(0.999), _f32(1e-8), start
        dev = "cuda"
        p0 = torch.randn(n, device=dev)
        m0 = 0.01 * torch.randn(n, device=dev) if start else torch.zeros(n, device=dev)
        v0 = 1e-4 * torch.rand(n, device=dev) + 1e-6 if start else torch.zeros(n, device=dev)
        self.p, self.m, self.v = p0.clone(), m0.clone(), v0.clone()
        self.p64, self.m64, self.v64 = p0.double(), m0.double(), v0.double()
        self.ref = torch.nn.Parameter(p0.clone())
        self.opt = torch.optim.Adam([self.ref], lr=self.lr0, betas=(self.b1, self.b2), eps=self.eps)
        if start:
            self.opt.state[self.ref] = {"step": torch.tensor(float(start)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
        self.g = torch.zeros(n + 1, device=dev)
        self.partial = torch.zeros(256 + 4, device=dev)       # (+ the ticket word of the update kernel: zero between launches)
        self.step_i = torch.full((1,), start, dtype=torch.int64, device=dev)
        self.step_f = torch.full((1,), float(start), device=dev)
        self.lr_out, self.loss_buf = torch.zeros((), device=dev), torch.zeros(cap, device=dev)

    def rate(self):
        return 0.5 * self.lr0 * (1.0 + math.cos(min(self.step, self.T) * math.pi / self.T))

    def run_step(self, grad, loss):
        import torch
        n, lr, t = self.n, self.rate(), self.step + 1
        self.g[:n].copy_(grad)
        self.g[n] = loss
        # float64: clip_grad_norm_'s rule, the cosine rate, Adam with its bias corrections
        g64 = grad.double() * self.scale
        norm = float(g64.pow(2).sum().sqrt())
        g64 = g64 * min(self.clip / (norm + 1e-6), 1.0)
        self.m64 = self.m64 + (g64 - self.m64) * (1.0 - self.b1)
        self.v64 = self.b2 * self.v64 + (1.0 - self.b2) * g64 * g64
        bc1, bc2 = 1.0 - self.b1 ** t, 1.0 - self.b2 ** t
        self.p64 = self.p64 - (lr / bc1) * self.m64 / (self.v64.sqrt() / math.sqrt(bc2) + self.eps)
        # float32 PyTorch
        for grp in self.opt.param_groups:
            grp["lr"] = lr
        self.ref.grad = grad * self.scale
        torch.nn.utils.clip_grad_norm_([self.ref], self.clip)
        self.opt.step()
        rc = self.L.nddm_train_adam_step(self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), n, self.partial.data_ptr(),
                                         self.scale, self.clip, self.lr0, float(self.T), self.b1, self.b2, self.eps, self.step_i.data_ptr(),
                                         self.step_f.data_ptr(), self.lr_out.data_ptr(), self.loss_buf.data_ptr(), self.cap,
                                         self.g[n:].data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        self.step += 1
        return norm, lr

    def triple(self):
        st = self.opt.state[self.ref]
        return [self.p, self.m, self.v], [self.ref.detach(), st["exp_avg"], st["exp_avg_sq"]], [self.p64, self.m64, self.v64]


ADAM_SIZES = (4, 1020, 262144 + 8, 1048576 + 1028)


def test_flat_adam_step_equals_float64_at_every_trip_count():
    """csrc/train_update.hip: parameters AND both moments after 6 steps (the first three clipped) against a float64 Adam, PyTorch's
    float32 clip_grad_norm_ + Adam as the yardstick, for n = 4 (one thread's worth), 1 020 (one workgroup, not full), 262 144 + 8 (the
    norm kernel's grid-stride loop takes a second trip) and 1 048 576 + 1 028 (the update kernel's does, its grid capped at 1 024
    workgroups).  Measured on the MI355X, pooled rms error kernel / pytorch (profiles/r24_train_shapes_yardstick.txt): p 1.00, m 0.98,
    v 1.09."""
    import torch
    torch.manual_seed(31)
    yard = _F64Yardstick()
    for n in ADAM_SIZES:
        run = _AdamRun(n, T=50)
        for it in range(6):
            big = it < 3
            grad = torch.randn(n, device="cuda") * (30.0 if big else 1e-3)
            norm, lr = run.run_step(grad, float(it + 1))
            assert (norm > run.clip) == big, (n, it, norm)                  # clipped at first, then not
            assert abs(float(run.lr_out) - lr) < 1e-9 and int(run.step_i) == it + 1 and float(run.step_f) == it + 1
        fused, plain, exact = run.triple()
        assert all(bool(torch.isfinite(t).all()) for t in fused) and float(run.partial[256]) == 0.0
        yard.add("adam", (n,), fused, plain, exact, ["p", "m", "v"])
        assert run.loss_buf.tolist() == [2.5, 3.0, 1.5, 2.0]                 # scaled losses in a ring of 4
    print("flat Adam step, pooled rms error kernel / pytorch-f32 against f64:", yard.finish())


def test_flat_adam_step_at_a_large_step_count():
    """step_i = step_f = 1 000 000 of total_steps = 2 000 000: ipow's bias corrections (beta2^1e6 by repeated squaring) and the float32
    cosine argument against float64 -- parameters and moments on the yardstick, and the counters, the reported rate and the loss ring
    as in tests/test_gpu_training.py.  Measured on the MI355X, pooled rms error kernel / pytorch
    (profiles/r24_train_shapes_yardstick.txt): p 1.00, m 0.78, v 0.98."""
    import torch
    torch.manual_seed(37)
    start, T, n = 1_000_000, 2_000_000, 4104
    run = _AdamRun(n, T=T, start=start)
    yard = _F64Yardstick()
    for it in range(6):
        grad = torch.randn(n, device="cuda") * (3.0 if it < 3 else 0.01)
        norm, lr = run.run_step(grad, float(it + 1))
        assert (norm > run.clip) == (it < 3)
        assert abs(float(run.lr_out) - lr) < 1e-9, (it, float(run.lr_out), lr)
        assert int(run.step_i) == start + it + 1 and float(run.step_f) == start + it + 1
    fused, plain, exact = run.triple()
    yard.add("adam at step 1e6", (n,), fused, plain, exact, ["p", "m", "v"])
    print("flat Adam step at step 1e6, pooled rms error kernel / pytorch-f32 against f64:", yard.finish())
    # slot (start + it) mod 4 holds scale x loss: 1e6 mod 4 == 0, steps 4 and 5 wrapped
    assert run.loss_buf.tolist() == [2.5, 3.0, 1.5, 2.0]


def test_flat_adam_step_with_an_all_zero_gradient():
    """An all-zero gradient (norm 0: the clip coefficient is min(clip / 1e-6, 1) = 1) from fresh moments leaves the parameters as they
    are, bit for bit, and nothing becomes non-finite."""
    import torch
    torch.manual_seed(41)
    for n in (4, 4104):
        run = _AdamRun(n, T=50)
        p0 = run.p.clone()
        for it in range(2):
            run.run_step(torch.zeros(n, device="cuda"), 0.0)
        assert torch.equal(run.p, p0)
        for t in (run.p, run.m, run.v, run.lr_out, run.loss_buf, run.step_f):
            assert bool(torch.isfinite(t).all())
        assert float(run.m.abs().max()) == 0.0 and float(run.v.abs().max()) == 0.0 and int(run.step_i) == 2


GUARD = -777.25


def test_stage_equals_copy_and_touches_nothing_else():
    """nddm_train_stage (the head of every pipelined iteration: the produced batch into the tensors the training graph reads, N and log N
    into their device scalars, one launch): bit-equal to Tensor.copy_ for either destination empty, the longer one first and second,
    and the training loop's own sizes, with n2 given and NULL; guard words after both destinations, and in n2 when it is not passed,
    stay as they were.  A count that is no multiple of 4, a misaligned pointer and a NULL with a non-zero count are refused."""
    import torch
    L = _lib()
    torch.manual_seed(43)
    st = torch.cuda.current_stream().cuda_stream
    for n_a, n_b in ((0, 4), (4, 0), (1024, 1028), (1028, 1024), (9600 * 2, 32 * 8)):
        for with_n2 in (True, False):
            src_a, src_b = torch.randn(n_a + 4, device="cuda"), torch.randn(n_b + 4, device="cuda")
            dst_a, dst_b = torch.full((n_a + 4,), GUARD, device="cuda"), torch.full((n_b + 4,), GUARD, device="cuda")
            want_a, want_b = dst_a.clone(), dst_b.clone()
            want_a[:n_a].copy_(src_a[:n_a]); want_b[:n_b].copy_(src_b[:n_b])
            n2 = torch.full((4,), GUARD, device="cuda")
            rc = L.nddm_train_stage(dst_a.data_ptr(), src_a.data_ptr(), n_a, dst_b.data_ptr(), src_b.data_ptr(), n_b,
                                    n2.data_ptr() if with_n2 else None, 137.0, math.log(137.0), st)
            assert rc == 0, (n_a, n_b, with_n2)
            assert torch.equal(dst_a, want_a) and torch.equal(dst_b, want_b), (n_a, n_b, with_n2)
            want_n2 = [_f32(137.0), _f32(math.log(137.0)), GUARD, GUARD] if with_n2 else [GUARD] * 4
            assert n2.tolist() == want_n2, (n_a, n_b, with_n2)
    a, b = torch.zeros(16, device="cuda"), torch.zeros(16, device="cuda")
    pa, pb = a.data_ptr(), b.data_ptr()
    assert L.nddm_train_stage(pa, pb, 6, pa, pb, 0, None, 1.0, 0.0, st) == 1          # a count that is not a multiple of 4
    assert L.nddm_train_stage(pa, pb, 4, pa, pb, 6, None, 1.0, 0.0, st) == 1
    assert L.nddm_train_stage(pa + 4, pb, 4, pa, pb, 4, None, 1.0, 0.0, st) == 1      # misaligned pointers
    assert L.nddm_train_stage(pa, pb, 4, pa, pb + 8, 4, None, 1.0, 0.0, st) == 1
    assert L.nddm_train_stage(None, pb, 4, pa, pb, 4, None, 1.0, 0.0, st) == 1        # NULL with a non-zero count
    assert L.nddm_train_stage(pa, pb, 4, pa, None, 4, None, 1.0, 0.0, st) == 1
    assert L.nddm_train_stage(pa, pb, -4, pa, pb, 4, None, 1.0, 0.0, st) == 1
    torch.cuda.synchronize()
    assert float(a.abs().max()) == 0.0 and float(b.abs().max()) == 0.0                # a refused call wrote nothing


def test_set2_writes_exactly_two_floats():
    """nddm_train_set2: dst[0] = a, dst[1] = b, and the word after them stays put; NULL is refused."""
    import torch
    L = _lib()
    st = torch.cuda.current_stream().cuda_stream
    dst = torch.full((4,), GUARD, device="cuda")
    assert L.nddm_train_set2(dst.data_ptr(), 237.0, math.log(237.0), st) == 0
    assert dst.tolist() == [_f32(237.0), _f32(math.log(237.0)), GUARD, GUARD]
    assert L.nddm_train_set2(None, 1.0, 2.0, st) == 1
    assert dst.tolist() == [_f32(237.0), _f32(math.log(237.0)), GUARD, GUARD]
