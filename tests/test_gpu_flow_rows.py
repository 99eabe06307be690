"""Three bit-for-bit promises of csrc/train_kernels.hip that the float64 yardsticks cannot see: a row of the flow depends on its
own row only (whichever tile and MFMA row it sits in), the loss form is the flow form on the gradients the loss implies, and no
store leaves its buffer (the RowBuf range check and the `row < R` guards).  The networks are made ill-conditioned as
tests/test_gpu_training_shapes.py makes its own."""
import ctypes

import pytest

from test_gpu_training_shapes import _lib, _prepared_flow

pytestmark = pytest.mark.gpu

#        (layers, R, D, C): DI 13 and 14 (both bank layouts of layer 1 in one network), tiles of 16, 16 and 1 rows; the smallest of
#        everything; L_MAX, D_MAX, M = 8, exactly one full tile; one row, DI odd in both halves
CASES = ((2, 33, 5, 11), (1, 17, 2, 1), (8, 16, 8, 24), (3, 1, 6, 4))
_NETS = {}


def _net(case):
    """One network per case, shared by the tests and left unchanged."""
    import torch
    if case not in _NETS:
        layers, R, D, C = case
        torch.manual_seed(100 + layers)
        net, _ = _prepared_flow(D, C, layers)
        _NETS[case] = (net, torch.randn(R, D, device="cuda"), torch.randn(R, C, device="cuda"),
                       torch.randn(R, D, device="cuda"), torch.randn(R, device="cuda"))
    return _NETS[case]


def _flow_rows(net, theta, cond, g_z, g_ld):
    """z, log|det|, d theta, d cond of the flow form: everything that is a function of a row alone."""
    import torch
    th, cd = theta.clone().requires_grad_(True), cond.clone().requires_grad_(True)
    assert net._fused_lib(th, cd) is not None
    z, ld = net(th, cd)
    g_th, g_cd = torch.autograd.grad([z, ld], [th, cd], grad_outputs=[g_z.contiguous(), g_ld.contiguous()])
    return [z.detach().clone(), ld.detach().clone(), g_th, g_cd]


@pytest.mark.parametrize("case", CASES, ids=str)
def test_a_row_depends_on_its_own_row_only(case):
    """The same rows rolled by 5 positions (another tile, another MFMA row) and the first, the 17th and the last row each alone give,
    row for row, the bits of one launch over all R rows.  (The weight gradients sum over the rows and are not part of this.)"""
    import torch
    _lib()
    net, theta, cond, g_z, g_ld = _net(case)
    R = case[1]
    full = _flow_rows(net, theta, cond, g_z, g_ld)
    idx = torch.roll(torch.arange(R, device="cuda"), 5)
    rolled = _flow_rows(net, theta[idx], cond[idx], g_z[idx], g_ld[idx])
    for name, a, b in zip(("z", "log|det|", "d theta", "d cond"), rolled, full):
        assert torch.equal(a, b[idx]), (case, "rolled", name, int((a != b[idx]).sum()))
    for r in sorted({0, 16, R - 1}):
        if r >= R:
            continue
        alone = _flow_rows(net, theta[r:r + 1], cond[r:r + 1], g_z[r:r + 1], g_ld[r:r + 1])
        for name, a, b in zip(("z", "log|det|", "d theta", "d cond"), alone, full):
            assert torch.equal(a, b[r:r + 1]), (case, "row alone", r, name)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_the_loss_form_is_the_flow_form_on_the_gradients_it_implies(case):
    """With g the gradient of the loss, the kernel derives g_ld = -g / (float)R and g_z = z * (g / R) itself (one division, one
    multiply) and the weight-gradient kernel reads the g_ld the chain kernel wrote: the flow form fed those very numbers -- computed
    in float32 by torch, the division by a TENSOR (a division by a Python scalar becomes a product with its reciprocal) -- runs
    identical code on identical numbers.  Equal bits for theta, the condition and every parameter."""
    import torch
    _lib()
    net, theta, cond, _, _ = _net(case)
    R = case[1]
    params = list(net.parameters())
    g = torch.tensor(3.0, device="cuda")
    th, cd = theta.clone().requires_grad_(True), cond.clone().requires_grad_(True)
    assert net._fused_lib(th, cd) is not None
    by_loss = torch.autograd.grad(net.nll(th, cd), [th, cd] + params, grad_outputs=g)
    z, ld = net(th, cd)
    g_over_r = g / torch.tensor(float(R), device="cuda")
    g_z, g_ld = z.detach() * g_over_r, (-g_over_r).expand(R).contiguous()
    by_flow = torch.autograd.grad([z, ld], [th, cd] + params, grad_outputs=[g_z, g_ld])
    names = ["d theta", "d cond"] + [n for n, _ in net.named_parameters()]
    for name, a, b in zip(names, by_loss, by_flow):
        assert a.shape == b.shape and torch.equal(a, b), (case, name, int((a != b).sum()))


SENTINEL, TAIL = -777.25, 4096


def test_nothing_escapes_the_buffers():
    """nddm_train_flow_fwd and nddm_train_flow_bwd through the C ABI at (2, 33, 5, 11) -- 15 dropped rows in the last tile -- with every
    output and scratch buffer pre-filled with a finite sentinel and followed by a tail of 4096 floats: every tail stays untouched,
    and within the buffers no element of the saved tensors, log|det|, the two input gradients or any parameter gradient still
    holds the sentinel."""
    import torch
    L = _lib()
    case = CASES[0]
    net, theta, cond, g_z, g_ld = _net(case)
    nl, R, D, C = case
    Hd, d1 = 128, net.layers[0].d1
    params = [p.detach() for p in net._flow_params()]
    assert len(params) == 14 * nl

    def buf(n):
        return torch.full((n + TAIL,), SENTINEL, dtype=torch.float32, device="cuda")

    sizes = {"z_all": nl * R * D, "out_all": nl * R * D, "s_all": nl * R * D, "h_all": nl * 4 * R * Hd, "ld": R, "gz_all": nl * R * D,
             "gx": R * D, "gcond": R * C, "work": 2 * nl * R * (2 * Hd + 16)}
    bufs = {k: buf(n) for k, n in sizes.items()}
    grads = [buf(p.numel()) for p in params]
    ptrs = (ctypes.c_void_p * (14 * nl))(*[p.data_ptr() for p in params])
    gptr = (ctypes.c_void_p * (14 * nl))(*[t.data_ptr() for t in grads])
    perm = (ctypes.c_int * (nl * D))(*[int(v) for p in net._perm_host for v in p])
    st = torch.cuda.current_stream().cuda_stream
    b = {k: t.data_ptr() for k, t in bufs.items()}
    g_z, g_ld = g_z.contiguous(), g_ld.clone()
    rc = L.nddm_train_flow_fwd(nl, R, D, d1, C, float(net.layers[0].clamp), ptrs, perm, theta.data_ptr(), cond.data_ptr(), b["z_all"],
                               b["out_all"], b["s_all"], b["h_all"], b["ld"], None, st)
    assert rc == 0
    rc = L.nddm_train_flow_bwd(nl, R, D, d1, C, float(net.layers[0].clamp), ptrs, perm, gptr, theta.data_ptr(), cond.data_ptr(), b["z_all"],
                               b["out_all"], b["s_all"], b["h_all"], g_z.data_ptr(), g_ld.data_ptr(), None, b["gz_all"], b["gx"],
                               b["gcond"], b["work"], st)
    assert rc == 0
    torch.cuda.synchronize()
    for k, t in list(bufs.items()) + [(f"grad {i}", t) for i, t in enumerate(grads)]:
        n = t.numel() - TAIL
        assert bool((t[n:] == SENTINEL).all()), (k, "tail touched", int((t[n:] != SENTINEL).sum()))
        if k not in ("gz_all", "work"):
            assert bool(torch.isfinite(t[:n]).all()) and not bool((t[:n] == SENTINEL).any()), (k, "unwritten", int((t[:n] == SENTINEL).sum()))
    z, ld = net(theta, cond)                              # the same launch through the autograd node: the buffers hold its results
    assert torch.equal(bufs["out_all"][(nl - 1) * R * D:nl * R * D].view(R, D), z) and torch.equal(bufs["ld"][:R], ld)
