"""csrc/train_deepset.hip: the kernels that run two MLPs in one launch (nddm_deepset_mlp2_fwd, nddm_deepset_mlp2_bwd) write what two
launches of the single kernels write, BIT FOR BIT -- the promise of their C comments, which the float64 yardsticks of
tests/test_gpu_training*.py cannot see.  Straight through the C ABI with raw pointers; every output buffer of every launch is
pre-filled with a finite sentinel and compared whole (torch.equal), so a missing or a stray store shows as well."""
import itertools

import pytest

pytestmark = pytest.mark.gpu

HS, SENTINEL = 64, 7.0
#          B, N: one full tile and one of 6 rows per set (S = 2); one row (S = 1)
SHAPES = ((2, 70), (1, 1))
D_INS = (2, 64)                         # A's / Y's input: the small path and the MFMA path
MASKS = ("none", "mask", "count")       # no mask; a 0/1 mask with 40 real trials (the second tile is all padding); the count form of it
N_REAL = 40


def _lib():
    from bayesflow_nddms_amd import _train_lib
    L = _train_lib.lib()
    assert L is not None, "libnddm_train.so did not build / load"
    return L


def _p(t):
    return None if t is None else t.data_ptr()


def _mlp(torch, ldw1):
    """W1 [64, ldw1], b1, W2, b2, W3, b3 of one MLP."""
    return [0.2 * torch.randn(HS, ldw1, device="cuda"), 0.1 * torch.randn(HS, device="cuda"), 0.2 * torch.randn(HS, HS, device="cuda"),
            0.1 * torch.randn(HS, device="cuda"), 0.2 * torch.randn(HS, HS, device="cuda"), 0.1 * torch.randn(HS, device="cuda")]


class _Case:
    """The 22 leading arguments of the four entry points for one shape and mask form."""

    def __init__(self, torch, B, N, mask_form):
        self.B, self.N, self.S = B, N, (N + HS - 1) // HS
        n_real = min(N_REAL, N)
        self.mask, self.is_count, self.inv_n_host = None, 0, 1.0 / N
        if mask_form == "mask":
            self.mask, self.inv_n_host = (torch.arange(N, device="cuda") < n_real).float().contiguous(), 1.0 / n_real
        elif mask_form == "count":
            self.mask, self.is_count, self.inv_n_host = torch.tensor([float(n_real)], device="cuda"), 1, 0.0
        self.ctx_part = torch.randn(B, 2, HS, device="cuda")            # S_ctx = 2

    def common(self, x, d_in, P, ctx):
        """x [B * N, d_in] through the MLP P = (W1, b1, W2, b2, W3, b3), with (ctx) or without the set's pooled context."""
        W1, b1, W2, b2, W3, b3 = P
        assert W1.shape[1] == d_in + (HS if ctx else 0)
        return [_p(x), d_in, self.B, self.N, self.S, HS, _p(self.mask), self.is_count, None, self.inv_n_host,
                _p(self.ctx_part) if ctx else None, 2 if ctx else 0, _p(W1), W1.shape[1], _p(b1), _p(W2), _p(b2), _p(W3), _p(b3), HS, None, 0]

    def rows(self, torch, *tail):
        return torch.full((self.B * self.N,) + tail, SENTINEL, device="cuda")

    def parts(self, torch, *tail):
        return torch.full((self.B * self.S,) + tail, SENTINEL, device="cuda")


def _same(torch, names, pair, two):
    torch.cuda.synchronize()
    for name, a, b in zip(names, pair, two):
        assert bool(torch.isfinite(a).all()), name
        assert torch.equal(a, b), (name, int((a != b).sum()), float((a - b).abs().max()))


@pytest.mark.parametrize("shape,d_in,mask_form", list(itertools.product(SHAPES, D_INS, MASKS)))
def test_paired_forward_equals_two_single_forwards(shape, d_in, mask_form):
    """nddm_deepset_mlp2_fwd(A, B) against nddm_deepset_mlp_fwd(A: y wanted, no pooling) then nddm_deepset_mlp_fwd(B on that y: d_in
    64, no context, only the pooled sums wanted): h1, h2, y, h1b, h2b, pool_part_b."""
    import torch
    L = _lib()
    torch.manual_seed(41)
    B, N = shape
    K = _Case(torch, B, N, mask_form)
    x = torch.randn(B * N, d_in, device="cuda")
    PA, PB = _mlp(torch, d_in + HS), _mlp(torch, HS)
    pair = [K.rows(torch, HS) for _ in range(5)] + [K.parts(torch, HS)]
    two = [K.rows(torch, HS) for _ in range(5)] + [K.parts(torch, HS)]
    h1, h2, y, h1b, h2b, pool = pair
    assert L.nddm_deepset_mlp2_fwd(*K.common(x, d_in, PA, True), _p(h1), _p(h2), _p(y), *[_p(w) for w in PB], _p(h1b), _p(h2b), _p(pool), None) == 0
    h1, h2, y, h1b, h2b, pool = two
    assert L.nddm_deepset_mlp_fwd(*K.common(x, d_in, PA, True), _p(h1), _p(h2), _p(y), None, 0, None, 0, 0, None) == 0
    assert L.nddm_deepset_mlp_fwd(*K.common(y, HS, PB, False), _p(h1b), _p(h2b), None, _p(pool), 0, None, 0, 0, None) == 0
    _same(torch, ("h1", "h2", "y", "h1b", "h2b", "pool_part_b"), pair, two)
    assert not bool((pair[2] == SENTINEL).any()) and not bool((pair[5] == SENTINEL).any())      # (every row and sum was written)


@pytest.mark.parametrize("shape,d_in,mask_form,gp_form,with_prev",
                         list(itertools.product(SHAPES, D_INS, MASKS, ("context", "mean"), (True, False))))
def test_paired_backward_equals_two_single_backwards(shape, d_in, mask_form, gp_form, with_prev):
    """nddm_deepset_mlp2_bwd(Y, X) against nddm_deepset_mlp_bwd(X), which ADDS its input gradient to a buffer that holds a copy of
    gx_prev (zeros where there is none: both sides compute buffer + gradient), then nddm_deepset_mlp_bwd(Y) with that buffer as its
    output gradient and no pooled gradient: Y's gx (64-wide input only), dctx_part and both MLPs' weight-gradient rows, each
    allocated at its full ld_part.  The pooled gradient of X in both forms of BwdIO."""
    import torch
    L = _lib()
    torch.manual_seed(43)
    B, N = shape
    K = _Case(torch, B, N, mask_form)
    x, x1 = torch.randn(B * N, d_in, device="cuda"), torch.randn(B * N, HS, device="cuda")
    PY, PX = _mlp(torch, d_in + HS), _mlp(torch, HS)
    h1y, h2y, h1x, h2x = (torch.relu(torch.randn(B * N, HS, device="cuda")) for _ in range(4))      # saved activations: zeros and positives
    if gp_form == "context":            # the consumer's per-workgroup sums, through its context columns [64, 64] of a W1 [64, 128]
        gpool, gp_S, Wc, gp_ldw = torch.randn(B, 2, HS, device="cuda"), 2, 0.2 * torch.randn(HS, 2 * HS, device="cuda"), 2 * HS
        gp_W = Wc.data_ptr() + 4 * HS
    else:                               # the gradient of the masked mean
        gpool, gp_S, gp_W, gp_ldw = torch.randn(B, HS, device="cuda"), 0, None, 0
    gx_prev = torch.randn(B * N, HS, device="cuda") if with_prev else None
    ld_part = HS * (d_in + HS) + HS + 2 * (HS * HS + HS)                # Y's row, the longer one
    big = d_in == HS

    def outputs():
        return [K.rows(torch, HS), K.parts(torch, HS), K.parts(torch, ld_part), K.parts(torch, ld_part)]

    pair, two = outputs(), outputs()
    gx, dctx, wy, wx = pair
    assert L.nddm_deepset_mlp2_bwd(*K.common(x, d_in, PY, True), _p(h1y), _p(h2y), _p(gx) if big else None, _p(dctx), _p(wy), _p(x1),
                                   *[_p(w) for w in PX], _p(h1x), _p(h2x), _p(gpool), gp_S, gp_W, gp_ldw, _p(gx_prev), _p(wx), ld_part, None) == 0
    gx, dctx, wy, wx = two
    gy = gx_prev.clone() if with_prev else torch.zeros(B * N, HS, device="cuda")
    assert L.nddm_deepset_mlp_bwd(*K.common(x1, HS, PX, False), _p(h1x), _p(h2x), None, 0, _p(gpool), gp_S, gp_W, gp_ldw, _p(gy), 1, None,
                                  _p(wx), ld_part, None) == 0
    assert L.nddm_deepset_mlp_bwd(*K.common(x, d_in, PY, True), _p(h1y), _p(h2y), _p(gy), HS, None, 0, None, 0, _p(gx) if big else None, 0,
                                  _p(dctx), _p(wy), ld_part, None) == 0
    _same(torch, ("gx", "dctx_part", "wpart_y", "wpart_x"), pair, two)
    assert bool((pair[0] == SENTINEL).all()) != big and not bool((pair[1] == SENTINEL).any())      # (gx: written, or not touched)
    assert bool((pair[3][:, 3 * (HS * HS + HS):] == SENTINEL).all())                               # (X's row ends where its gradients end)
