"""Minimal PyTorch-ROCm stand-in for the BayesFlow objects the reference builds at basic_ddm_dc.py:163-176 and drives
at :199-207, :223 (SURVEY f-4 / BASELINE config 5): a DeepSet summary network, a conditional affine-coupling flow, an
amortized posterior, and a trainer with online and experience-replay loops that consume `generative_model(B)` ->
`configurator(dict)` exactly as BayesFlow's Trainer does.

    summary_net = InvariantNetwork()
    inference_net = InvertibleNetwork(num_params=num_params)
    amortizer = AmortizedPosterior(inference_net, summary_net)
    trainer = Trainer(amortizer=amortizer, generative_model=generative_model, configurator=configurator,
                      checkpoint_path=f"checkpoint/{model_name}")
    losses = trainer.train_experience_replay(epochs=…, batch_size=32, iterations_per_epoch=1000)
    post = amortizer.sample(configurator(generative_model(1)), n_samples=10000)

BayesFlow/TensorFlow are not installable here, so parity with BayesFlow's networks is UNPINNED; what is pinned is
the dictionary contract on both sides ('summary_conditions', 'direct_conditions', 'parameters').  The networks are plain
PyTorch modules; on the GPU the flow and the summary network's per-trial MLPs run as hand-written kernels
(csrc/train_kernels.hip, csrc/train_deepset.hip -- at batch 32 the PyTorch composition is ~600 launches of a few
microseconds per training iteration), with the PyTorch composition as the definition they are tested against.
"""
import math
import os
import pickle

import numpy as np
import torch
from torch import nn


class _PerSetLinearFn(torch.autograd.Function):
    """y = x W^T + b for x [B, N, in] with the weight gradient computed per set and then summed: as ONE GEMM it is a
    [in, B*N] x [B*N, out] product with a 64 x 64 result -- two workgroups on a 256-CU chip, 50 us at B*N = 9600 -- as a
    batched GEMM over the B sets it is 6 us (+ a 32-row sum).  14 such products are a fifth of a graph-replayed iteration."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return torch.addmm(b, x.reshape(-1, x.shape[-1]), w.t()).view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g = g.contiguous()
        gx = (g.reshape(-1, g.shape[-1]) @ w).view_as(x) if ctx.needs_input_grad[0] else None
        gw = torch.bmm(g.transpose(1, 2), x).sum(0)
        return gx, gw, g.sum((0, 1))


class _Linear(nn.Linear):
    def forward(self, x):
        if x.dim() == 3 and x.is_cuda and torch.is_grad_enabled():
            return _PerSetLinearFn.apply(x, self.weight, self.bias)
        return super().forward(x)


def _mlp(d_in, d_hidden, d_out, n_hidden=2, act=nn.ReLU, keras_init=True):
    layers, d = [], d_in
    for _ in range(n_hidden):
        layers += [_Linear(d, d_hidden), act()]
        d = d_hidden
    layers.append(_Linear(d, d_out))
    # Keras-style initialisation (the reference's networks are BayesFlow/Keras Dense layers: Glorot weights, zero biases),
    # with He scaling on the hidden layers: PyTorch's Linear default shrinks the signal by ~0.58 per layer, and through the ~15
    # stacked layers of the summary network the data-dependent part of its output was 1e-5 of the bias-driven part at
    # initialisation -- the amortizer then learns the prior long before it starts looking at the data
    # (the coupling layers' internal networks keep PyTorch's small default: a flow should start near the identity)
    if keras_init:
        for m in layers[:-1]:
            if isinstance(m, nn.Linear):
                nn.init.kaiming_uniform_(m.weight, nonlinearity="relu")
                nn.init.zeros_(m.bias)
        nn.init.xavier_uniform_(layers[-1].weight)
        nn.init.zeros_(layers[-1].bias)
    return nn.Sequential(*layers)


class _Equivariant(nn.Module):
    """x[b,n,:] -> f(x[b,n,:], mean_n g(x[b,n,:])): permutation-equivariant DeepSet block."""

    def __init__(self, d_in, d_hidden):
        super().__init__()
        self.inv = _mlp(d_in, d_hidden, d_hidden)
        self.eq = _mlp(d_in + d_hidden, d_hidden, d_hidden)

    def forward(self, x, mask=None, inv_n=None):
        g = self.inv(x)
        pooled = g.mean(dim=1, keepdim=True) if mask is None else (g * mask).sum(dim=1, keepdim=True) * inv_n
        return self.eq(torch.cat([x, pooled.expand(-1, x.shape[1], -1)], dim=-1))


class InvariantNetwork(nn.Module):
    """bf.networks.InvariantNetwork(): exchangeable trials [B, N, D] -> learned summary [B, summary_dim]."""

    def __init__(self, input_dim=2, summary_dim=10, hidden=64, num_equiv=2):
        super().__init__()
        blocks, d = [], input_dim
        for _ in range(num_equiv):
            blocks.append(_Equivariant(d, hidden))
            d = hidden
        self.equiv = nn.Sequential(*blocks)
        self.pre_pool = _mlp(d, hidden, hidden)
        self.post_pool = _mlp(hidden, hidden, summary_dim)
        self.summary_dim = summary_dim
        self.fused = True           # the hand-written kernels where they apply (False: always the PyTorch composition)

    def _fused_lib(self, x):
        """libnddm_train.so if its per-trial MLP kernels cover this network and this tensor, else None (the PyTorch composition)."""
        if not (self.fused and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.shape[1] >= 1):
            return None
        # the kernels are the TRAINING path: their forward always stores every hidden activation for the backward (2.5 KB per
        # trial row) and the backward one partial weight-gradient block per 64 rows.  Inference (no_grad: validation_loss,
        # sample) and batches beyond FUSED_MAX_ROWS trial rows take the PyTorch composition, which keeps nothing; and the
        # kernels produce no gradient of the data.
        if not torch.is_grad_enabled() or x.shape[0] * x.shape[1] > self.FUSED_MAX_ROWS or x.requires_grad:
            return None
        return self._deepset_lib(x.shape[2])

    def _deepset_lib(self, d_in):
        """libnddm_train.so if the network has the shape its DeepSet kernels are written for (3-layer ReLU MLPs of hidden width 64)."""
        mlps = [m for blk in self.equiv for m in (blk.inv, blk.eq)] + [self.pre_pool, self.post_pool]
        if any(len(m) != 5 or not isinstance(m[1], nn.ReLU) or m[2].weight.shape != (64, 64) or m[4].weight.shape[1] != 64
               for m in mlps) or any(m[4].weight.shape[0] != 64 for m in mlps[:-1]) or not 1 <= self.summary_dim <= 64:
            return None
        from . import _train_lib
        L = _train_lib.lib()
        return L if L is not None and L.nddm_deepset_supported(64, d_in) else None

    def _summary_lib(self, x, direct):
        """`summarize`'s gate, its own (`_fused_lib` is the training path's and refuses no_grad): the library if the inference
        kernels (csrc/train_deepset.hip: nddm_deepset_summary) serve this tensor -- cuda, float32, [B, N, d_in <= 4] -- this network
        (hidden width 64, float32 parameters on x's device) and these direct conditions ([B, k] with summary_dim + k <= 64)."""
        if not (self.fused and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.shape[0] >= 1 and x.shape[1] >= 1 and x.shape[2] <= 4):
            return None
        if direct is not None and (direct.dim() != 2 or direct.shape[0] != x.shape[0] or self.summary_dim + direct.shape[1] > 64):
            return None
        if any(p.dtype != torch.float32 or p.device != x.device or not p.is_contiguous() for p in self.parameters()):
            return None
        return self._deepset_lib(x.shape[2])

    def fused_params(self):
        """The parameter tensors in the order the kernels (and their flat weight-gradient buffer) take them: per block the
        invariant then the equivariant MLP, then the pre-pooling and the post-pooling MLP; W1, b1, W2, b2, W3, b3 of each."""
        ps = [t for blk in self.equiv for mlp in (blk.inv, blk.eq) for k in (0, 2, 4) for t in (mlp[k].weight, mlp[k].bias)]
        return ps + [t for mlp in (self.pre_pool, self.post_pool) for k in (0, 2, 4) for t in (mlp[k].weight, mlp[k].bias)]

    # a GraphTrainer may point this at the slice of ITS flat gradient buffer that holds fused_params() back to back: the backward's
    # last kernel then writes the gradients where the optimizer reads them (no gather copy); None: a buffer of the call's own
    grad_sink = None

    FUSED_MAX_ROWS = 1 << 19      # sets x trials (the training loop's 32 x 300 is 9600): 1.3 GB of saved activations at the cap

    @staticmethod
    def _set_counts(counts, B, N, device):
        """counts -> int32 [B] on `device`.  Host-side counts (a sequence, an array, a CPU tensor) are checked against [1, N]; a
        tensor already on an accelerator is not read back: its rows are the caller's responsibility."""
        if torch.is_tensor(counts) and counts.device.type != "cpu":
            c = counts.reshape(-1)
        else:
            c = torch.as_tensor(np.asarray(counts.detach().numpy() if torch.is_tensor(counts) else counts)).reshape(-1)
            if c.numel() and (c.is_floating_point() and bool((c != c.round()).any()) or int(c.min()) < 1 or int(c.max()) > N):
                raise ValueError(f"counts must be whole numbers in [1, {N}] (the sets are padded to {N} trials)")
        if c.numel() != B:
            raise ValueError(f"counts has {c.numel()} entries for {B} data sets")
        return c.to(device=device, dtype=torch.int32)

    def _forward_counts(self, x, counts, direct):
        """The definition of a ragged batch (`forward(x, counts=...)`): the mask / inv_n arithmetic with a mask [B, N, 1] and a
        1 / n per set; the padding is zeroed first, so whatever it holds (NaN too) never enters a product."""
        B, N = x.shape[0], x.shape[1]
        c = self._set_counts(counts, B, N, x.device)
        real = torch.arange(N, device=x.device).view(1, N, 1) < c.view(B, 1, 1)
        mask, inv_n = real.to(x.dtype), 1.0 / c.to(x.dtype)
        x = torch.where(real, x, torch.zeros((), dtype=x.dtype, device=x.device))
        for block in self.equiv:
            x = block(x, mask, inv_n.view(B, 1, 1))
        summ = self.post_pool((self.pre_pool(x) * mask).sum(dim=1) * inv_n.view(B, 1))
        return summ if direct is None else torch.cat([summ, direct.to(summ.device, summ.dtype)], dim=-1)

    @torch.no_grad()
    def summarize(self, x, counts=None, direct=None):
        """The inference forward: x [B, N, d] -> [B, summary_dim (+ k)], where set b's summary is over its first counts[b] trials
        (counts: B whole numbers in [1, N], a sequence or a tensor; None: all N of every set) and direct [B, k] is appended as
        `forward` appends it.  On the device -- float32, hidden width 64, d <= 4, summary_dim + k <= 64, `self.fused` -- the whole
        network is blocks + 2 launches that keep nothing for a backward and never read a row at or beyond its set's count (csrc/
        train_deepset.hip: nddm_deepset_summary); row b is bit for bit what the call gives for x[b:b+1, :counts[b]] alone, and with
        equal counts what the training kernels' forward gives.  Everywhere else: `forward(x, counts=counts, direct=direct)`."""
        if direct is not None:
            direct = torch.as_tensor(direct).to(x.device, x.dtype)
        L = self._summary_lib(x, direct)
        if L is None:
            return self.forward(x, direct=direct) if counts is None else self.forward(x, counts=counts, direct=direct)
        import ctypes
        B, N, d = x.shape
        x = x.contiguous()
        cnt = None if counts is None else self._set_counts(counts, B, N, x.device).contiguous()
        params, nb = self.fused_params(), len(self.equiv)
        ptrs = (ctypes.c_void_p * len(params))(*[p.data_ptr() for p in params])
        k = 0 if direct is None else direct.shape[1]
        if direct is not None and k > 1 and direct.stride(1) != 1:
            direct = direct.contiguous()
        nbytes = L.nddm_deepset_summary_work_bytes(B, N, nb)
        work = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=x.device)
        out = torch.empty((B, self.summary_dim + k), dtype=torch.float32, device=x.device)
        rc = L.nddm_deepset_summary(x.data_ptr(), d, B, N, None if cnt is None else cnt.data_ptr(), nb, ptrs, self.summary_dim,
                                    None if direct is None else direct.data_ptr(), k, 0 if direct is None else direct.stride(0),
                                    out.data_ptr(), work.data_ptr(), nbytes, torch.cuda.current_stream(x.device).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"nddm_deepset_summary failed ({rc})")
        return out

    def forward(self, x, mask=None, inv_n=None, n_valid=None, direct=None, counts=None):
        """direct [B, k] (or broadcastable rows): "direct conditions" (log N, basic_ddm_dc.py:151-155) appended to the summary --
        the result is then the flow's condition [B, summary_dim + k] (the kernels write both into one buffer: no concatenation,
        and the backward takes the condition's gradient as it comes).
        mask [1, N, 1] (1 = a real trial, 0 = padding) and inv_n = 1 / (number of real trials), both device tensors -- or
        n_valid, the number of real trials as a device scalar (the first n_valid trials are the real ones): the pooled means
        then run over the real trials only, so a batch padded to a fixed length (one hipGraph per length bucket,
        GraphTrainer) gives what the unpadded batch gives.
        counts (B whole numbers in [1, N]; not with mask / inv_n / n_valid): a RAGGED batch -- the first counts[b] trials of set b
        are real and row b of the result is what the network gives for x[b:b+1, :counts[b]] alone, to float32 round-off.  This
        is the PyTorch composition on every device (differentiable in the parameters); `summarize` is its inference kernel."""
        if counts is not None:
            if mask is not None or inv_n is not None or n_valid is not None:
                raise ValueError("counts (a trial count per set) cannot be combined with mask / inv_n / n_valid (batch-shared)")
            return self._forward_counts(x, counts, direct)
        L = self._fused_lib(x)
        if direct is not None and (L is None or direct.dim() != 2 or direct.shape[0] != x.shape[0] or direct.dtype != torch.float32
                                   or self.summary_dim + direct.shape[1] > 64 or direct.requires_grad):
            return torch.cat([self.forward(x, mask, inv_n, n_valid), direct.to(x.device, torch.float32)], dim=-1)
        if n_valid is not None and mask is None:
            n_valid = n_valid.reshape(-1).to(torch.float32)
            if L is not None:
                return _FusedDeepSetFn.apply((L, self.grad_sink), len(self.equiv), x, n_valid, None, direct, *self.fused_params())
            mask = (torch.arange(x.shape[1], device=x.device, dtype=torch.float32) < n_valid).to(torch.float32).view(1, -1, 1)
            inv_n = 1.0 / n_valid
        if L is not None:
            params = self.fused_params()
            m = None if mask is None else mask.reshape(-1).to(torch.float32)
            inv = None if inv_n is None else (inv_n if torch.is_tensor(inv_n) else torch.full((1,), float(inv_n), device=x.device))
            if inv is not None:
                inv = inv.reshape(-1).to(torch.float32)
            return _FusedDeepSetFn.apply((L, self.grad_sink), len(self.equiv), x, m, inv, direct, *params)
        for block in self.equiv:
            x = block(x, mask, inv_n)
        h = self.pre_pool(x)
        pooled = h.mean(dim=1) if mask is None else (h * mask).sum(dim=1) * inv_n
        return self.post_pool(pooled)


class _FusedDeepSetFn(torch.autograd.Function):
    """The summary network -- every equivariant block (an MLP whose masked per-set mean is the context of a second MLP), the
    pre-pooling MLP with its masked mean, and the MLP after the pooling -- as hand-written kernels (csrc/train_deepset.hip): one
    launch per 3-layer MLP each way plus one reduction of the weight gradients, instead of ~170 PyTorch launches of 4-7
    microseconds over [sets x trials, 64].  x [B, N, d] -> summary [B, summary_dim].  params: W1, b1, W2, b2, W3, b3 of the
    blocks' (invariant, equivariant) MLPs in order, then of the pre-pooling MLP, then of the post-pooling MLP.
    mask [N] and inv_n (device scalar), or mask = ONE float, the number of real trials, and inv_n None; or both None."""

    ROWS_PER_WG = 64     # one 64-row tile per workgroup: 160 workgroups at 32 sets x 300 trials (the chip has 256 CUs)

    @staticmethod
    def _common(x_t, d, B, N, S, rpw, mask, inv_n, ctx_part, S_ctx, prm, x_part=None, S_x=0):
        count = mask is not None and mask.numel() == 1 and inv_n is None       # the number of real trials instead of a 0/1 mask
        return (None if x_t is None else x_t.data_ptr(), d, B, N, S, rpw, None if mask is None else mask.data_ptr(), int(count),
                None if inv_n is None else inv_n.data_ptr(), 1.0 / N, None if ctx_part is None else ctx_part.data_ptr(), S_ctx,
                prm[0].data_ptr(), prm[0].shape[1], prm[1].data_ptr(), prm[2].data_ptr(), prm[3].data_ptr(), prm[4].data_ptr(),
                prm[5].data_ptr(), prm[4].shape[0], None if x_part is None else x_part.data_ptr(), S_x)

    @staticmethod
    def forward(ctx, L_sink, nb, x, mask, inv_n, direct, *params):
        L, ctx.sink = L_sink
        (B, N, d0), dev, rpw = x.shape, x.device, _FusedDeepSetFn.ROWS_PER_WG
        T, S, Hd = B * N, -(-N // rpw), 64
        Sp = -(-B // rpw)                           # the post-pooling MLP runs on one row per set: B rows in all
        x = x.contiguous()
        acts = torch.empty(((2 * nb + 1) * 2 * T + 2 * B, Hd), dtype=torch.float32, device=dev)   # h1, h2 of every MLP
        act = lambda k, j: acts[(2 * k + j) * T:(2 * k + j + 1) * T]
        act_post = lambda j: acts[(2 * nb + 1) * 2 * T + j * B:(2 * nb + 1) * 2 * T + (j + 1) * B]
        xs_next = torch.empty((max(nb, 1), T, Hd), dtype=torch.float32, device=dev)
        pools = torch.empty((nb + 1, B, S, Hd), dtype=torch.float32, device=dev)
        post = params[12 * nb + 6:]
        d_sum = post[4].shape[0]
        n_extra = 0 if direct is None else direct.shape[1]
        if direct is not None and n_extra > 1 and direct.stride(1) != 1:
            direct = direct.contiguous()
        summary = torch.empty((B, d_sum + n_extra), dtype=torch.float32, device=dev)      # (+ the direct conditions' columns)
        st = torch.cuda.current_stream(dev).cuda_stream
        cm = _FusedDeepSetFn._common
        count = mask is not None and mask.numel() == 1 and inv_n is None
        # every MLP that pools (the blocks' invariant halves, the pre-pooling MLP) consumes the rows the equivariant MLP before
        # it produces: the two run as ONE launch (the first invariant MLP, on the raw trials, alone)
        cur, d, rc = x, d0, 0
        pooling = [params[12 * i:12 * i + 6] for i in range(nb)] + [params[12 * nb:12 * nb + 6]]     # inv_0 .. inv_{nb-1}, pre
        rc |= L.nddm_deepset_mlp_fwd(*cm(cur, d, B, N, S, rpw, mask, inv_n, None, 0, pooling[0]), act(0, 0).data_ptr(),
                                     act(0, 1).data_ptr(), None, pools[0].data_ptr(), 0, None, 0, 0, st)
        for i in range(nb):
            eq, nxt = params[12 * i + 6:12 * i + 12], pooling[i + 1]
            rc |= L.nddm_deepset_mlp2_fwd(*cm(cur, d, B, N, S, rpw, mask, inv_n, pools[i], S, eq), act(2 * i + 1, 0).data_ptr(),
                                          act(2 * i + 1, 1).data_ptr(), xs_next[i].data_ptr(), *[t.data_ptr() for t in nxt],
                                          act(2 * i + 2, 0).data_ptr(), act(2 * i + 2, 1).data_ptr(), pools[i + 1].data_ptr(), st)
            cur, d = xs_next[i], Hd
        # (1 / N as the host's value must be THIS launch's N, not the B rows the post-pooling MLP is launched over)
        cp = list(cm(None, Hd, 1, B, Sp, rpw, mask if count else None, inv_n, None, 0, post, pools[nb], S))
        cp[9] = 1.0 / N
        rc |= L.nddm_deepset_mlp_fwd(*cp, act_post(0).data_ptr(), act_post(1).data_ptr(), summary.data_ptr(), None, d_sum + n_extra,
                                     None if direct is None else direct.data_ptr(), n_extra, 0 if direct is None else direct.stride(0), st)
        if rc != 0:
            raise RuntimeError(f"nddm_deepset_mlp_fwd failed ({rc})")
        ctx.L, ctx.nb, ctx.has_mask, ctx.has_inv, ctx.ld_out = L, nb, mask is not None, inv_n is not None, d_sum + n_extra
        ctx.save_for_backward(x, acts, xs_next, pools, *([mask] if mask is not None else []), *([inv_n] if inv_n is not None else []),
                              *params)
        return summary

    @staticmethod
    def backward(ctx, g_summary):
        L, nb, rpw = ctx.L, ctx.nb, _FusedDeepSetFn.ROWS_PER_WG
        x, acts, xs_next, pools, *rest = ctx.saved_tensors
        mask = rest.pop(0) if ctx.has_mask else None
        inv_n = rest.pop(0) if ctx.has_inv else None
        params = rest
        (B, N, d0), dev, Hd = x.shape, x.device, 64
        T, S, Sp = B * N, pools.shape[2], -(-B // rpw)
        G = B * S
        act = lambda k, j: acts[(2 * k + j) * T:(2 * k + j + 1) * T]
        act_post = lambda j: acts[(2 * nb + 1) * 2 * T + j * B:(2 * nb + 1) * 2 * T + (j + 1) * B]
        sizes = [p.numel() for p in params]
        per_mlp = [sum(sizes[6 * k:6 * k + 6]) for k in range(2 * nb + 2)]
        offs = [sum(per_mlp[:k]) for k in range(2 * nb + 2)]
        P = sum(per_mlp)
        part = torch.empty((G, P), dtype=torch.float32, device=dev)
        sink = ctx.sink
        flat = sink if (sink is not None and sink.numel() == P and sink.device == dev) else torch.empty(P, dtype=torch.float32, device=dev)
        gxbuf = torch.empty((max(nb, 1), T, Hd), dtype=torch.float32, device=dev)
        dctx = torch.empty((max(nb, 1), B, S, Hd), dtype=torch.float32, device=dev)
        g_pooled = torch.empty((B, Hd), dtype=torch.float32, device=dev)
        g_summary = g_summary.contiguous()
        st, F = torch.cuda.current_stream(dev).cuda_stream, 4
        cm = _FusedDeepSetFn._common
        count = mask is not None and mask.numel() == 1 and inv_n is None
        pp = part.data_ptr()

        def x_of(i):                                # input of block i (and of the pre-pooling MLP for i == nb)
            return (xs_next[i - 1], Hd) if i else (x, d0)

        post = params[12 * nb + 6:]
        cp = list(cm(None, Hd, 1, B, Sp, rpw, mask if count else None, inv_n, None, 0, post, pools[nb], S))
        cp[9] = 1.0 / N
        rc = L.nddm_deepset_mlp_bwd(*cp, act_post(0).data_ptr(), act_post(1).data_ptr(), g_summary.data_ptr(), ctx.ld_out, None, 0, None, 0,
                                    g_pooled.data_ptr(), 0, None, pp + offs[2 * nb + 1] * F, P, st)
        pre = params[12 * nb:12 * nb + 6]
        if nb == 0:
            rc |= L.nddm_deepset_mlp_bwd(*cm(x, d0, B, N, S, rpw, mask, inv_n, None, 0, pre), act(0, 0).data_ptr(), act(0, 1).data_ptr(),
                                         None, 0, g_pooled.data_ptr(), 0, None, 0, None, 0, None, pp + offs[0] * F, P, st)
        # The backward of a pooling MLP X (pre-pooling, or a block's invariant half) and of the equivariant MLP Y that produced X's
        # input are ONE launch each (csrc/train_deepset.hip: mlp2_bwd_kernel): pre + eq_{nb-1}, then inv_i + eq_{i-1}, then inv_0
        # alone.  X's input gradient -- plus eq_i's, which the launch before left in gxbuf -- is Y's output gradient.
        for j in reversed(range(nb)):                       # Y = eq_j;  X = pre (j == nb - 1) or inv_{j+1}
            eq = params[12 * j + 6:12 * j + 12]
            xin, d = x_of(j)
            if j == nb - 1:
                X, hx, ox = pre, 2 * nb, offs[2 * nb]
                gpool, gp_S, gp_W, gp_ldw, gx_prev = g_pooled.data_ptr(), 0, None, 0, None
            else:
                X, hx, ox = params[12 * (j + 1):12 * (j + 1) + 6], 2 * (j + 1), offs[2 * (j + 1)]
                eq_next = params[12 * (j + 1) + 6:12 * (j + 1) + 12]          # (its context columns carry the pooled gradient)
                gpool, gp_S, gp_W, gp_ldw, gx_prev = dctx[j + 1].data_ptr(), S, eq_next[0].data_ptr() + Hd * F, 2 * Hd, gxbuf[j].data_ptr()
            rc |= L.nddm_deepset_mlp2_bwd(*cm(xin, d, B, N, S, rpw, mask, inv_n, pools[j], S, eq), act(2 * j + 1, 0).data_ptr(),
                                          act(2 * j + 1, 1).data_ptr(), gxbuf[j - 1].data_ptr() if j else None, dctx[j].data_ptr(),
                                          pp + offs[2 * j + 1] * F, xs_next[j].data_ptr(), *[t.data_ptr() for t in X],
                                          act(hx, 0).data_ptr(), act(hx, 1).data_ptr(), gpool, gp_S, gp_W, gp_ldw, gx_prev, pp + ox * F, P, st)
        if nb:
            inv, eq = params[0:6], params[6:12]
            rc |= L.nddm_deepset_mlp_bwd(*cm(x, d0, B, N, S, rpw, mask, inv_n, None, 0, inv), act(0, 0).data_ptr(), act(0, 1).data_ptr(),
                                         None, 0, dctx[0].data_ptr(), S, eq[0].data_ptr() + d0 * F, d0 + Hd, None, 0, None, pp + offs[0] * F, P, st)
        rc |= L.nddm_deepset_reduce(pp, G, P, offs[2 * nb + 1], Sp, flat.data_ptr(), st)
        if rc != 0:
            raise RuntimeError(f"nddm_deepset_mlp_bwd failed ({rc})")
        grads, o = [], 0
        for p, n in zip(params, sizes):
            grads.append(flat[o:o + n].view(p.shape))
            o += n
        return (None, None, None, None, None, None, *grads)


class _FusedFlowFn(torch.autograd.Function):
    """The whole conditional flow -- per layer an ActNorm, a fixed permutation and two conditional affine-coupling half-layers
    (concatenate, three Linear layers with two ELUs, soft clamp, exp, multiply-add) -- as ONE hand-written kernel forward and ONE
    backward (csrc/train_kernels.hip) and one autograd node: at batch 32 the PyTorch composition is ~400 launches of a few
    microseconds each way, with a slice / concatenate / select bookkeeping kernel between any two.  (The backward is two
    kernels: the chain of activation gradients, and the weight gradients of all half-layers side by side.)
    -> (z [R, D], log|det| [R]); with nll=True -> the maximum-likelihood loss mean(|z|^2 / 2 - log|det|) itself (the backward
    then derives the gradients of z and log|det| inside the kernel: ~12 more PyTorch launches gone).
    params: per layer ActNorm log-scale and bias, then weight, bias x 3 of both sub-networks."""

    @staticmethod
    def forward(ctx, L_sink, clamp, d1, perms, nll, theta, cond, *params):
        import ctypes
        L, ctx.sink = L_sink
        nl, (R, D), C = len(perms), theta.shape, cond.shape[1]
        Hd, dev = params[4].shape[0], theta.device
        theta, cond = theta.contiguous(), cond.contiguous()
        saved = torch.empty(3 * nl * R * D + 4 * nl * R * Hd, dtype=torch.float32, device=dev)
        z_all, out_all, s_all = (saved[i * nl * R * D:(i + 1) * nl * R * D].view(nl, R, D) for i in range(3))
        h_all = saved[3 * nl * R * D:]
        ld = torch.empty(R + 1, dtype=torch.float32, device=dev)           # (+ the loss)
        loss = ld[R:]
        if nll and ctx.sink is not None and ctx.sink.get("loss") is not None and ctx.sink["loss"].device == dev:
            loss = ctx.sink["loss"]                                        # the trainer's slot: no copy of the loss afterwards
        ptrs = (ctypes.c_void_p * (14 * nl))(*[p.data_ptr() for p in params])
        perm = (ctypes.c_int * (nl * D))(*[int(v) for p in perms for v in p])
        rc = L.nddm_train_flow_fwd(nl, R, D, d1, C, float(clamp), ptrs, perm, theta.data_ptr(), cond.data_ptr(), z_all.data_ptr(),
                                   out_all.data_ptr(), s_all.data_ptr(), h_all.data_ptr(), ld.data_ptr(),
                                   loss.data_ptr() if nll else None, torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"nddm_train_flow_fwd failed ({rc})")
        ctx.L, ctx.clamp, ctx.d1, ctx.perm, ctx.ptrs, ctx.nl, ctx.nll = L, float(clamp), d1, perm, ptrs, nl, bool(nll)
        ctx.save_for_backward(theta, cond, saved, *params)
        return loss.view(()) if nll else (out_all[nl - 1], ld[:R])

    @staticmethod
    def backward(ctx, *gs):
        import ctypes
        theta, cond, saved, *params = ctx.saved_tensors
        L, nl, d1 = ctx.L, ctx.nl, ctx.d1
        (R, D), C, dev = theta.shape, cond.shape[1], theta.device
        n_rd = nl * R * D
        sizes = [p.numel() for p in params]
        Hd = params[4].shape[0]
        n_scratch = [nl * R * D, R * D, R * C, R, 2 * nl * R * (2 * Hd + 16)]
        slots = None if ctx.sink is None else [ctx.sink["grads"].get(p.data_ptr()) for p in params]
        in_place = slots is not None and all(s_ is not None and s_.shape == p.shape and s_.device == dev for s_, p in zip(slots, params))
        flat = torch.empty((0 if in_place else sum(sizes)) + sum(n_scratch), dtype=torch.float32, device=dev)
        grads, o = [], 0
        for k, (p, n) in enumerate(zip(params, sizes)):      # the trainer's slots (its flat gradient buffer), or a buffer of this call's own
            if in_place:
                grads.append(slots[k])
            else:
                grads.append(flat[o:o + n].view(p.shape))
                o += n
        scratch = []
        for n in n_scratch:
            scratch.append(flat[o:o + n])
            o += n
        gz_all, gx, gcond, w_gld, work = scratch
        if ctx.nll:
            g_nll, g_z, g_ld = gs[0].contiguous(), None, w_gld
        else:
            g_nll = None
            g_z = gs[0].contiguous() if gs[0] is not None else torch.zeros_like(theta)
            g_ld = gs[1].contiguous() if gs[1] is not None else torch.zeros(R, dtype=torch.float32, device=dev)
        gptr = (ctypes.c_void_p * (14 * nl))(*[g.data_ptr() for g in grads])
        sp, F = saved.data_ptr(), 4
        rc = L.nddm_train_flow_bwd(nl, R, D, d1, C, ctx.clamp, ctx.ptrs, ctx.perm, gptr, theta.data_ptr(), cond.data_ptr(),
                                   sp, sp + n_rd * F, sp + 2 * n_rd * F, sp + 3 * n_rd * F, None if g_z is None else g_z.data_ptr(),
                                   g_ld.data_ptr(), None if g_nll is None else g_nll.data_ptr(), gz_all.data_ptr(), gx.data_ptr(),
                                   gcond.data_ptr(), work.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"nddm_train_flow_bwd failed ({rc})")
        return (None, None, None, None, None, gx.view(R, D), gcond.view(R, C), *grads)


class _AffineCoupling(nn.Module):
    def __init__(self, dim, cond_dim, hidden, clamp=1.9):
        super().__init__()
        self.d1 = dim // 2
        self.d2 = dim - self.d1
        self.clamp = clamp
        self.net1 = _mlp(self.d1 + cond_dim, hidden, 2 * self.d2, act=nn.ELU, keras_init=False)
        self.net2 = _mlp(self.d2 + cond_dim, hidden, 2 * self.d1, act=nn.ELU, keras_init=False)

    def _st(self, net, h, cond):
        s, t = net(torch.cat([h, cond], dim=-1)).chunk(2, dim=-1)
        return self.clamp * torch.tanh(s / self.clamp), t


    def forward(self, x, cond):
        """-> (y, [s_a, s_b]): the log-scales are summed ONCE by the caller for all layers (one cat + one sum instead of a
        sum and an add per half layer, forward and backward).  (The PyTorch composition; the fused form is _FusedFlowFn.)"""
        x1, x2 = x[:, :self.d1], x[:, self.d1:]
        sa, t = self._st(self.net1, x1, cond)
        y2 = torch.addcmul(t, x2, torch.exp(sa))               # x2 * exp(s) + t, one kernel fewer each way
        sb, t = self._st(self.net2, y2, cond)
        y1 = torch.addcmul(t, x1, torch.exp(sb))
        return torch.cat([y1, y2], dim=-1), [sa, sb]

    def inverse(self, y, cond, scales=None):
        """scales: a list that receives the two log-scales [s_b, s_a] -- the forward's, at the point this returns."""
        y1, y2 = y[:, :self.d1], y[:, self.d1:]
        sb, t = self._st(self.net2, y2, cond)
        x1 = (y1 - t) * torch.exp(-sb)
        sa, t = self._st(self.net1, x1, cond)
        x2 = (y2 - t) * torch.exp(-sa)
        if scales is not None:
            scales += [sb, sa]
        return torch.cat([x1, x2], dim=-1)


class InvertibleNetwork(nn.Module):
    """bf.networks.InvertibleNetwork(num_params): conditional normalising flow of affine coupling layers with fixed
    permutations and a learnable ActNorm in front of each."""

    def __init__(self, num_params, cond_dim=11, num_coupling_layers=6, hidden=128, seed=0):
        super().__init__()
        self.num_params = num_params
        self.layers = nn.ModuleList(_AffineCoupling(num_params, cond_dim, hidden) for _ in range(num_coupling_layers))
        g = torch.Generator().manual_seed(seed)
        # fixed permutations, applied as products with 0/1 matrices: a column gather costs an index kernel forward and an
        # index_put with a radix sort backward (five launches), the 5 x 5 product one each way
        for i in range(num_coupling_layers):
            perm = torch.randperm(num_params, generator=g)
            self.register_buffer(f"perm{i}", perm)
            # (derived from perm{i}: not part of the state dict, rebuilt after a load -- a mismatched pair cannot be loaded)
            self.register_buffer(f"pmat{i}", torch.eye(num_params)[:, perm].contiguous(), persistent=False)
        # one parameter per layer (not rows of one matrix: selecting a row costs autograd a zero-fill and a copy each way)
        self.an_scale = nn.ParameterList(nn.Parameter(torch.zeros(num_params)) for _ in range(num_coupling_layers))
        self.an_bias = nn.ParameterList(nn.Parameter(torch.zeros(num_params)) for _ in range(num_coupling_layers))
        self.fused = True           # the hand-written kernels where they apply (False: always the PyTorch composition)
        self._refresh_host_perms()  # (host copies: reading the buffers back would synchronise, which a graph capture forbids)
        self.register_load_state_dict_post_hook(self._refresh_host_perms)

    def _fused_lib(self, theta, cond, rows_limit=True):
        """libnddm_train.so if the fused flow covers this network and these tensors, else None (the PyTorch composition).
        rows_limit=False: the sampler's gate (csrc/train_sample.hip takes any number of draws)."""
        if not (self.fused and len(self.layers) and theta.is_cuda and theta.dtype == torch.float32 and cond.dtype == torch.float32
                and (theta.shape[0] <= self.FUSED_MAX_ROWS or not rows_limit)):
            return None
        l0 = self.layers[0]
        if any(len(n) != 5 or not isinstance(n[1], nn.ELU) for l in self.layers for n in (l.net1, l.net2)):
            return None
        from . import _train_lib
        L = _train_lib.lib()
        ok = L is not None and L.nddm_train_flow_supported(l0.net1[0].weight.shape[0], len(self.layers), self.num_params, l0.d1,
                                                           cond.shape[1])
        return L if ok else None

    # (the fused kernels take 16 rows per workgroup, and one workgroup per half-layer sums the weight gradients over all rows:
    # made for the training loop's batches of 32 ... a few hundred rows)
    FUSED_MAX_ROWS = 4096
    # a GraphTrainer may set {"grads": {parameter data_ptr: its slot in the trainer's flat gradient buffer}, "loss": the loss's slot}:
    # the backward then writes every gradient (and the forward the loss) where the optimizer reads them -- no gather copies
    grad_sink = None

    def _flow_params(self):
        params = []
        for i, l in enumerate(self.layers):
            params += [self.an_scale[i], self.an_bias[i]]
            params += [t for n in (l.net1, l.net2) for k in (0, 2, 4) for t in (n[k].weight, n[k].bias)]
        return params

    def nll(self, theta, cond):
        """mean(|z|^2 / 2 - log|det|): the maximum-likelihood loss of bf.amortizers.AmortizedPosterior."""
        L = self._fused_lib(theta, cond)
        if L is not None:
            return _FusedFlowFn.apply((L, self.grad_sink), self.layers[0].clamp, self.layers[0].d1, self._perm_host, True, theta, cond, *self._flow_params())
        z, log_det = self(theta, cond)
        return (0.5 * (z ** 2).sum(-1) - log_det).mean()

    def _refresh_host_perms(self, *_):
        self._perm_host = [getattr(self, f"perm{i}").tolist() for i in range(len(self.layers))]
        with torch.no_grad():
            for i, perm in enumerate(self._perm_host):
                pm = getattr(self, f"pmat{i}")
                pm.copy_(torch.eye(self.num_params)[:, perm])

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        """Checkpoints of earlier layouts: ActNorm's log-scale and bias were ONE [layers, D] tensor each (now one parameter per
        layer, `an_scale.0` ...), and `pmat{i}` used to be stored (now derived from `perm{i}`)."""
        for name in ("an_scale", "an_bias"):
            old = state_dict.pop(prefix + name, None)
            if old is not None:
                for i in range(old.shape[0]):
                    state_dict.setdefault(f"{prefix}{name}.{i}", old[i].clone())
        for i in range(len(self.layers)):
            state_dict.pop(f"{prefix}pmat{i}", None)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def forward(self, theta, cond):
        L = self._fused_lib(theta, cond)
        if L is not None:
            return _FusedFlowFn.apply((L, self.grad_sink), self.layers[0].clamp, self.layers[0].d1, self._perm_host, False, theta, cond, *self._flow_params())
        z, scales = theta, []
        for i, layer in enumerate(self.layers):
            z = torch.addcmul(self.an_bias[i], z, torch.exp(self.an_scale[i]))
            z = z @ getattr(self, f"pmat{i}")                 # == z[:, perm]
            z, s2 = layer(z, cond)
            scales += s2
        return z, torch.cat(scales, dim=-1).sum(-1) + torch.cat(list(self.an_scale)).sum()

    def inverse(self, z, cond):
        x = z
        for i in reversed(range(len(self.layers))):
            x = self.layers[i].inverse(x, cond)
            x = x @ getattr(self, f"pmat{i}").t()             # == x[:, argsort(perm)]
            x = (x - self.an_bias[i]) * torch.exp(-self.an_scale[i])
        return x

    def inverse_with_log_density(self, z, cond):
        """`inverse` with the log-scales kept: z [R, D], cond [R, C] -> (theta [R, D], log_q [R]), the flow's own log density at the draw
        it returns, log q(theta | cond) = -|z|^2 / 2 - (D / 2) log 2 pi + log|det| -- the forward's log|det| is the sum of the SAME
        soft-clamped log-scales the inverse forms on its way (each half-layer sees the inputs the forward's sees) and of the ActNorm
        log-scales.  The PyTorch composition: the fallback of inverse_per_set(log_density=True) and the fused sampler's yardstick."""
        x, scales = z, []
        for i in reversed(range(len(self.layers))):
            x = self.layers[i].inverse(x, cond, scales)
            x = x @ getattr(self, f"pmat{i}").t()
            x = (x - self.an_bias[i]) * torch.exp(-self.an_scale[i])
        log_det = torch.cat(scales, dim=-1).sum(-1) + torch.cat(list(self.an_scale)).sum()
        return x, -0.5 * (z ** 2).sum(-1) - 0.5 * self.num_params * math.log(2.0 * math.pi) + log_det

    def _sample_lib(self, z, cond):
        """libnddm_train.so if the fused sampler covers z [B, S, D] with one condition row per set, cond [B, C]; else None.  The
        kernel is no autograd node: where a gradient could be asked for, the PyTorch composition serves."""
        if z.dim() != 3 or cond.dim() != 2 or z.shape[0] != cond.shape[0] or z.numel() == 0 or z.device != cond.device:
            return None
        if torch.is_grad_enabled() and (z.requires_grad or cond.requires_grad or any(p.requires_grad for p in self.parameters())):
            return None
        return self._fused_lib(z.reshape(-1, z.shape[-1]), cond, rows_limit=False)

    def _fused_sample(self, L, z, cond, box=None, draws=True, moments=False, out=None, sums=None, n_outside=None, log_q=False,
                      log_q_out=None):
        """One launch of csrc/train_sample.hip on z [B, S, D], cond [B, C] -> (theta [B, S, D] or None, sums [B, 2 D] float64 or None,
        n_outside [B] int64 or None): the draws (draws=True), and / or (moments=True) per set the float64 sums of theta and of
        theta^2 over the draws INSIDE -- every component finite and, with box = (lo [D], hi [D]) float32 tensors, within it -- and
        the number of draws outside.  out / sums / n_outside: contiguous tensors to write into (else allocated here).
        log_q=True appends a fourth item, log_q [B, S] float32 (written into log_q_out if given): the flow's own log density at each
        draw, from the same launch -- the other three keep their bits (inverse_with_log_density is the PyTorch form)."""
        import ctypes
        (B, S, D), C, dev, nl = z.shape, cond.shape[1], z.device, len(self.layers)
        params = self._flow_params()
        ptrs = (ctypes.c_void_p * (14 * nl))(*[p.data_ptr() for p in params])
        perm = (ctypes.c_int * (nl * D))(*[int(v) for p in self._perm_host for v in p])
        z, cond = z.contiguous(), cond.contiguous()
        if draws and out is None:
            out = torch.empty(B, S, D, dtype=torch.float32, device=dev)
        if moments:
            sums = torch.empty(B, 2 * D, dtype=torch.float64, device=dev) if sums is None else sums
            n_outside = torch.empty(B, dtype=torch.int64, device=dev) if n_outside is None else n_outside
        if log_q and log_q_out is None:
            log_q_out = torch.empty(B, S, dtype=torch.float32, device=dev)
        lo, hi = (None, None) if box is None else (v.to(dev, torch.float32).contiguous() for v in box)
        work = torch.empty(int(L.nddm_train_flow_sample_work_bytes(B, S, D)), dtype=torch.uint8, device=dev)
        ptr = lambda v: None if v is None else v.data_ptr()       # noqa: E731
        args = (params[4].shape[0], nl, B, S, D, self.layers[0].d1, C, float(self.layers[0].clamp), ptrs, perm, z.data_ptr(), cond.data_ptr(),
                ptr(out) if draws else None, ptr(lo), ptr(hi), ptr(sums) if moments else None, ptr(n_outside) if moments else None)
        st = torch.cuda.current_stream(dev).cuda_stream
        if log_q:
            rc = L.nddm_train_flow_sample_logq(*args, log_q_out.data_ptr(), work.data_ptr(), st)
        else:
            rc = L.nddm_train_flow_sample(*args, work.data_ptr(), st)
        if rc != 0:
            raise RuntimeError(f"nddm_train_flow_sample failed ({rc})")
        res = (out if draws else None), (sums if moments else None), (n_outside if moments else None)
        return res + (log_q_out,) if log_q else res

    def inverse_per_set(self, z, cond, log_density=False):
        """The inverse on draws grouped by data set: z [B, S, D] base normals, cond [B, C] ONE condition row per set -> [B, S, D].
        Where the fused sampler applies (cuda, float32, the shapes of nddm_train_flow_supported, self.fused, no gradient asked for) it
        is one kernel that never expands the condition (csrc/train_sample.hip); otherwise `inverse` on the condition repeated S
        times -- the same map.  log_density=True -> (theta [B, S, D], log_q [B, S]): the flow's log density at each draw as well, from
        the same kernel, or from inverse_with_log_density."""
        B, S, D = z.shape
        L = self._sample_lib(z, cond)
        if L is not None:
            if log_density:
                res = self._fused_sample(L, z, cond, log_q=True)
                return res[0], res[3]
            return self._fused_sample(L, z, cond)[0]
        if log_density:
            th, lq = self.inverse_with_log_density(z.reshape(B * S, D), cond.repeat_interleave(S, dim=0))
            return th.reshape(B, S, D), lq.reshape(B, S)
        return self.inverse(z.reshape(B * S, D), cond.repeat_interleave(S, dim=0)).reshape(B, S, D)


def _quantile_lib(theta, n_probs):
    """libnddm_train.so if its selection kernel (csrc/train_quantile.hip) covers theta [B, S, D] and this many probabilities, else
    None (draw_quantiles' PyTorch evaluation of the same definition)."""
    if not (theta.is_cuda and theta.dtype == torch.float32 and theta.is_contiguous() and 1 <= theta.shape[2] <= 8
            and 1 <= n_probs <= 16):
        return None
    from . import _train_lib
    L = _train_lib.lib()
    return L if L is not None and theta.shape[1] <= L.nddm_train_draw_quantiles_max_draws() else None


@torch.no_grad()
def draw_quantiles(theta, probs, box=None):
    """Exact quantiles of draws per (set, column): theta [B, S, D] (or [S, D]: one set), probs K probabilities in [0, 1] ->
    {"quantiles" [B, K, D] float64, "order" [B, K, 2, D] float32, "n_inside" [B] int64}, tensors on theta's device.

    A row (draw) is INSIDE if all its D components are finite and, with box = (low, high) of length D, within it -- the mask is per
    row, as posterior_moments'.  With x_(0) <= ... <= x_(n-1) the inside values of a column, in float64: h = (n - 1) * p, j = floor(h),
    g = h - j, a = x_(j), b = x_(min(j + 1, n - 1)); order = (a, b) as the float32 values themselves and quantile = a + (b - a) * g,
    each operation rounded on its own: np.quantile's default rule (NumPy forms h otherwise: equal to rounding, not bit for bit).  No
    inside row: nan, n_inside 0.  Zeros come back as +0.

    On the device (float32, contiguous, D <= 8, S <= the kernel's cap, K <= 16) one kernel sorts each (set, column)'s keys in LDS
    (csrc/train_quantile.hip); everywhere else -- a CPU, more draws, no library -- torch.sort evaluates the same definition, and the
    two agree bit for bit."""
    p = np.ascontiguousarray(np.asarray(probs, dtype=np.float64).reshape(-1))
    if p.size == 0 or not np.all((p >= 0.0) & (p <= 1.0)):
        raise ValueError("probs must be probabilities in [0, 1]")
    if theta.dim() == 2:
        theta = theta[None]
    if theta.dim() != 3 or theta.numel() == 0:
        raise ValueError(f"theta must be [B, S, D] (or [S, D]) and not empty; got {tuple(theta.shape)}")
    (B, S, D), K, dev = theta.shape, p.size, theta.device
    if box is not None:
        box = tuple(v.to(dev, torch.float32).contiguous() if torch.is_tensor(v) else torch.as_tensor(np.asarray(v, dtype=np.float32), device=dev)
                    for v in box)
        if len(box) != 2 or box[0].shape != (D,) or box[1].shape != (D,):
            raise ValueError(f"box must be a (low, high) pair of length-{D} sequences")
    L = _quantile_lib(theta, K)
    if L is not None:
        quant = torch.empty(B, K, D, dtype=torch.float64, device=dev)
        order = torch.empty(B, K, 2, D, dtype=torch.float32, device=dev)
        n_in = torch.empty(B, dtype=torch.int64, device=dev)
        lo, hi = (None, None) if box is None else (box[0].data_ptr(), box[1].data_ptr())
        rc = L.nddm_train_draw_quantiles(B, S, D, theta.data_ptr(), lo, hi, p.ctypes.data, K, quant.data_ptr(), order.data_ptr(),
                                         n_in.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"nddm_train_draw_quantiles failed ({rc})")
        return {"quantiles": quant, "order": order, "n_inside": n_in}
    th = theta.to(torch.float32)
    inside = torch.isfinite(th).all(dim=-1)
    if box is not None:
        inside &= ((th >= box[0]) & (th <= box[1])).all(dim=-1)
    n_in = inside.sum(dim=1)
    # (+ 0.0: -0 becomes +0, as in the kernel's keys; outside rows sort to the end)
    srt = torch.sort(torch.where(inside[..., None], th + 0.0, torch.full((), float("inf"), device=dev)), dim=1).values
    last = n_in.clamp(min=1) - 1
    h = last.double()[:, None] * torch.as_tensor(p, device=dev)[None, :]                 # [B, K]
    fl = h.floor()
    g, j = (h - fl)[..., None], fl.long()
    j1 = torch.minimum(j + 1, last[:, None])
    a = torch.gather(srt, 1, j[..., None].expand(B, K, D))
    b = torch.gather(srt, 1, j1[..., None].expand(B, K, D))
    empty = (n_in == 0)[:, None, None]
    nan32 = torch.full((), float("nan"), device=dev)
    a, b = torch.where(empty, nan32, a), torch.where(empty, nan32, b)
    ad, bd = a.double(), b.double()
    return {"quantiles": ad + (bd - ad) * g, "order": torch.stack([a, b], dim=2), "n_inside": n_in}


WEIGHT_ONE = 2 ** 36        # the integer weight of a set's largest finite log weight (quantize_weights)


@torch.no_grad()
def quantize_weights(log_w):
    """Log weights [B, S] (or [S]) -> integer weights, int64 of the same shape, per set (the last dimension): with m the largest FINITE
    log_w of the set, W = rint(exp(log_w - m) * 2^36) in float64 (torch.round: half to even), and 0 where log_w is not finite (NaN, +-inf).  So 0 <= W <= 2^36, the
    largest is exactly 2^36, and a draw below 2^-37 of the largest weighs nothing.  Sums of up to 32 768 such weights are exact in int64
    and in float64, whatever the order: what weighted_draw_quantiles' definition stands on."""
    lw = log_w.to(torch.float64)
    fin = torch.isfinite(lw)
    ninf = torch.full((), float("-inf"), dtype=torch.float64, device=lw.device)
    m = torch.where(fin, lw, ninf).max(dim=-1, keepdim=True).values
    u = torch.round(torch.exp(lw - m) * float(WEIGHT_ONE))
    return torch.where(fin, u, torch.zeros((), dtype=torch.float64, device=lw.device)).to(torch.int64)


def _wquantile_lib(theta, n_probs, w):
    """libnddm_train.so if its weighted selection kernel (csrc/train_wquantile.hip) covers theta [B, S, D], this many probabilities and
    w [B, S] (float64 log weights or int64 weights), else None (weighted_draw_quantiles' PyTorch evaluation of the same definition)."""
    if not (theta.is_cuda and theta.dtype == torch.float32 and theta.is_contiguous() and 1 <= theta.shape[2] <= 8 and 1 <= n_probs <= 16
            and w.device == theta.device and w.is_contiguous() and w.dtype in (torch.float64, torch.int64)):
        return None
    from . import _train_lib
    L = _train_lib.lib()
    return L if L is not None and theta.shape[1] <= L.nddm_train_weighted_quantiles_max_draws() else None


@torch.no_grad()
def weighted_draw_quantiles(theta, probs, log_w=None, weights=None, want_weights=False):
    """Exact WEIGHTED quantiles of draws per (set, column): theta [B, S, D] (or [S, D]: one set), probs K probabilities in [0, 1], and
    EXACTLY ONE of log_w [B, S] (log weights: importance_weights' "log_w") and weights [B, S] int64 in [0, 2^36] (quantize_weights'
    output; the range is the caller's to keep) -> {"quantiles" [B, K, D] float64, "order" [B, K, 2, D] float32, "n_positive" [B] int64;
    "weights" [B, S] int64 with want_weights}, tensors on theta's device.

    The definition is on the integer weights W = quantize_weights(log_w), so that every sum is exact and every route agrees bit for
    bit.  A row is INSIDE if W >= 1 and all its D components are finite (no box: the prior term of an importance weight has already
    zeroed what a box would remove); n_positive counts them.  Per column the inside rows sorted by value (-0 taken as +0), ties by row
    index: x_0 <= ... <= x_(n-1) with weights W_0 .. W_(n-1), S_k = W_0 + ... + W_k, c_k = 2 S_k - W_k - W_0 (so c_0 = 0 and
    c_(k+1) - c_k = W_k + W_(k+1) > 0) and T = c_(n-1).  For p, in float64 with every operation rounded on its own: h = p T; k the
    largest index with c_k <= h; if k = n - 1: a = b = x_(n-1), g = 0; else a = x_k, b = x_(k+1), g = (h - c_k) / (W_k + W_(k+1));
    order = (a, b) and quantile = a + (b - a) g.  Equal weights give draw_quantiles' rule (np.quantile's default) bit for bit; p = 0
    gives the smallest inside value and p = 1 the largest; the quantile is non-decreasing in p.  No inside row: nan, n_positive 0.

    On the device (float32 contiguous theta, D <= 8, K <= 16, S <= the kernel's cap, 16 384) one kernel sorts each (set, column)'s
    (key, row) items in LDS and scans the integer weights in sorted order (csrc/train_wquantile.hip); everywhere else -- a CPU, more
    draws, no library -- a stable torch.sort, an int64 cumsum and searchsorted evaluate the same definition.  Given `weights` the two
    agree bit for bit; given log_w they can differ only through exp, by at most 1 in a W."""
    p = np.ascontiguousarray(np.asarray(probs, dtype=np.float64).reshape(-1))
    if p.size == 0 or not np.all((p >= 0.0) & (p <= 1.0)):
        raise ValueError("probs must be probabilities in [0, 1]")
    if (log_w is None) == (weights is None):
        raise ValueError("give exactly one of log_w and weights")
    if theta.dim() == 2:
        theta = theta[None]
        log_w, weights = (None if v is None else v.reshape(1, -1) for v in (log_w, weights))
    if theta.dim() != 3 or theta.numel() == 0:
        raise ValueError(f"theta must be [B, S, D] (or [S, D]) and not empty; got {tuple(theta.shape)}")
    (B, S, D), K, dev = theta.shape, p.size, theta.device
    w = log_w if weights is None else weights
    if tuple(w.shape) != (B, S) or w.device != dev:
        raise ValueError(f"log_w / weights must be [{B}, {S}] on theta's device; got {tuple(w.shape)} on {w.device}")
    if weights is not None and weights.dtype != torch.int64:
        raise ValueError(f"weights must be int64 (quantize_weights' output); got {weights.dtype}")
    w = w.contiguous() if weights is not None else w.to(torch.float64).contiguous()
    L = _wquantile_lib(theta, K, w)
    if L is not None:
        quant = torch.empty(B, K, D, dtype=torch.float64, device=dev)
        order = torch.empty(B, K, 2, D, dtype=torch.float32, device=dev)
        n_pos = torch.empty(B, dtype=torch.int64, device=dev)
        w_out = torch.empty(B, S, dtype=torch.int64, device=dev) if want_weights and weights is None else None
        rc = L.nddm_train_weighted_quantiles(B, S, D, theta.data_ptr(), w.data_ptr() if weights is None else None,
                                             None if weights is None else w.data_ptr(), p.ctypes.data, K, quant.data_ptr(), order.data_ptr(),
                                             n_pos.data_ptr(), None if w_out is None else w_out.data_ptr(),
                                             torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"nddm_train_weighted_quantiles failed ({rc})")
        res = {"quantiles": quant, "order": order, "n_positive": n_pos}
        if want_weights:
            res["weights"] = w if w_out is None else w_out
        return res
    W = w if weights is not None else quantize_weights(w)
    th = theta.to(torch.float32)
    inside = torch.isfinite(th).all(dim=-1) & (W >= 1)
    n = inside.sum(dim=1)
    # (+ 0.0: -0 becomes +0, as in the kernel's keys; rows not inside sort to the end with weight 0; stable: ties by row index)
    srt, idx = torch.sort(torch.where(inside[..., None], th + 0.0, torch.full((), float("inf"), device=dev)), dim=1, stable=True)
    Ws = torch.gather(torch.where(inside, W, torch.zeros((), dtype=torch.int64, device=dev))[..., None].expand(B, S, D), 1, idx)
    c = 2 * torch.cumsum(Ws, dim=1) - Ws - Ws[:, :1]                                     # [B, S, D]: increasing up to n - 1, larger after
    last = (n.clamp(min=1) - 1)[:, None, None].expand(B, 1, D)
    h = torch.as_tensor(p, device=dev)[None, :, None] * torch.gather(c, 1, last).double()   # [B, K, D]
    cd = c.double().transpose(1, 2).contiguous()                                        # [B, D, S] (exact: every c <= 2^52)
    k = (torch.searchsorted(cd, h.transpose(1, 2).contiguous(), right=True) - 1).transpose(1, 2)      # [B, K, D]: the largest k with c_k <= h
    k = torch.minimum(k.clamp(min=0), last)
    k1 = torch.minimum(k + 1, last)
    a, b = torch.gather(srt, 1, k), torch.gather(srt, 1, k1)
    step = (torch.gather(Ws, 1, k) + torch.gather(Ws, 1, k1)).double()
    g = torch.where(k == last, torch.zeros((), dtype=torch.float64, device=dev), (h - torch.gather(c, 1, k).double()) / step)
    empty = (n == 0)[:, None, None]
    nan32 = torch.full((), float("nan"), device=dev)
    a, b = torch.where(empty, nan32, a), torch.where(empty, nan32, b)
    ad, bd = a.double(), b.double()
    res = {"quantiles": ad + (bd - ad) * g, "order": torch.stack([a, b], dim=2), "n_positive": n}
    if want_weights:
        res["weights"] = W
    return res


def _importance_lib(theta, log_q, log_lik):
    """libnddm_train.so if its weight-and-reduce kernel (csrc/train_importance.hip) covers these tensors, else None
    (importance_weights' torch evaluation of the same definition)."""
    if not (theta.is_cuda and log_q.device == theta.device and log_lik.device == theta.device and theta.dtype == torch.float32
            and log_q.dtype == torch.float32 and log_lik.dtype == torch.float64 and theta.is_contiguous() and log_q.is_contiguous()
            and log_lik.is_contiguous() and 1 <= theta.shape[2] <= 8):
        return None
    from . import _train_lib
    return _train_lib.lib()


def _log_prior_torch(table, th):
    """priors.log_prior_density in torch float64 on th [..., P]'s device (table: priors.prior_table's host array)."""
    ninf = torch.full((), float("-inf"), dtype=torch.float64, device=th.device)
    out = torch.zeros(th.shape[:-1], dtype=torch.float64, device=th.device)
    for d, (kind, p1, p2, lo, hi, ln) in enumerate(table.tolist()):
        x = th[..., d]
        if kind in (0.0, 1.0):
            u = (x - p1) / p2
            lp = -0.5 * u * u - ln
        elif kind == 2.0:
            lp = torch.full_like(x, -ln)
            if p1 != 1.0:
                lp = lp + (p1 - 1.0) * torch.log(x)
            if p2 != 1.0:
                lp = lp + (p2 - 1.0) * torch.log1p(-x)
        else:
            lp = torch.full_like(x, -ln)
        out = out + torch.where(torch.isfinite(x) & (x >= lo) & (x <= hi), lp, ninf)
    return out


@torch.no_grad()
def importance_weights(theta, log_q, log_lik, prior, want_log_w=False, out=None):
    """Self-normalised importance sampling of a proposal's draws against the exact posterior, per data set: theta [B, S, D] draws of
    q (or [S, D]: one set), log_q [B, S] their log density under q (InvertibleNetwork.inverse_per_set(log_density=True)), log_lik [B, S]
    the exact log-likelihood of the set's data at each draw (diagnostics.posterior_log_likelihood), prior a model name of
    priors.PRIOR_DENSITY ("basic", "single", "scale"), such a description, or priors.prior_table's array ->
    {"log_evidence", "ess", "max_share" [B]; "mean", "sd" [B, D] float64; "n_zero", "n_nan" [B] int64; "log_w" [B, S] float64 with
    want_log_w}, tensors on theta's device.  In float64, per draw
        log w = log_lik + log prior(theta) - log_q
    with weight 0 (log w = -inf), in this order: where the log prior is -inf -- a component outside its support or not finite --
    whatever log_lik holds (counted in n_zero); else where log_lik or log_q is NaN (counted in n_nan, and only there: nothing is
    swept under the rug); else where log_lik or log w is -inf (n_zero); else where log w is +inf (n_nan).  With m = max log w and
    u = exp(log w - m):  log_evidence = m + log(sum u / S), an estimate of log p(data) -- by S, not by the number of positive
    weights: a draw of q outside the prior's support is a draw whose weight is zero;  ess = (sum u)^2 / sum u^2;  max_share =
    1 / sum u, the largest normalised weight;  mean, sd the weighted moments (ddof 0, the variance clamped at 0).  A set without
    a positive weight: nan mean, sd and max_share, ess 0, log_evidence -inf.

    On the device (float32 contiguous theta and log_q, float64 log_lik, D <= 8) one kernel, a workgroup per set, the float64 sums in
    a fixed order (csrc/train_importance.hip: bit-reproducible, a set's numbers independent of B); everywhere else the same
    definition in torch float64.  The two agree to the summation bound and a few ulp of exp, not bit for bit.
    out: a dict of contiguous tensors, by the result's keys, to write into (posterior_importance's slices)."""
    from . import priors
    table = np.ascontiguousarray(prior if isinstance(prior, np.ndarray) else priors.prior_table(prior), dtype=np.float64)
    if theta.dim() == 2:
        theta, log_q, log_lik = theta[None], log_q.reshape(1, -1), log_lik.reshape(1, -1)
    if theta.dim() != 3 or theta.numel() == 0:
        raise ValueError(f"theta must be [B, S, D] (or [S, D]) and not empty; got {tuple(theta.shape)}")
    (B, S, D), dev = theta.shape, theta.device
    if tuple(log_q.shape) != (B, S) or tuple(log_lik.shape) != (B, S) or table.shape != (D, 6):
        raise ValueError(f"log_q and log_lik must be [{B}, {S}] and the prior have {D} columns")
    L = _importance_lib(theta, log_q, log_lik)
    if L is not None:
        o = dict(out or {})
        for k, shape, dt in (("log_evidence", (B,), torch.float64), ("ess", (B,), torch.float64), ("max_share", (B,), torch.float64),
                             ("mean", (B, D), torch.float64), ("sd", (B, D), torch.float64), ("n_zero", (B,), torch.int64),
                             ("n_nan", (B,), torch.int64)) + ((("log_w", (B, S), torch.float64),) if want_log_w else ()):
            if k not in o:
                o[k] = torch.empty(shape, dtype=dt, device=dev)
        tab = torch.as_tensor(table, device=dev)
        st = torch.cuda.current_stream(dev)
        rc = L.nddm_train_importance(B, S, D, theta.data_ptr(), log_q.data_ptr(), log_lik.data_ptr(), tab.data_ptr(),
                                     o["log_evidence"].data_ptr(), o["ess"].data_ptr(), o["max_share"].data_ptr(), o["mean"].data_ptr(),
                                     o["sd"].data_ptr(), o["n_zero"].data_ptr(), o["n_nan"].data_ptr(),
                                     o["log_w"].data_ptr() if want_log_w else None, st.cuda_stream)
        if rc != 0:
            raise RuntimeError(f"nddm_train_importance failed ({rc})")
        return o                                                  # (tab was made on this stream: the allocator reuses it in stream order)
    th, lq, ll = theta.double(), log_q.double(), log_lik.double()
    ninf = torch.full((), float("-inf"), dtype=torch.float64, device=dev)
    lp = _log_prior_torch(table, th)
    zero_prior = lp == ninf
    nan = ~zero_prior & (torch.isnan(ll) | torch.isnan(lq))
    lw = torch.where(zero_prior | nan | (ll == ninf), ninf, ll + lp - lq)
    nan = nan | (~zero_prior & (torch.isnan(lw) | (lw == float("inf"))))
    lw = torch.where(nan, ninf, lw)
    m = lw.max(dim=1, keepdim=True).values
    u = torch.where(lw == ninf, torch.zeros((), dtype=torch.float64, device=dev), torch.exp(lw - torch.where(m == ninf, torch.zeros_like(m), m)))
    tz = torch.where((u > 0)[..., None], th, torch.zeros((), dtype=torch.float64, device=dev))      # (a zero weight's draw may not be finite)
    sw, sw2 = u.sum(dim=1), (u * u).sum(dim=1)
    any_w = sw > 0
    nan64 = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    mean = (u[..., None] * tz).sum(dim=1) / sw[:, None]
    var = (u[..., None] * (tz * tz)).sum(dim=1) / sw[:, None] - mean * mean
    res = {"log_evidence": torch.where(any_w, m[:, 0] + torch.log(sw / S), ninf), "ess": torch.where(any_w, sw * sw / sw2, torch.zeros_like(sw)),
           "max_share": torch.where(any_w, 1.0 / sw, nan64), "mean": torch.where(any_w[:, None], mean, nan64),
           "sd": torch.where(any_w[:, None], var.clamp_min(0.0).sqrt(), nan64), "n_zero": ((lw == ninf) & ~nan).sum(dim=1),
           "n_nan": nan.sum(dim=1)}
    if want_log_w:
        res["log_w"] = lw
    for k, v in (out or {}).items():
        if k in res:
            res[k] = v.copy_(res[k])
    return res


@torch.no_grad()
def weighted_moments(theta, log_w, out=None):
    """The moments of GIVEN log weights: theta [B, S, D] draws (or [S, D]: one set), log_w [B, S] -> importance_weights' result --
    {"log_evidence", "ess", "max_share" [B]; "mean", "sd" [B, D]; "n_zero", "n_nan" [B]} -- with log_w in the place of log_lik + log
    prior - log_q: the same kernel (csrc/train_importance.hip) with a zero log_q and a NEUTRAL prior table (every column uniform on
    (-inf, inf) with log normaliser 0), so the kernel's log w is log_w + 0 - 0, the given number.  What pareto_smooth's log weights go
    through.  A NaN or +inf log weight is counted in n_nan and weighs nothing, as there; a draw with a non-finite component counts
    in n_zero.  out: importance_weights' (a dict of tensors to write into)."""
    if theta.dim() == 2:
        theta, log_w = theta[None], log_w.reshape(1, -1)
    if theta.dim() != 3 or theta.numel() == 0 or tuple(log_w.shape) != tuple(theta.shape[:2]):
        raise ValueError(f"theta must be [B, S, D] (or [S, D]), not empty, and log_w [B, S]; got {tuple(theta.shape)} and {tuple(log_w.shape)}")
    D = theta.shape[2]
    neutral = np.tile(np.array([3.0, 0.0, 0.0, -np.inf, np.inf, 0.0]), (D, 1))      # (priors.PRIOR_KINDS["uniform"] = 3)
    log_q = torch.zeros(theta.shape[:2], dtype=torch.float32, device=theta.device)
    return importance_weights(theta, log_q, log_w.to(torch.float64).contiguous(), neutral, out=out)


PSIS_LOG_DBL_MIN = -708.3964185322641      # log(DBL_MIN): the floor of pareto_smooth's cutoff


def pareto_tail_size(S):
    """M = min(ceil(S / 5), ceil(3 sqrt(S))), in integers: how many of a set's S weights pareto_smooth fits at most."""
    S = int(S)
    return min((S + 4) // 5, math.isqrt(9 * S - 1) + 1)


def pareto_k_threshold(S):
    """min(1 - 1 / log10(S), 0.7): the pareto_k below which an importance-sampling estimate from S draws is reliable."""
    S = int(S)
    return min(1.0 - 1.0 / math.log10(S), 0.7) if S > 1 else float("-inf")


def _psis_lib(log_w):
    """libnddm_train.so if its smoothing kernel (csrc/train_psis.hip) covers log_w [B, S], else None (pareto_smooth's torch evaluation)."""
    if not (log_w.is_cuda and log_w.dtype == torch.float64 and log_w.is_contiguous()):
        return None
    from . import _train_lib
    L = _train_lib.lib()
    return L if L is not None and log_w.shape[1] <= L.nddm_train_pareto_smooth_max_draws() else None


def _pareto_smooth_torch(lw, M, want_log_w):
    """pareto_smooth's definition on lw [B, S] float64 on any device, every set at once and without a host synchronisation ->
    (pareto_k, sigma, cutoff [B] float64, n_tail [B] int64, the smoothed log weights [B, S] or None).  A stable sort gives the cutoff and
    the tail in (value, row) order as its last M columns; a set's n <= M tail rows are the last n of those, the others are masked."""
    (B, S), dev = lw.shape, lw.device
    c = lambda v: torch.full((), v, dtype=torch.float64, device=dev)                      # noqa: E731
    fin = torch.isfinite(lw)
    m = torch.where(fin, lw, c(-math.inf)).max(dim=1, keepdim=True).values                # (-inf: no finite log weight, every x -inf)
    xs, idx = torch.sort(torch.where(fin, lw - m, c(-math.inf)), dim=1, stable=True)      # ascending by value, ties by row index
    cutoff = (xs[:, S - M - 1] if S - M - 1 >= 0 else c(-math.inf).expand(B)).clamp_min(PSIS_LOG_DBL_MIN)
    tx, rows = xs[:, S - M:], idx[:, S - M:]
    inside = tx > cutoff[:, None]
    n = inside.sum(dim=1)
    nd, fit = n.double(), n > 4
    e_c = torch.exp(cutoff)[:, None]
    y = torch.where(inside, torch.exp(tx) - e_c, c(0.0))
    first = M - n                                                                         # the column of rank 0
    m_est = 30.0 + torch.floor(torch.sqrt(nd))
    j = torch.arange(1, 31 + math.isqrt(M), dtype=torch.float64, device=dev)[None, :]
    live = j <= m_est[:, None]
    yq = y.gather(1, (first + torch.floor(nd / 4.0 + 0.5).long() - 1).clamp(0, M - 1)[:, None])

    def mean_log1p(b):                                                                    # b [B, J] -> mean over the tail of log1p(-b y), [B, J]
        return torch.where(inside[:, None, :], torch.log1p(-b[:, :, None] * y[:, None, :]), c(0.0)).sum(dim=2) / nd[:, None]

    bj = (1.0 - torch.sqrt(m_est[:, None] / (j - 0.5))) / (3.0 * yq) + 1.0 / y[:, M - 1:]
    kj = mean_log1p(bj)
    Lj = nd[:, None] * (torch.log(-bj / kj) - kj - 1.0)
    wj = torch.where(live, 1.0 / torch.where(live[:, None, :], torch.exp(Lj[:, None, :] - Lj[:, :, None]), c(0.0)).sum(dim=2), c(0.0))
    b = torch.where(live, bj * (wj / wj.sum(dim=1, keepdim=True)), c(0.0)).sum(dim=1)
    k_raw = mean_log1p(b[:, None])[:, 0]
    sigma = torch.where(fit, -k_raw / b, c(math.nan))
    k = torch.where(fit, (nd * k_raw + 5.0) / (nd + 10.0), c(math.inf))
    if not want_log_w:
        return k, sigma, cutoff, n, None
    apply = fit & torch.isfinite(k) & torch.isfinite(sigma) & (sigma > 0.0)
    lp = torch.log1p(-((torch.arange(M, device=dev)[None, :] - first[:, None]).double() + 0.5) / nd[:, None])
    q = torch.where((k == 0.0)[:, None], -sigma[:, None] * lp, sigma[:, None] * torch.expm1(-k[:, None] * lp) / k[:, None])
    new = torch.where(apply[:, None] & inside, m + torch.log(q + e_c).clamp_max(0.0), lw.gather(1, rows))
    return k, sigma, cutoff, n, lw.clone().scatter_(1, rows, new)                          # (every other row: its input bits)


@torch.no_grad()
def pareto_smooth(log_w, want_log_w=True, out=None):
    """Pareto-smoothed importance sampling (Vehtari, Simpson, Gelman, Yao, Gabry) of log weights [B, S] (or [S]: one set), per set ->
    {"pareto_k", "sigma", "cutoff" [B] float64, "n_tail" [B] int64; "log_w" [B, S] float64 with want_log_w}, tensors on log_w's device.
    pareto_k (k-hat) is the shape of a generalised Pareto distribution fitted to the set's largest weights, the diagnostic:
    below pareto_k_threshold(S) (0.7 from 1000 draws on) an estimate from these weights is reliable at this sample size, above it
    it is not -- whatever ess and max_share say, which look healthy on a sample that has not met the heavy tail yet.  "log_w" holds
    the input with those largest weights replaced by the fitted distribution's expected order statistics (a lower-variance estimate;
    feed it to weighted_moments and weighted_draw_quantiles).

    The definition, float64, one set: a log weight that is not finite (NaN, +-inf) is a weight of zero (quantize_weights' rule); m the
    largest finite log_w, x = log_w - m (-inf where not finite); M = pareto_tail_size(S); c the order statistic of rank S - M - 1 of x
    (ascending, 0-based; -inf if the rank is negative); cutoff = max(c, log DBL_MIN).  The tail is the rows with x > cutoff, strictly (so
    n_tail <= M; a value equal to the cutoff stays out), ordered by value, ties by row index.  No finite log weight or n_tail <= 4:
    pareto_k = +inf, sigma = nan, "log_w" is the input.  Else y_r = exp(x_(r)) - exp(cutoff) and Zhang and Stephens' estimator with the
    PSIS prior: m_est = 30 + isqrt(n) candidates b_j = (1 - sqrt(m_est / (j - 0.5))) / (3 y_q) + 1 / y_(n-1), q = floor(n / 4 + 0.5) - 1;
    k_j = mean_r log1p(-b_j y_r); L_j = n (log(-b_j / k_j) - k_j - 1); w_j = 1 / sum_i exp(L_i - L_j), normalised; b = sum_j b_j w_j;
    k_raw = mean_r log1p(-b y_r); sigma = -k_raw / b; pareto_k = (n k_raw + 5) / (n + 10).  If pareto_k and sigma are finite and sigma
    > 0 the tail row of rank r becomes m + min(log(q_r + exp(cutoff)), 0), q_r = sigma expm1(-pareto_k log1p(-p_r)) / pareto_k at p_r =
    (r + 0.5) / n; otherwise "log_w" is the input and pareto_k is reported as computed.  Every other row keeps its input bits.

    On the device (float64 contiguous log_w, S <= the kernel's cap, 16 384) one kernel, a workgroup per set (csrc/train_psis.hip: an
    exact selection of the cutoff, the tail ranked in LDS, the fit's sums in a fixed tree -- bit-reproducible, a set's numbers
    independent of B, unchanged by a permutation of distinct rows); everywhere else -- a CPU, more draws, no library -- a torch float64
    evaluation of the same definition, every set at once.  n_tail, cutoff and which rows change agree exactly; pareto_k, sigma and the
    smoothed values to the summation order and a few ulp of exp / log1p / expm1 (tests/psis_ref.py::tolerances).
    out: a contiguous float64 tensor [B, S] on log_w's device, not log_w itself, to write "log_w" into (posterior_importance's scratch)."""
    if log_w.dim() == 1:
        log_w = log_w[None]
    if log_w.dim() != 2 or log_w.numel() == 0:
        raise ValueError(f"log_w must be [B, S] (or [S]) and not empty; got {tuple(log_w.shape)}")
    (B, S), dev = log_w.shape, log_w.device
    lw = log_w.to(torch.float64).contiguous()
    M = pareto_tail_size(S)
    if not want_log_w:
        out = None
    elif out is not None and (tuple(out.shape) != (B, S) or out.dtype != torch.float64 or out.device != dev or not out.is_contiguous()
                              or out.data_ptr() == lw.data_ptr()):
        raise ValueError(f"out must be a contiguous float64 tensor [{B}, {S}] on log_w's device and not log_w itself")
    L = _psis_lib(lw)
    if L is not None:
        res = {k: torch.empty(B, dtype=torch.float64, device=dev) for k in ("pareto_k", "sigma", "cutoff")}
        res["n_tail"] = torch.empty(B, dtype=torch.int64, device=dev)
        if want_log_w and out is None:
            out = torch.empty(B, S, dtype=torch.float64, device=dev)
        rc = L.nddm_train_pareto_smooth(B, S, M, lw.data_ptr(), None if out is None else out.data_ptr(), res["pareto_k"].data_ptr(),
                                        res["sigma"].data_ptr(), res["n_tail"].data_ptr(), res["cutoff"].data_ptr(),
                                        torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"nddm_train_pareto_smooth failed ({rc})")
        if want_log_w:
            res["log_w"] = out
        return res
    per = max(1, (8 << 20) // ((31 + math.isqrt(M)) * M))                # sets per pass: the fit's [sets, candidates, M] terms within 64 MB
    parts = [_pareto_smooth_torch(lw[b0:b0 + per], M, want_log_w) for b0 in range(0, B, per)]
    res = {key: torch.cat([p[i] for p in parts]) for i, key in enumerate(("pareto_k", "sigma", "cutoff", "n_tail"))}
    if want_log_w:
        res["log_w"] = torch.cat([p[4] for p in parts]) if out is None else out.copy_(torch.cat([p[4] for p in parts]))
    return res


RESAMPLE_MAX_OUT = 2 ** 20     # the largest M resample_draws' kernel takes: the comb's 64-bit terms stay below 2^63 up to here


def resample_words(B, seed=0):
    """One 64-bit word per data set for resample_draws: uint64 [B] (numpy) from np.random.Generator(np.random.Philox(seed)), so torch's
    generator is never touched.  Set b's word is words[b] whatever the launch split; the first B' words of a longer call are the same."""
    B = int(B)
    if B < 1:
        raise ValueError("resample_words needs B >= 1")
    return np.random.Generator(np.random.Philox(int(seed))).integers(0, 2 ** 64, size=B, dtype=np.uint64)


def _resample_lib(theta, M, w):
    """libnddm_train.so if its resampling kernel (csrc/train_resample.hip) covers theta [B, S, D], M outputs and w [B, S] (float64 log
    weights or int64 weights), else None (resample_draws' PyTorch evaluation of the same definition)."""
    if not (theta.is_cuda and theta.dtype == torch.float32 and theta.is_contiguous() and 1 <= theta.shape[2] <= 8 and 1 <= M <= RESAMPLE_MAX_OUT
            and w.device == theta.device and w.is_contiguous() and w.dtype in (torch.float64, torch.int64)):
        return None
    from . import _train_lib
    L = _train_lib.lib()
    return L if L is not None and theta.shape[1] <= L.nddm_train_resample_max_draws() and M <= L.nddm_train_resample_max_out() else None


@torch.no_grad()
def resample_draws(theta, M, log_w=None, weights=None, words=None, seed=0, want_weights=False):
    """Sampling-importance-resampling: S weighted draws per data set -> M EQUALLY weighted draws of the weighted sample (of the exact
    posterior, when the weights are importance_weights').  theta [B, S, D] (or [S, D]: one set), EXACTLY ONE of log_w [B, S] (log
    weights) and weights [B, S] int64 in [0, 2^36] (quantize_weights' output; the range is the caller's to keep), words: one 64-bit
    word per set (a uint64 array [B], an int64 tensor of the same bits, or None: resample_words(B, seed)) -> {"draws" [B, M, D]
    float32, "ancestors" [B, M] int32, "n_unique", "n_positive" [B] int64; "weights" [B, S] int64 with want_weights}, tensors on
    theta's device.

    The definition is on the integer weights W = quantize_weights(log_w), so that every sum is exact and every route agrees on every
    ancestor.  V_i = W_i if all D components of row i are finite, else 0 (weighted_draw_quantiles' inside rule; n_positive counts the
    rows with V_i >= 1).  Running sums IN ROW ORDER, no sort: C_k = V_0 + ... + V_k, T = C_(S-1).  The offset U = (r T) >> 64, the high
    half of the 128-bit product of the set's word r (unsigned) and T: 0 <= U < T, uniform when r is.  The systematic comb t_j =
    floor((j T + U) / M), j = 0 .. M - 1; the ancestor a_j is the smallest k with C_k > t_j, and draws[j] = theta[a_j], the float32
    bits copied.  n_unique is the number of distinct ancestors.  So a_j does not decrease in j, a row of weight 0 is never chosen, row
    k appears floor or ceil of M V_k / T times (|n_k T - M V_k| < T), equal weights with M = S give a_j = j, and summed over all T
    offsets row k is chosen exactly M V_k times: exactly unbiased given a uniform U.  A set with T = 0: NaN draws, ancestors -1,
    n_unique 0.

    On the device (float32 contiguous theta, D <= 8, S <= the kernel's cap, 16 384, M <= 2^20) one kernel, a workgroup per set, scans
    the integer weights in LDS and searches them per output (csrc/train_resample.hip); everywhere else -- a CPU, more draws, no
    library, a larger M -- an int64 cumsum and searchsorted evaluate the same definition, U in Python integers on the host.  Given
    `weights` the two agree bit for bit; given log_w they can differ only through exp, by at most 1 in a W."""
    M = int(M)
    if M < 1:
        raise ValueError("M must be at least 1")
    if (log_w is None) == (weights is None):
        raise ValueError("give exactly one of log_w and weights")
    if theta.dim() == 2:
        theta = theta[None]
        log_w, weights = (None if v is None else v.reshape(1, -1) for v in (log_w, weights))
    if theta.dim() != 3 or theta.numel() == 0:
        raise ValueError(f"theta must be [B, S, D] (or [S, D]) and not empty; got {tuple(theta.shape)}")
    (B, S, D), dev = theta.shape, theta.device
    w = log_w if weights is None else weights
    if tuple(w.shape) != (B, S) or w.device != dev:
        raise ValueError(f"log_w / weights must be [{B}, {S}] on theta's device; got {tuple(w.shape)} on {w.device}")
    if weights is not None and weights.dtype != torch.int64:
        raise ValueError(f"weights must be int64 (quantize_weights' output); got {weights.dtype}")
    w = w.contiguous() if weights is not None else w.to(torch.float64).contiguous()
    if words is None:
        words = resample_words(B, seed)
    if torch.is_tensor(words):
        if words.dtype not in (torch.int64, torch.uint64) or tuple(words.shape) != (B,):
            raise ValueError(f"words must be {B} 64-bit words; got {words.dtype} {tuple(words.shape)}")
        words_t = words.view(torch.int64).to(dev).contiguous()
    else:
        words = np.asarray(words)
        if words.dtype != np.uint64 or words.shape != (B,):
            raise ValueError(f"words must be a uint64 array [{B}] (resample_words); got {words.dtype} {words.shape}")
        words_t = None
    L = _resample_lib(theta, M, w)
    if L is not None:
        if words_t is None:
            words_t = torch.from_numpy(np.ascontiguousarray(words).view(np.int64)).to(dev)
        out = torch.empty(B, M, D, dtype=torch.float32, device=dev)
        anc = torch.empty(B, M, dtype=torch.int32, device=dev)
        n_uni, n_pos = torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.int64, device=dev)
        w_out = torch.empty(B, S, dtype=torch.int64, device=dev) if want_weights and weights is None else None
        rc = L.nddm_train_resample(B, S, D, M, theta.data_ptr(), w.data_ptr() if weights is None else None,
                                   None if weights is None else w.data_ptr(), words_t.data_ptr(), out.data_ptr(), anc.data_ptr(),
                                   n_uni.data_ptr(), n_pos.data_ptr(), None if w_out is None else w_out.data_ptr(),
                                   torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"nddm_train_resample failed ({rc})")
        res = {"draws": out, "ancestors": anc, "n_unique": n_uni, "n_positive": n_pos}
        if want_weights:
            res["weights"] = w if w_out is None else w_out
        return res
    W = w if weights is not None else quantize_weights(w)
    th = theta.to(torch.float32)
    V = torch.where(torch.isfinite(th).all(dim=-1), W, torch.zeros((), dtype=torch.int64, device=dev))
    C = torch.cumsum(V, dim=1)                                                            # [B, S] int64: exact
    T = C[:, -1]
    r = [int(v) & (2 ** 64 - 1) for v in (words_t.tolist() if words_t is not None else words.tolist())]
    U = torch.tensor([(rb * Tb) >> 64 for rb, Tb in zip(r, T.tolist())], dtype=torch.int64, device=dev)      # Python integers: exact
    fl = lambda a, d: torch.div(a, d, rounding_mode="floor")                              # noqa: E731  (non-negative int64)
    q, qU = fl(T, M), fl(U, M)
    rho, rhoU = T - q * M, U - qU * M
    j = torch.arange(M, dtype=torch.int64, device=dev)[None, :]
    tj = j * q[:, None] + qU[:, None] + fl(j * rho[:, None] + rhoU[:, None], M)           # [B, M]
    empty = (T == 0)[:, None]
    a = torch.searchsorted(C, tj, right=True).clamp(max=S - 1)                            # the smallest k with C_k > t_j (T = 0: masked below)
    out = torch.gather(th, 1, a[..., None].expand(B, M, D))
    out = torch.where(empty[..., None], torch.full((), float("nan"), device=dev), out)
    n_uni = torch.where(empty[:, 0], torch.zeros((), dtype=torch.int64, device=dev), 1 + (a[:, 1:] != a[:, :-1]).sum(dim=1))
    a = torch.where(empty, torch.full((), -1, dtype=torch.int64, device=dev), a)
    res = {"draws": out, "ancestors": a.to(torch.int32), "n_unique": n_uni, "n_positive": (V >= 1).sum(dim=1)}
    if want_weights:
        res["weights"] = W
    return res


class SingleTrialTarget:
    """What posterior_importance(..., target=...) weighs the draws against: the single-trial model's MARGINAL likelihood (the latent
    per-trial boundary integrated out, engine.wiener_marginal_log_likelihood) under its prior RESTRICTED to the rows that likelihood's
    accuracy is stated on (priors.restricted_density, priors.MARGINAL_DOMAIN).  Made by single_trial_target."""

    def __init__(self, t_censor, gamma, domain):
        from . import priors
        self.t_censor, self.gamma = t_censor, gamma
        self.model, self.num_params = ("scale", 8) if gamma is None else ("single", 7)
        self.domain = dict(domain)
        self.density = priors.restricted_density(self.model, self.domain)

    def __repr__(self):
        return f"SingleTrialTarget(t_censor={self.t_censor!r}, gamma={self.gamma!r}, domain={self.domain!r})"


def single_trial_target(t_censor, gamma=1.0, domain=None):
    """The target of posterior_importance / sample_exact for the single-trial model (single_trial_alpha_not_scaled): its marginal
    likelihood and its restricted prior.

    t_censor: the decision time a timeout (choicert == 0) is censored at, the simulator's max_steps * dt, >= 0; None or 0: a timeout
    has no likelihood, its draws' weights are NaN and counted in "n_nan".  gamma: 1.0 -- the reference's main model, a 7-column flow
    (drift, mu_alpha, beta, ter, std_alpha, dc, sigma1), gamma fixed at 1 -- or None: the flow's 8th column is gamma ("scale", gamma ~
    U(0, 2)).  Another fixed gamma is not covered: the kernel's 7-column row is gamma = 1.  domain: None (priors.MARGINAL_DOMAIN) or
    lower bounds of std_alpha, dc, sigma1 by name, as priors.restricted_density takes them."""
    from . import priors
    tc = 0.0 if t_censor is None else float(t_censor)
    if math.isnan(tc) or tc < 0:
        raise ValueError("t_censor must be >= 0 (or None: timeouts then have no likelihood)")
    if gamma is not None and float(gamma) != 1.0:
        raise ValueError("gamma must be 1.0 (a 7-column flow, gamma fixed at 1) or None (the flow's 8th column is gamma)")
    return SingleTrialTarget(tc, None if gamma is None else 1.0, priors.MARGINAL_DOMAIN if domain is None else domain)


def observed_batch(datasets, device=None):
    """Observed data sets of DIFFERENT trial counts -- a sequence of arrays [n_b, d], a participant each -- as ONE amortizer input:
    {"summary_conditions": float32 [B, max n_b, d], set b's trials first and ZEROS after them; "summary_counts": int32 [B], the n_b;
    "direct_conditions": float32 [B, 1], log n_b (what the models' configurators compute from sim_non_batchable_context)}, torch
    tensors on `device` (None: the CPU).  With it

        post = amortizer.sample(observed_batch(per_participant), 1000, fused=True)

    replaces the reference's loop of one configurator(...) and one amortizer.sample(...) per participant (fitting_stahl_data.py:
    196-211); posterior_moments, posterior_summary and log_posterior take the same dict.  The summary network never reads the
    padding.  posterior_importance does, and the ZERO padding is what makes it work there: a row (rt 0, choice 0) is to basic_ddm_dc's
    likelihood a censored timeout at t = 0 - tau <= 0, which scores log 1 = 0 (csrc/nddm_wiener.h), so a padded set's likelihood
    is its own trials'."""
    sets = [np.asarray(s, dtype=np.float32) for s in datasets]
    if not sets:
        raise ValueError("observed_batch needs at least one data set")
    if any(s.ndim != 2 or s.shape[0] < 1 for s in sets):
        raise ValueError("every data set must be an array [n_b, d] with n_b >= 1 trials")
    d = sets[0].shape[1]
    if d < 1 or any(s.shape[1] != d for s in sets):
        raise ValueError(f"every data set must have the same number of columns; got {sorted({s.shape[1] for s in sets})}")
    counts = np.array([s.shape[0] for s in sets], dtype=np.int32)
    x = np.zeros((len(sets), int(counts.max()), d), dtype=np.float32)
    for b, s in enumerate(sets):
        x[b, :s.shape[0]] = s
    out = {"summary_conditions": x, "summary_counts": counts, "direct_conditions": np.log(counts.astype(np.float64)).astype(np.float32)[:, None]}
    return {k: torch.as_tensor(v, device=device) for k, v in out.items()}


class AmortizedPosterior(nn.Module):
    """bf.amortizers.AmortizedPosterior(inference_net, summary_net): maximum-likelihood training of q(theta | data)."""

    def __init__(self, inference_net, summary_net):
        super().__init__()
        self.inference_net, self.summary_net = inference_net, summary_net

    def _t(self, v):
        dev = next(self.parameters()).device
        return v.to(dev, torch.float32) if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v), dtype=torch.float32, device=dev)

    def _conditions(self, input_dict):
        pad = input_dict.get("summary_mask", None)        # (mask, inv_n) of a batch padded to a bucket length (additive keys), or
        nv = input_dict.get("summary_n", None)            # the number of real trials, a device scalar
        x = self._t(input_dict["summary_conditions"])
        direct = input_dict.get("direct_conditions", None)
        direct = None if direct is None else self._t(direct)
        cnt = input_dict.get("summary_counts", None)      # a trial count per set (additive key): a ragged batch, `observed_batch`
        if cnt is not None:
            if pad is not None or nv is not None:
                raise ValueError("summary_counts (a trial count per set) cannot be combined with summary_mask / summary_n (batch-shared)")
            if not isinstance(self.summary_net, InvariantNetwork):
                raise TypeError("summary_counts needs a summary network that takes a count per set (InvariantNetwork)")
            # inference (sample, posterior_*, log_posterior) through the kernels, training through the differentiable definition
            return self.summary_net(x, counts=cnt, direct=direct) if torch.is_grad_enabled() else self.summary_net.summarize(x, cnt, direct)
        if direct is not None and isinstance(self.summary_net, InvariantNetwork):
            # (the summary network appends the direct conditions itself: with the kernels, without a concatenation)
            if nv is not None:
                return self.summary_net(x, n_valid=nv, direct=direct)
            return self.summary_net(x, direct=direct) if pad is None else self.summary_net(x, pad[0], pad[1], direct=direct)
        if nv is not None:
            summ = self.summary_net(x, n_valid=nv)
        else:
            summ = self.summary_net(x) if pad is None else self.summary_net(x, pad[0], pad[1])
        return summ if direct is None else torch.cat([summ, direct], dim=-1)

    def forward(self, input_dict):
        return self.inference_net(self._t(input_dict["parameters"]), self._conditions(input_dict))

    def compute_loss(self, input_dict):
        theta, cond = self._t(input_dict["parameters"]), self._conditions(input_dict)
        if hasattr(self.inference_net, "nll"):
            return self.inference_net.nll(theta, cond)
        z, log_det = self.inference_net(theta, cond)
        return (0.5 * (z ** 2).sum(-1) - log_det).mean()

    @torch.no_grad()
    def sample(self, input_dict, n_samples, to_numpy=True, reject_outside=None, max_redraws=16, fused=False):
        """amortizer.sample(dict, n_samples) (basic_ddm_dc.py:223): [n_samples, P] for a single data set,
        [B, n_samples, P] for a batch.

        reject_outside: None (the default: every draw of the flow is returned, which is what the reference's call gets) or a
        (low, high) pair of length-P sequences -- draws with a component outside [low, high] (or non-finite) are REDRAWN from fresh
        base normals, i.e. the sample is from q(theta | data) restricted to the box.  Why one might want it: a sharply trained
        coupling flow carries ~1e-6 of its mass in a far tail (one draw in 1e5-1e6 lands 1e4-1e6 prior widths away, DESIGN.md
        section 8), and a posterior MEAN over 10 000 draws -- the statistic the reference's recovery plots use, basic_ddm_dc.py:
        230-236 -- is carried off by one such draw; `priors.prior_box(model)` is a generous box (the prior's support widened by
        its own width on each side) that removes them and nothing else.  The number of redrawn draws of the last call is kept in
        `self.last_redrawn` (0 with the option off).

        fused=True: the same base normals (the generator is consumed identically) go through `inverse_per_set` -- on the device one
        kernel for all draws, which reads each data set's condition row once instead of n_samples copies of it (csrc/
        train_sample.hip) -- and the few redrawn rows through the PyTorch inverse.  The draws agree with the default's to float32
        round-off (tests/test_gpu_flow_sample.py), not bit for bit; the default (False) is the PyTorch composition, unchanged."""
        cond = self._conditions(input_dict)
        B = cond.shape[0]
        P = self.inference_net.num_params
        z = torch.randn(B * n_samples, P, device=cond.device)
        if fused and hasattr(self.inference_net, "inverse_per_set"):
            out = self.inference_net.inverse_per_set(z.view(B, n_samples, P), cond).reshape(B * n_samples, P)
            cond_rows = lambda idx: cond[torch.div(idx, n_samples, rounding_mode="floor")]      # noqa: E731
        else:
            cond_rep = cond.repeat_interleave(n_samples, dim=0)
            out = self.inference_net.inverse(z, cond_rep)
            cond_rows = lambda idx: cond_rep[idx]                                                 # noqa: E731
        self.last_redrawn = 0
        if reject_outside is not None:
            lo, hi = (torch.as_tensor(np.asarray(v, dtype=np.float32), device=out.device) for v in reject_outside)
            if lo.shape != (P,) or hi.shape != (P,):
                raise ValueError(f"reject_outside must be a (low, high) pair of length-{P} sequences")
            for _ in range(int(max_redraws)):
                bad = ((out < lo) | (out > hi) | ~torch.isfinite(out)).any(dim=-1)
                idx = bad.nonzero(as_tuple=False)[:, 0]
                if idx.numel() == 0:
                    break
                self.last_redrawn += int(idx.numel())
                out[idx] = self.inference_net.inverse(torch.randn(idx.numel(), P, device=out.device), cond_rows(idx))
            out = torch.minimum(torch.maximum(torch.nan_to_num(out, nan=0.0), lo), hi)      # (what max_redraws rounds did not cure: clipped)
        out = out.reshape(B, n_samples, -1)
        if B == 1:
            out = out[0]
        return out.cpu().numpy() if to_numpy else out

    @torch.no_grad()
    def posterior_moments(self, input_dict, n_samples, box=None, z_bytes=64 << 20):
        """Posterior mean and standard deviation of every data set from n_samples draws each, WITHOUT keeping the draws:
        {"mean" [B, P], "sd" [B, P] (population, ddof 0, as the reference's np.var), "n_outside" [B], "n_samples"}, float64 (numpy).

        box: None or a (low, high) pair of length-P sequences.  A draw is INSIDE if every component is finite and, with a box,
        within [low, high]; the moments are over the inside draws and `n_outside` counts the others.  With box=priors.prior_box(
        model) this is the tail-safe posterior mean (see `sample`: one draw in 1e5-1e6 of a sharply trained flow lands far outside
        the prior): leaving the outside draws out of the mean is the same law as redrawing them.  A set with no inside draw
        has nan moments.

        On the device the sums are accumulated in float64 by the sampler itself in a fixed order (csrc/train_sample.hip:
        bit-reproducible), whole data sets per launch, as many as keep the base normals of a launch within z_bytes.  Elsewhere
        (a CPU, a shape the kernel does not cover) the same numbers come from the PyTorch inverse's draws, summed in float64.  The
        base normals are torch.randn(sets * n_samples, P) per launch: those of sample() whenever one launch holds all B sets."""
        return self._moments(*self._moment_sums(input_dict, n_samples, box, z_bytes), n_samples)

    @staticmethod
    def _moments(sums, n_out, n_samples):
        P = sums.shape[1] // 2
        n_in = (n_samples - n_out).double()[:, None]
        mean = sums[:, :P] / n_in
        sd = (sums[:, P:] / n_in - mean * mean).clamp_min(0.0).sqrt()
        return {"mean": mean.cpu().numpy(), "sd": sd.cpu().numpy(), "n_outside": n_out.cpu().numpy(), "n_samples": int(n_samples)}

    def _moment_sums(self, input_dict, n_samples, box, z_bytes, on_draws=None):
        """posterior_moments' loop -> (sums [B, 2 P] float64, n_outside [B] int64), device tensors.  on_draws(theta [sets, n_samples, P],
        box): called after every launch with that launch's draws (a scratch buffer that the next launch overwrites) and the box
        as device tensors; the sampler then writes the draws as well as the sums."""
        cond = self._conditions(input_dict)
        B, P, dev, net = cond.shape[0], self.inference_net.num_params, cond.device, self.inference_net
        if box is not None:
            box = tuple(torch.as_tensor(np.asarray(v, dtype=np.float32), device=dev) for v in box)
            if box[0].shape != (P,) or box[1].shape != (P,):
                raise ValueError(f"box must be a (low, high) pair of length-{P} sequences")
        sums = torch.empty(B, 2 * P, dtype=torch.float64, device=dev)
        n_out = torch.empty(B, dtype=torch.int64, device=dev)
        per = max(1, int(z_bytes) // max(1, 4 * n_samples * P))
        scratch = None
        for b0 in range(0, B, per):
            c = cond[b0:b0 + per]
            nb = c.shape[0]
            z = torch.randn(nb * n_samples, P, device=dev)
            L = net._sample_lib(z.view(nb, n_samples, P), c) if hasattr(net, "_sample_lib") else None
            if L is not None:
                if on_draws is not None and scratch is None:
                    scratch = torch.empty(min(per, B), n_samples, P, dtype=torch.float32, device=dev)
                net._fused_sample(L, z.view(nb, n_samples, P), c, box=box, draws=on_draws is not None, moments=True,
                                  out=None if on_draws is None else scratch[:nb], sums=sums[b0:b0 + nb], n_outside=n_out[b0:b0 + nb])
                if on_draws is not None:
                    on_draws(scratch[:nb], box)
                continue
            th = net.inverse(z, c.repeat_interleave(n_samples, dim=0)).reshape(nb, n_samples, P)
            if on_draws is not None:
                on_draws(th.contiguous(), box)
            inside = torch.isfinite(th).all(dim=-1)
            if box is not None:
                inside &= ((th >= box[0]) & (th <= box[1])).all(dim=-1)
            th = torch.where(inside[..., None], th.double(), torch.zeros((), dtype=torch.float64, device=dev))
            sums[b0:b0 + nb] = torch.cat([th.sum(dim=1), (th * th).sum(dim=1)], dim=-1)
            n_out[b0:b0 + nb] = (~inside).sum(dim=1)
        return sums, n_out

    # pyhddmjagsutils.summary's names for the quantiles its recovery plots draw
    SUMMARY_NAMES = {0.5: "median", 0.025: "95lower", 0.975: "95upper", 0.005: "99lower", 0.995: "99upper"}

    @torch.no_grad()
    def posterior_summary(self, input_dict, n_samples, probs=(.005, .025, .5, .975, .995), box=None, z_bytes=64 << 20, keep_draws=False):
        """The reference's posterior summary (pyhddmjagsutils.summary: mean, std, median, 95 % and 99 % credible intervals) of every
        data set from n_samples draws each, without the draws leaving the device:
        {"mean", "std", "median", "95lower", "95upper", "99lower", "99upper" [B, P] each; "quantiles" [B, K, P], "probs" [K],
        "n_outside" [B], "n_samples"}, float64 (numpy).  A named quantile is present when `probs` holds its probability (.5, .025,
        .975, .005, .995).  keep_draws=True adds "draws" [B, n_samples, P] float32 (small B, tests).

        posterior_moments' loop and random stream: whole data sets per launch, torch.randn(sets * n_samples, P) per launch, as
        many sets as keep the base normals within z_bytes; `mean`, `std` (its `sd`) and `n_outside` are that call's numbers, bit for
        bit under the same seed, box and z_bytes.  Each launch's draws go into one scratch buffer of the base normals' size (so
        the call holds up to 2 x z_bytes: fewer sets per launch would consume torch.randn otherwise than posterior_moments does),
        which `draw_quantiles` turns into exact order statistics on the same stream before the next launch overwrites it.  box:
        posterior_moments' -- the quantiles are over the inside draws, the sample the moments use.  Where the fused sampler does
        not apply the draws come from the PyTorch inverse and the quantiles from draw_quantiles' fallback."""
        p = np.asarray(probs, dtype=np.float64).reshape(-1)
        if p.size == 0 or not np.all((p >= 0.0) & (p <= 1.0)):
            raise ValueError("probs must be probabilities in [0, 1]")
        quants, kept = [], []

        def on_draws(theta, box_t):
            quants.append(draw_quantiles(theta, p, box=box_t)["quantiles"])
            if keep_draws:
                kept.append(theta.clone())

        m = self._moments(*self._moment_sums(input_dict, n_samples, box, z_bytes, on_draws), n_samples)
        q = torch.cat(quants, dim=0).cpu().numpy()
        out = {"mean": m["mean"], "std": m["sd"]}
        for k, pk in enumerate(p):
            name = self.SUMMARY_NAMES.get(float(pk))
            if name is not None:
                out[name] = q[:, k, :]
        out.update(quantiles=q, probs=p, n_outside=m["n_outside"], n_samples=int(n_samples))
        if keep_draws:
            out["draws"] = torch.cat(kept, dim=0).cpu().numpy()
        return out

    @torch.no_grad()
    def posterior_importance(self, input_dict, n_samples, model="basic", z_bytes=64 << 20, keep_draws=False, keep_weights=False, probs=None,
                             smooth=False, resample=None, resample_seed=0, _resampled_on_device=False, target=None):
        """The amortizer's draws importance-weighted against the EXACT posterior of every data set (importance_weights: log w =
        log p(data | theta) + log p(theta) - log q(theta | data)), without the draws leaving the device:
        {"mean", "std" [B, P]: the weighted posterior moments -- a consistent estimate of the exact posterior's, whatever the
        amortizer's error, and a far-tail draw simply has weight 0;  "ess" [B]: the effective sample size, per data set how good the
        amortizer is;  "log_evidence" [B]: an estimate of log p(data);  "max_share" [B]: the largest normalised weight;  "n_zero",
        "n_nan" [B], "n_samples"}, float64 / int64 (numpy).  keep_draws=True adds "draws" [B, n_samples, P] float32 and "log_q"
        [B, n_samples] float32, keep_weights=True "log_w" [B, n_samples] float64 (small B, tests).

        posterior_moments' loop and random stream: whole data sets per launch, torch.randn(sets * n_samples, P) per launch, as
        many sets as keep the base normals within z_bytes -- the draws are those of sample(..., fused=True) under the same seed
        whenever one launch holds all sets.  Per launch three kernels, all on torch's current stream (engine launches there too):
        the fused sampler writes draws and log q into scratch (csrc/train_sample.hip), the broadcast-layout Wiener likelihood scores
        them against the set's trials, input_dict["summary_conditions"] -- basic_ddm_dc's (rt, choice), timeouts right-censored --
        and csrc/train_importance.hip weighs and reduces.  Where the fused sampler does not apply the draws and log q come from
        inverse_with_log_density.  model: "basic" only; the single-trial models' likelihood is not wired here yet.

        probs: None (the default: the call above, nothing more launched or allocated) or K probabilities in [0, 1] -- the WEIGHTED
        quantiles of the exact posterior as well (weighted_draw_quantiles' definition on the call's own log weights): the result gains
        "quantiles" [B, K, P] and "probs" [K] and, for the probabilities pyhddmjagsutils.summary names (.5, .025, .975, .005, .995),
        "median", "95lower", "95upper", "99lower", "99upper" [B, P] -- with probs=(.005, .025, .5, .975, .995) the reference's whole
        summary under the exact posterior.  Each launch then keeps its log weights in a scratch buffer [sets, n_samples] float64 and
        a fourth kernel (csrc/train_wquantile.hip, up to 16 384 draws; the torch evaluation beyond) turns draws and weights into
        quantiles on the same stream before the next launch overwrites them; every other number keeps its bits.

        A ragged batch (`observed_batch`: "summary_counts") needs nothing more, because its padding is ZEROS: the likelihood scores
        all max n_b rows of every set, and a row (rt 0, choice 0) is a timeout censored at t = -tau <= 0, log 1 = 0 exactly, so each
        set's log-likelihood is its own trials' (tests/test_gpu_ragged_summary.py).  Padding of any other value would be scored.

        smooth: False (the default: the call above, its bits and its launches) or True -- Pareto-smoothed importance sampling.  Each
        launch's log weights then go through pareto_smooth into a second scratch buffer [sets, n_samples] float64 (csrc/train_psis.hip, up
        to 16 384 draws; the torch evaluation beyond), weighted_moments launches csrc/train_importance.hip a second time on the smoothed
        weights, and with probs the weighted quantiles are taken on them.  "mean", "std", "ess", "max_share", "log_evidence" and the
        quantiles are then those of the SMOOTHED weights, and the result gains "pareto_k" [B] float64 -- the diagnostic: at or above
        "k_threshold" (pareto_k_threshold(n_samples), a float) a set's numbers are not to be trusted at this sample size, whatever
        its ess says -- "n_tail" [B] int64, and "raw": a dict of the unsmoothed "mean", "std", "ess", "max_share" and "log_evidence", the
        smooth=False call's bits under the same seed.  keep_weights=True also returns "log_w_smoothed" [B, n_samples] float64.

        resample: None (the default: the call above, its keys, bits, launches and allocations) or M >= 1 -- sampling-importance-
        resampling: the result gains "resampled" [B, M, P] float32, M EQUALLY weighted draws of the exact posterior per data set
        (resample_draws' definition on the call's own log weights -- the smoothed ones with smooth=True -- and the words
        resample_words(B, resample_seed): set b's word is words[b] whatever the launch split), "n_unique" [B] int64, how many different
        draws they are, and "resample_seed".  Each launch's draws and log weights go through one more kernel (csrc/train_resample.hip, up
        to 16 384 draws and M <= 2^20; the torch evaluation beyond) on the same stream before the next launch overwrites them.  Every
        other number keeps its bits, and torch's random stream is consumed exactly as without the option.  (_resampled_on_device:
        sample_exact's -- "resampled" stays a device tensor instead of making the way to the host.)

        target: None (the default: the call above, its keys, bits, launches, allocations and use of torch's random stream) or a
        single_trial_target(t_censor, gamma) -- the single-trial model (`model` is then the target's).  summary_conditions are its
        (choicert, z1) [B, N, 2]; the flow has 7 columns (gamma = 1) or 8 (gamma=None), ValueError otherwise.  The likelihood launch is
        the marginal one, one quadrature per (draw, trial), on the draws as the sampler leaves them -- the kernel reads 7-column rows --
        and "summary_counts", if present, goes to it as a trial count per set: the padding is never read, whatever it holds.  THE
        PRIOR IS THE RESTRICTED ONE, priors.restricted_density(target.model): std_alpha >= 0.02, dc >= 0.05, sigma1 >= 0.02, the rows
        the marginal kernel's accuracy is stated on; a draw outside has weight 0 and is counted in "n_zero".  The result gains
        "domain", those lower bounds, and every number -- "log_evidence" too -- is that of the RESTRICTED model: the posterior given
        that the parameters lie in the domain, not the reference prior's.  A timeout in the data with t_censor 0 gives NaN
        likelihoods, counted in "n_nan".  Everything after the weights (probs, smooth, resample, keep_*) is the path above."""
        if target is None:
            if model != "basic":
                raise NotImplementedError(f"posterior_importance scores model='basic' only; for {model!r} the next step is the marginal "
                                          "likelihood, likelihood.single_trial_logpdf, as the target")
        else:
            if not isinstance(target, SingleTrialTarget):
                raise TypeError("target must be None or a single_trial_target(...)")
            if model not in ("basic", target.model):
                raise ValueError(f"model {model!r} contradicts the target's {target.model!r}")
            if self.inference_net.num_params != target.num_params:
                raise ValueError(f"the target (gamma={target.gamma!r}) takes a flow of {target.num_params} parameters; this one has "
                                 f"{self.inference_net.num_params}")
            shape = tuple(getattr(input_dict["summary_conditions"], "shape", ()))
            if len(shape) != 3 or shape[2] != 2:
                raise ValueError(f"the single-trial model's summary_conditions are (choicert, z1) trials [B, N, 2], got {shape}")
        from . import engine, priors
        if target is not None:
            try:
                engine.require_device()
            except ImportError as e:                                    # (no library: the same refusal as no device)
                raise RuntimeError(f"posterior_importance with a target needs the HIP library and a ROCm GPU: {e}") from e
        if probs is not None:
            probs = np.asarray(probs, dtype=np.float64).reshape(-1)
            if probs.size == 0 or not np.all((probs >= 0.0) & (probs <= 1.0)):
                raise ValueError("probs must be probabilities in [0, 1]")
        if resample is not None and int(resample) < 1:
            raise ValueError("resample must be None or a number of draws M >= 1")
        table = priors.prior_table(model if target is None else target.density)
        cond = self._conditions(input_dict)
        data = self._t(input_dict["summary_conditions"])
        B, P, dev, net, S = cond.shape[0], self.inference_net.num_params, cond.device, self.inference_net, int(n_samples)
        counts = None
        if target is not None and input_dict.get("summary_counts", None) is not None:
            counts = InvariantNetwork._set_counts(input_dict["summary_counts"], B, data.shape[1], dev)
        if table.shape[0] != P or data.dim() != 3 or data.shape[0] != B or data.shape[2] != 2:
            raise ValueError(f"model {model!r} has {table.shape[0]} parameters and (rt, choice) trials [B, N, 2]; the network has {P} and "
                             f"summary_conditions are {tuple(data.shape)}")
        res = {k: torch.empty(B, dtype=torch.float64, device=dev) for k in ("log_evidence", "ess", "max_share")}
        res.update({k: torch.empty(B, P, dtype=torch.float64, device=dev) for k in ("mean", "sd")})
        res.update({k: torch.empty(B, dtype=torch.int64, device=dev) for k in ("n_zero", "n_nan")})
        per = max(1, int(z_bytes) // max(1, 4 * S * P))
        scratch = torch.empty(min(per, B), S, P, dtype=torch.float32, device=dev)
        scratch_q = torch.empty(min(per, B), S, dtype=torch.float32, device=dev)
        scratch_w = None if probs is None and not smooth and resample is None else torch.empty(min(per, B), S, dtype=torch.float64, device=dev)
        kept, kept_q, kept_w, quants = [], [], [], []
        if smooth:
            scratch_s, kept_s = torch.empty(min(per, B), S, dtype=torch.float64, device=dev), []
            res_s = {k: torch.empty_like(v) for k, v in res.items()}
            res_k = {"pareto_k": torch.empty(B, dtype=torch.float64, device=dev), "n_tail": torch.empty(B, dtype=torch.int64, device=dev)}
        if resample is not None:
            words, resampled, n_unique = resample_words(B, resample_seed), [], []
        for b0 in range(0, B, per):
            c = cond[b0:b0 + per]
            nb = c.shape[0]
            z = torch.randn(nb * S, P, device=dev)
            L = net._sample_lib(z.view(nb, S, P), c) if hasattr(net, "_sample_lib") else None
            if L is not None:
                th, lq = scratch[:nb], scratch_q[:nb]
                net._fused_sample(L, z.view(nb, S, P), c, out=th, log_q=True, log_q_out=lq)
            else:
                th, lq = net.inverse_with_log_density(z, c.repeat_interleave(S, dim=0))
                th, lq = th.reshape(nb, S, P).contiguous(), lq.reshape(nb, S).contiguous()
            if target is None:
                ll = engine.wiener_log_likelihood(engine.BASIC_DDM_DC, th.view(nb * S, P), data[b0:b0 + nb], draws_per_dataset=S,
                                                  device=dev)["loglik"].view(nb, S)
            else:
                ll = engine.wiener_marginal_log_likelihood(engine.SINGLE_TRIAL, th.view(nb * S, P), data[b0:b0 + nb], draws_per_dataset=S,
                                                           t_censor=target.t_censor, device=dev,
                                                           counts=None if counts is None else counts[b0:b0 + nb])["loglik"].view(nb, S)
            out_w = {k: v[b0:b0 + nb] for k, v in res.items()}
            if scratch_w is not None:
                out_w["log_w"] = scratch_w[:nb]
            w = importance_weights(th, lq, ll, table, want_log_w=keep_weights or scratch_w is not None, out=out_w)
            log_w = w["log_w"] if keep_weights or scratch_w is not None else None
            if smooth:
                sm = pareto_smooth(log_w, out=scratch_s[:nb])
                for k, v in res_k.items():
                    v[b0:b0 + nb] = sm[k]
                log_w = sm["log_w"]
                weighted_moments(th, log_w, out={k: v[b0:b0 + nb] for k, v in res_s.items()})
                if keep_weights:
                    kept_s.append(log_w.clone())
            if probs is not None:
                quants.append(weighted_draw_quantiles(th, probs, log_w=log_w)["quantiles"])
            if resample is not None:
                rs = resample_draws(th, int(resample), log_w=log_w, words=words[b0:b0 + nb])
                resampled.append(rs["draws"])
                n_unique.append(rs["n_unique"])
            if keep_draws:
                kept.append(th.clone())
                kept_q.append(lq.clone())
            if keep_weights:
                kept_w.append(w["log_w"] if scratch_w is None else w["log_w"].clone())
        out = {("std" if k == "sd" else k): v.cpu().numpy() for k, v in res.items()}
        out["n_samples"] = S
        if target is not None:
            out["domain"] = dict(target.domain)
        if smooth:
            out["raw"] = {k: out[k] for k in ("mean", "std", "ess", "max_share", "log_evidence")}
            out.update({("std" if k == "sd" else k): res_s[k].cpu().numpy() for k in ("mean", "sd", "ess", "max_share", "log_evidence")})
            out.update({k: v.cpu().numpy() for k, v in res_k.items()}, k_threshold=pareto_k_threshold(S))
            if keep_weights:
                out["log_w_smoothed"] = torch.cat(kept_s, dim=0).cpu().numpy()
        if probs is not None:
            q = torch.cat(quants, dim=0).cpu().numpy()
            for k, pk in enumerate(probs):
                name = self.SUMMARY_NAMES.get(float(pk))
                if name is not None:
                    out[name] = q[:, k, :]
            out.update(quantiles=q, probs=probs)
        if resample is not None:
            rs = resampled[0] if len(resampled) == 1 else torch.cat(resampled, dim=0)
            out.update(resampled=rs if _resampled_on_device else rs.cpu().numpy(), n_unique=torch.cat(n_unique, dim=0).cpu().numpy(),
                       resample_seed=int(resample_seed))
        if keep_draws:
            out["draws"], out["log_q"] = torch.cat(kept, dim=0).cpu().numpy(), torch.cat(kept_q, dim=0).cpu().numpy()
        if keep_weights:
            out["log_w"] = torch.cat(kept_w, dim=0).cpu().numpy()
        return out

    @torch.no_grad()
    def sample_exact(self, input_dict, n_samples, n_proposals=None, smooth=True, seed=0, to_numpy=True, target=None):
        """Draws of the EXACT posterior of every data set: [n_samples, P] for a single data set, [B, n_samples, P] for a batch, as
        `sample` -- n_proposals (default: n_samples) draws of the flow, importance-weighted against the exact Wiener likelihood and
        resampled into n_samples equally weighted ones (posterior_importance(..., resample=n_samples, resample_seed=seed); smooth:
        on the Pareto-smoothed weights).  For joint plots, correlations, posterior-predictive simulation, starting points of fit_hmc.
        Whether to believe them is in `self.last_exact`: "ess" and "n_unique" [B] (how many of the proposals carry the weight, and how
        many different rows came back), and with smooth "pareto_k" [B] against "k_threshold" (else None).  model="basic", as
        posterior_importance; a ragged batch (`observed_batch`) needs nothing more.  target: None, or a single_trial_target(...) --
        the single-trial model's posterior under its restricted prior (posterior_importance's `target`)."""
        S = int(n_samples if n_proposals is None else n_proposals)
        r = self.posterior_importance(input_dict, S, smooth=smooth, resample=int(n_samples), resample_seed=seed,
                                      _resampled_on_device=not to_numpy, target=target)
        self.last_exact = {"ess": r["ess"], "n_unique": r["n_unique"], "pareto_k": r.get("pareto_k"), "k_threshold": r.get("k_threshold"),
                           "n_proposals": S}
        out = r["resampled"]
        if out.shape[0] == 1:
            out = out[0]
        return out

    @torch.no_grad()
    def log_posterior(self, input_dict, to_numpy=True):
        """bf.amortizers.AmortizedPosterior.log_posterior: log q(parameters | conditions) through the flow's FORWARD, z, log|det| =
        inference_net(parameters, conditions) -> -|z|^2 / 2 - (P / 2) log 2 pi + log|det|.  input_dict["parameters"]: [B, P], a row
        per data set -> [B]; or [B, S, P], S rows per data set (posterior draws: the condition row is repeated) -> [B, S].  The
        independent route to the number the fused sampler emits with its draws (inverse_per_set(log_density=True))."""
        theta, cond = self._t(input_dict["parameters"]), self._conditions(input_dict)
        shape = theta.shape[:-1]
        if theta.dim() == 3:
            if theta.shape[0] != cond.shape[0]:
                raise ValueError(f"parameters hold {theta.shape[0]} data sets but the conditions {cond.shape[0]}")
            cond = cond.repeat_interleave(theta.shape[1], dim=0)
            theta = theta.reshape(-1, theta.shape[-1])
        z, log_det = self.inference_net(theta.contiguous(), cond)
        lq = (-0.5 * (z ** 2).sum(-1) - 0.5 * theta.shape[-1] * math.log(2.0 * math.pi) + log_det).reshape(shape)
        return lq.cpu().numpy() if to_numpy else lq


class Trainer:
    """bf.trainers.Trainer(amortizer, generative_model, configurator, checkpoint_path): online and experience-replay
    training (basic_ddm_dc.py:172-176, 199-202), `load_pretrained_network` (:207).  Checkpoints also carry the
    simulator's (seed, offset) stream state, so a resumed run continues the random stream."""

    def __init__(self, amortizer, generative_model, configurator=None, checkpoint_path=None, learning_rate=5e-4,
                 device=None, stream_state=None, graph=False):
        """graph=True: train_online / train_experience_replay keep the reference's call shape (basic_ddm_dc.py:199-202) and
        run as hipGraph replays (graph_trainer.GraphTrainer: device prior -> simulate -> forward/backward -> clip -> Adam, one
        batch ahead) when the generative model says how it is made (`graph_spec`, set by the model modules'
        make_generative_model): ~25 x the eager loop at batch 32.  The batches then come from the library's on-device prior
        and simulator keyed by `graph_spec['seed']` -- the same distributions, another random stream than the generative
        model's own -- and a ValueError says so if the model cannot be run that way."""
        self.graph = bool(graph)
        self.amortizer, self.generative_model = amortizer, generative_model
        self.configurator = configurator or (lambda d: d)
        self.checkpoint_path = checkpoint_path
        self.device = torch.device(device) if device is not None else (
            torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu"))
        self.amortizer.to(self.device)
        self.lr = learning_rate
        self.optimizer = torch.optim.Adam(self.amortizer.parameters(), lr=learning_rate)
        self.scheduler = None
        self._optimizer_spent = False      # set when a train_* call ends with reuse_optimizer=False (BayesFlow's default)
        self.stream_state = stream_state
        self.loss_history = []
        self.replay = []
        self._graph_pos = None             # graph=True: where the last train_* call left the random stream and the replay buffer
        self._graph_opt = None             # graph=True: the running call's optimizer / schedule state at its last epoch checkpoint
        self._graph_resume = None          # ... as load_pretrained_network found it in ckpt.pt: an interrupted call is continued

    def _simulate(self, batch_size):
        return self.configurator(self.generative_model(batch_size))

    def _step(self, conf):
        loss = self.amortizer.compute_loss(conf)
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(self.amortizer.parameters(), 5.0)
        self.optimizer.step()
        if self.scheduler is not None:
            self.scheduler.step()
        return float(loss.detach())

    def _setup_schedule(self, total_steps, optimizer=None, scheduler=None):
        """`optimizer` given (BayesFlow's train_*(optimizer=...)): the caller's optimizer -- and learning-rate scheduler, if
        any -- is used as it is; nothing is reset (one schedule can then span several calls).  Otherwise:
        every train_* call is a run of its own, as in BayesFlow 1.1's Trainer: a cosine decay from the Trainer's learning
        rate over THIS call's epochs x iterations (held at its final value beyond, like Keras' CosineDecay) and -- unless the
        previous call was made with reuse_optimizer=True, or a checkpoint has just been loaded -- a fresh Adam.  (Stacking a
        second CosineAnnealingLR on an optimizer whose rate the first one had annealed to 0 trained the second call, and every
        resumed run, at rate 0.)"""
        if optimizer is not None:
            self.optimizer, self.scheduler, self._optimizer_spent = optimizer, scheduler, False
            return
        if self._optimizer_spent:
            self.optimizer = torch.optim.Adam(self.amortizer.parameters(), lr=self.lr)
            self._optimizer_spent = False
        for g in self.optimizer.param_groups:
            g["lr"] = self.lr
            g["initial_lr"] = self.lr
        total = max(1, int(total_steps))
        self.scheduler = torch.optim.lr_scheduler.LambdaLR(
            self.optimizer, lambda step: 0.5 * (1.0 + math.cos(math.pi * min(step, total) / total)))

    def _prefetcher(self, batch_size, total, prefetch=True):
        """Yields `total` configured batches, simulating batch i+1 on a side stream BEFORE batch i is trained on: the
        simulator launch (and a host-side prior) then overlaps the training step, whose loss read-back is the only
        synchronisation point of an iteration.  Batches come in the same order from the same random stream as without
        prefetching (prefetch=False, or no device: one after the other); nothing is simulated beyond `total`."""
        if not prefetch or self.device.type != "cuda" or total <= 0:
            for _ in range(total):
                yield self._simulate(batch_size)
            return
        side = torch.cuda.Stream(device=self.device)

        def launch():
            with torch.cuda.stream(side):
                conf = self._simulate(batch_size)
                ev = torch.cuda.Event()
                ev.record(side)
            return conf, ev

        nxt = launch()
        for i in range(total):
            conf, ev = nxt
            main = torch.cuda.current_stream(self.device)
            main.wait_event(ev)
            for v in conf.values():          # the tensors were allocated on the side stream's pool
                if torch.is_tensor(v) and v.is_cuda:
                    v.record_stream(main)
            if i + 1 < total:
                nxt = launch()
            yield conf

    def _graph_loop(self, replay, epochs, iterations_per_epoch, batch_size, capacity_in_batches, validation_sims, save_checkpoint,
                    optimizer):
        """The call as graph replays: one GraphTrainer for THIS call (its cosine schedule spans epochs x iterations, a fresh Adam:
        _setup_schedule's semantics), an epoch = one train_* call of it, validation loss and checkpoint between epochs.

        The run's POSITION outlives the call (`self._graph_pos`, also in ckpt.pt): the next call -- and a run resumed through
        load_pretrained_network -- continues the random stream (next parameter sets, next batch-shared N) and the experience-replay
        buffer where this one stopped, as the eager loop does through `stream_state` and `self.replay`.  Training's parameter
        sets start at graph_trainer.TRAIN_OFFSET_BASE of the seed's index space; the generative model's own draws (validation
        sims, recovery data sets) count up from 0, so the two never meet."""
        spec = getattr(self.generative_model, "graph_spec", None)
        if spec is None or self.device.type != "cuda" or optimizer is not None:
            raise ValueError("Trainer(graph=True) needs a generative model made by a model module's make_generative_model "
                             "(it carries `graph_spec`), a ROCm device, and no caller-supplied optimizer")
        from .graph_trainer import TRAIN_OFFSET_BASE, GraphTrainer
        val = []
        total = epochs * iterations_per_epoch
        resume, self._graph_resume = self._graph_resume, None
        with GraphTrainer(self.amortizer, batch_size=batch_size, total_steps=total, learning_rate=self.lr,
                          device=self.device, offset_base=TRAIN_OFFSET_BASE, **spec) as gt:
            done_epochs = 0
            if (resume is not None and int(resume["total_steps"]) == total and int(resume["iterations_per_epoch"]) == iterations_per_epoch
                    and int(resume["batch_size"]) == batch_size and bool(resume["replay"]) == bool(replay) and 0 < int(resume["iteration"]) < total):
                # The checkpoint was written BETWEEN TWO EPOCHS of a call of this very shape: that call is continued -- Adam's moments
                # and step count, the place on the cosine schedule, the losses so far -- and only its remaining epochs run, so an
                # interrupted run + its resumption equal the uninterrupted run.  (Any other call after a load is a run of its own,
                # as every train_* call is: fresh Adam, its own schedule.)
                gt.load_optimizer_state(resume)
                done_epochs = int(resume["iteration"]) // iterations_per_epoch
                self.loss_history = self.loss_history[:max(0, len(self.loss_history) - int(resume["iteration"]))]      # (gt brings them back)
            if self._graph_pos is not None:
                gt.set_position(self._graph_pos)
            for _ in range(done_epochs, epochs):
                if replay:
                    gt.train_experience_replay(iterations_per_epoch, capacity_in_batches=capacity_in_batches)
                else:
                    gt.train_online(iterations_per_epoch)
                if validation_sims is not None:
                    val.append(gt.validation_loss(self.configurator(validation_sims)))
                if save_checkpoint and self.checkpoint_path:
                    self._graph_pos = gt.position()
                    self._graph_opt = dict(gt.optimizer_state(), iterations_per_epoch=int(iterations_per_epoch), batch_size=int(batch_size),
                                           replay=bool(replay))
                    self.loss_history_graph = gt.loss_history()
                    self.save_checkpoint(extra_losses=self.loss_history_graph)
            self._graph_pos = gt.position()
            self._graph_opt = None             # the call is complete: nothing to continue
            self.loss_history += gt.loss_history()
        if save_checkpoint and self.checkpoint_path:
            self.save_checkpoint()             # ... and the checkpoint says so (a later load starts a run of its own)
        self._optimizer_spent = True
        return val

    def _eager_loop(self, train_on, epochs, iterations_per_epoch, batch_size, validation_sims, save_checkpoint, prefetch,
                    reuse_optimizer, optimizer, scheduler):
        """The call as eager steps: this call's schedule, per epoch `iterations_per_epoch` steps -- each on train_on(fresh batch) --
        then the validation loss (returned, one per epoch) and the checkpoint."""
        self._setup_schedule(epochs * iterations_per_epoch, optimizer, scheduler)
        val = []
        for _ in range(epochs):
            for conf in self._prefetcher(batch_size, iterations_per_epoch, prefetch):
                self.loss_history.append(self._step(train_on(conf)))
            if validation_sims is not None:
                with torch.no_grad():
                    val.append(float(self.amortizer.compute_loss(self.configurator(validation_sims))))
            if save_checkpoint:
                self.save_checkpoint()
        self._optimizer_spent = not (reuse_optimizer or optimizer is not None)
        return val

    def train_online(self, epochs, iterations_per_epoch, batch_size, save_checkpoint=True, prefetch=True, reuse_optimizer=False,
                     optimizer=None, scheduler=None, **_):
        if self.graph:
            self._graph_loop(False, epochs, iterations_per_epoch, batch_size, 0, None, save_checkpoint, optimizer)
        else:
            self._eager_loop(lambda conf: conf, epochs, iterations_per_epoch, batch_size, None, save_checkpoint, prefetch,
                             reuse_optimizer, optimizer, scheduler)
        return self.loss_history

    def train_experience_replay(self, epochs, iterations_per_epoch, batch_size, capacity_in_batches=100,
                                save_checkpoint=True, validation_sims=None, prefetch=True, reuse_optimizer=False,
                                optimizer=None, scheduler=None, **_):
        """Each iteration simulates one fresh batch into a ring buffer of `capacity_in_batches` batches and trains on
        a randomly chosen stored batch (BayesFlow's experience replay, used at basic_ddm_dc.py:199-202).  Batches keep
        their own N (the non-batchable context), as in BayesFlow's buffer."""
        if self.graph:
            val = self._graph_loop(True, epochs, iterations_per_epoch, batch_size, capacity_in_batches, validation_sims, save_checkpoint,
                                   optimizer)
            return {"train_losses": self.loss_history, "val_losses": val}
        rng = np.random.default_rng(0)

        def stored(conf):
            if len(self.replay) < capacity_in_batches:
                self.replay.append(conf)
            else:
                self.replay[rng.integers(capacity_in_batches)] = conf
            return self.replay[rng.integers(len(self.replay))]

        val = self._eager_loop(stored, epochs, iterations_per_epoch, batch_size, validation_sims, save_checkpoint, prefetch,
                               reuse_optimizer, optimizer, scheduler)
        return {"train_losses": self.loss_history, "val_losses": val}

    # ---- checkpoint / resume -----------------------------------------------------------------------
    def save_checkpoint(self, extra_losses=()):
        if not self.checkpoint_path:
            return
        os.makedirs(self.checkpoint_path, exist_ok=True)
        state = {"model": self.amortizer.state_dict(), "optimizer": self.optimizer.state_dict(),
                 "loss_history": self.loss_history + list(extra_losses)}
        if self.stream_state is not None:
            state["stream_state"] = self.stream_state.get_state()
        if self._graph_pos is not None:
            state["graph_position"] = self._graph_pos
        if self._graph_opt is not None:        # graph=True, written between two epochs of a call: what continues that call
            state["graph_optimizer"] = self._graph_opt
        from .graph_trainer import plain_state
        torch.save(plain_state(state), os.path.join(self.checkpoint_path, "ckpt.pt"))      # plain data only: loads with weights_only=True
        with open(os.path.join(self.checkpoint_path, "history.pkl"), "wb") as f:
            pickle.dump({"loss_history": state["loss_history"]}, f)

    def load_pretrained_network(self):
        path = os.path.join(self.checkpoint_path or "", "ckpt.pt")
        if not os.path.exists(path):
            return False
        state = torch.load(path, map_location=self.device, weights_only=True)        # (plain_state(): tensors, numbers, strings -- no pickle code)
        self.amortizer.load_state_dict(state["model"])
        self.optimizer.load_state_dict(state["optimizer"])
        self._optimizer_spent = False      # the loaded moments serve the next train_* call (which sets its own schedule)
        self.loss_history = list(state.get("loss_history", []))
        if self.stream_state is not None and "stream_state" in state:
            self.stream_state.set_state(state["stream_state"])
        self._graph_pos = state.get("graph_position", self._graph_pos)      # graph=True: the next call continues the stream
        self._graph_resume = state.get("graph_optimizer", None)             # ... and, if the file was written mid-call, that call
        return True


def posterior_estimates(amortizer, generative_model, configurator, n_datasets=100, n_samples=1000, fused=False):
    """n_datasets fresh data sets, one at a time as in the reference's loop (basic_ddm_dc.py:218-223): (true parameters [n, P],
    posterior means [n, P], posterior medians [n, P]) from n_samples posterior draws each.  fused: `AmortizedPosterior.sample`'s."""
    true, means, meds = [], [], []
    for _ in range(n_datasets):
        conf = configurator(generative_model(1))
        post = amortizer.sample(conf, n_samples, fused=fused)
        p = conf["parameters"]
        true.append((p.cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p))[0])
        means.append(post.mean(axis=0))
        meds.append(np.median(post, axis=0))
    return np.array(true), np.array(means), np.array(meds)


def posterior_recovery(amortizer, generative_model, configurator, n_datasets=100, n_samples=1000, statistic="mean", fused=False):
    """The recovery loop of basic_ddm_dc.py:218-223 in miniature: posterior means vs true parameters -> per-parameter
    Pearson correlation (the reference plots R^2 / rho, pyhddmjagsutils.py:609-623).  statistic="median": the posterior median
    instead.  A sharply trained flow carries ~5e-7 of its mass at |theta| up to 1e6 (regions maximum-likelihood training never
    visits: once the inverse's intermediate vector leaves the trained range, the conditioners' log-scales flip sign and every
    remaining half-layer multiplies by e^1.9; the inverse is exact there -- DESIGN.md section 8, tools/locate_tail_draws.py), and ONE
    such draw among a data set's ten thousand moves its mean (and one such data set among hundreds the correlation) while the
    posterior's bulk sits on the truth.  The mean is the reference's statistic and the default here.  fused: `AmortizedPosterior.
    sample`'s (`AmortizedPosterior.posterior_moments` with a box is the tail-safe mean without the draws)."""
    if statistic not in ("mean", "median"):
        raise ValueError("statistic must be 'mean' or 'median'")
    true, means, meds = posterior_estimates(amortizer, generative_model, configurator, n_datasets, n_samples, fused=fused)
    est = means if statistic == "mean" else meds
    return np.array([np.corrcoef(true[:, j], est[:, j])[0, 1] for j in range(true.shape[1])])
