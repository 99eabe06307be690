"""GPU tests of the summary network's inference kernels (csrc/train_deepset.hip: nddm_deepset_summary; InvariantNetwork.summarize):
the whole network with a trial count per set, in blocks + 2 launches that keep nothing for a backward -- and of the ragged batch
(`observed_batch`, the dict key `summary_counts`) through AmortizedPosterior's posterior calls."""
import copy
import ctypes
import itertools

import numpy as np
import pytest

from train_yardstick import _F64Yardstick

pytestmark = pytest.mark.gpu

CYCLE = (1, 63, 64, 65, 128, 129)
# (blocks, B, N, counts): counts at, one below and one above the 64-row tile; a set of one trial; tiles wholly beyond a set's count; 70
# sets, so that the MLP after the pooling spans two row tiles whose rows each take their own 1 / n; N = 1
BATTERIES = [(2, 5, 131, (131, 64, 65, 1, 100)), (2, 70, 129, tuple(itertools.islice(itertools.cycle(CYCLE), 70))), (0, 3, 200, (77, 200, 128)),
             (1, 2, 1, (1, 1))]
CASES = [(bt, d_in) for bt in BATTERIES for d_in in (2, 3)]
_cache = {}


def _case(battery, d_in):
    """(network, its float64 copy, trials [B, N, d_in], the three direct-condition forms), made once per case and left unchanged"""
    import torch
    key = (battery, d_in)
    if key not in _cache:
        blocks, B, N, _ = battery
        torch.manual_seed(5 + 10 * blocks + d_in)
        net = _net(blocks, d_in)
        cols = [0.3 + torch.rand(B, N, device="cuda") * 2.0, (torch.rand(B, N, device="cuda") < 0.7).float()] + [torch.randn(B, N, device="cuda")] * (d_in - 2)
        directs = (None, torch.log(torch.tensor(battery[3], device="cuda", dtype=torch.float32)).view(B, 1), torch.randn(B, 3, device="cuda"))
        _cache[key] = (net, copy.deepcopy(net).double(), torch.stack(cols, dim=-1), directs)
    return _cache[key]


def _net(blocks, d_in=2, **kw):
    import torch
    from bayesflow_nddms_amd.amortizer import InvariantNetwork
    net = InvariantNetwork(input_dim=d_in, num_equiv=blocks, **kw).cuda()
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.copy_(0.1 * torch.randn_like(p))                  # non-zero biases
    return net


def _poison(x, counts):
    x = x.clone()
    for b, c in enumerate(counts):
        x[b, c:] = float("nan")
    return x


def test_the_library_has_the_entry_and_summarize_takes_it():
    import torch
    from bayesflow_nddms_amd import _train_lib
    L = _train_lib.lib()
    assert L is not None, "libnddm_train.so did not build / load"
    assert L.nddm_deepset_summary_work_bytes(5, 131, 2) == 4 * 64 * (3 * 5 * 3 + 5 * 131) and L.nddm_deepset_summary_work_bytes(5, 131, 0) == 4 * 64 * 15
    assert L.nddm_deepset_summary_work_bytes(0, 131, 2) == -1
    net, _, x, _ = _case(BATTERIES[0], 2)
    with torch.no_grad():
        assert net._summary_lib(x, None) is L and net._fused_lib(x) is None          # (its own gate: the training path still refuses no_grad)


def test_accuracy_against_float64():
    """The kernels' summary against the same network in float64 under the definition forward(x, counts=...), PyTorch's float32
    composition of that definition as the measure (_F64Yardstick, its default bounds), over every battery, d_in 2 and 3, with and
    without direct conditions.  Measured on the MI355X: pooled rms error kernels / pytorch 0.864."""
    import torch
    yard = _F64Yardstick()
    for battery, d_in in CASES:
        net, net64, x, directs = _case(battery, d_in)
        counts, sd = battery[3], net.summary_dim
        for direct in directs:
            with torch.no_grad():
                got = net.summarize(x, counts, direct)
                plain = net(x, counts=counts, direct=direct)
                exact = net64(x.double(), counts=counts, direct=None if direct is None else direct.double())
            k = 0 if direct is None else direct.shape[1]
            assert got.shape == (battery[1], sd + k) and got.dtype == torch.float32 and torch.isfinite(got).all()
            if direct is not None:
                assert torch.equal(got[:, sd:], direct)
            yard.add("summary", (battery[:3], d_in, k), [got[:, :sd]], [plain[:, :sd]], [exact[:, :sd]], ["summary"])
    print("ragged summary, pooled rms error kernels / pytorch-f32 against f64:", yard.finish())


@pytest.mark.parametrize("battery,d_in", CASES)
def test_ragged_equals_alone_bit_for_bit_and_never_reads_the_padding(battery, d_in):
    """Row b of the ragged call is, bit for bit (+ 0.0: a zero's sign does not count), summarize on x[b:b+1, :counts[b]] alone: the same
    tiles, and the tiles beyond a set's count contribute exact zeros.  NaN in every row at or beyond a set's count changes no bit."""
    import torch
    net, _, x, directs = _case(battery, d_in)
    counts = battery[3]
    for direct in directs:
        got = net.summarize(x, counts, direct)
        assert torch.equal(net.summarize(_poison(x, counts), torch.tensor(counts, device="cuda"), direct), got)
        alone = torch.cat([net.summarize(x[b:b + 1, :c].contiguous(), None, None if direct is None else direct[b:b + 1]) for b, c in enumerate(counts)])
        assert torch.equal(got + 0.0, alone + 0.0)


@pytest.mark.parametrize("battery,d_in", [c for c in CASES if c[0][2] > 1])
def test_equal_counts_equal_the_training_forward_bit_for_bit(battery, d_in):
    """counts = [n] * B against InvariantNetwork.forward(x, n_valid=n) with gradients enabled -- the training kernels, whose steps
    these kernels are made of -- at n = N and n < N, with and without direct conditions; and no counts at all is n = N."""
    import torch
    net, _, x, directs = _case(battery, d_in)
    B, N = battery[1], battery[2]
    for n in (N, 100 if N > 100 else N - 1, 64):
        for direct in directs:
            assert net._fused_lib(x) is not None
            want = net(x, n_valid=torch.tensor([float(n)], device="cuda"), direct=direct).detach()
            assert torch.equal(net.summarize(x, [n] * B, direct), want)
            if n == N:
                assert torch.equal(net.summarize(x, None, direct), want)


def _entry(L, net, x, counts, direct, out, work, work_bytes):
    import torch
    params = net.fused_params()
    ptrs = (ctypes.c_void_p * len(params))(*[p.data_ptr() for p in params])
    B, N, d = x.shape
    return L.nddm_deepset_summary(x.data_ptr(), d, B, N, None if counts is None else counts.data_ptr(), len(net.equiv), ptrs, net.summary_dim,
                                  None if direct is None else direct.data_ptr(), 0 if direct is None else direct.shape[1],
                                  0 if direct is None else direct.stride(0), out.data_ptr(), work.data_ptr(), work_bytes,
                                  torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("battery", BATTERIES[:3])
def test_stores_are_confined_and_a_count_of_zero_spoils_its_own_row_only(battery):
    """The C entry on an output and a work buffer that each lie between guard bands of a sentinel: the bands are untouched and the
    output is summarize's.  Then one set's count is 0 (a device tensor is not checked): its row is non-finite, every other row keeps
    its bits, the bands stay untouched.  Bad arguments are refused before any launch."""
    import torch
    from bayesflow_nddms_amd import _train_lib
    L = _train_lib.lib()
    net, _, x, directs = _case(battery, 2)
    (blocks, B, N, counts), direct, G, sentinel = battery, directs[2], 4096, 12345.678
    width = net.summary_dim + 3
    nbytes = L.nddm_deepset_summary_work_bytes(B, N, blocks)
    o_buf = torch.full((2 * G + B * width,), sentinel, device="cuda")
    w_buf = torch.full((2 * G + nbytes // 4,), sentinel, device="cuda")
    out, work = o_buf[G:G + B * width].view(B, width), w_buf[G:G + nbytes // 4]

    def bands_untouched():
        return all(bool((t == t.new_tensor(sentinel)).all()) for t in (o_buf[:G], o_buf[-G:], w_buf[:G], w_buf[-G:]))

    cnt = torch.tensor(counts, device="cuda", dtype=torch.int32)
    assert _entry(L, net, x, cnt, direct, out, work, nbytes) == 0
    want = net.summarize(x, counts, direct)
    assert torch.equal(out, want) and bands_untouched()
    cnt0 = cnt.clone()
    cnt0[1] = 0
    out.fill_(sentinel)
    assert _entry(L, net, x, cnt0, direct, out, work, nbytes) == 0
    keep = torch.arange(B, device="cuda") != 1
    assert not torch.isfinite(out[1, :net.summary_dim]).any() and torch.equal(out[keep], want[keep]) and bands_untouched()
    # a count beyond N is clamped for addressing: the set is summarised over its N rows
    cnt_big = cnt.clone()
    cnt_big[0] = N + 1000
    assert _entry(L, net, x, cnt_big, direct, out, work, nbytes) == 0
    full = net.summarize(x, [N] + list(counts[1:]), direct)
    assert torch.equal(out, full) and bands_untouched()
    # refused: a work buffer too small or misaligned, a summary wider than 64 columns with the direct ones, d_in 5
    assert _entry(L, net, x, cnt, direct, out, work, nbytes - 4) == 1 and _entry(L, net, x, cnt, direct, out, w_buf[G + 1:], nbytes) == 1
    wide = torch.zeros(B, 60, device="cuda")
    assert _entry(L, net, x, cnt, wide, out, work, nbytes) == 1
    assert _entry(L, net, torch.zeros(B, N, 5, device="cuda"), cnt, direct, out, work, nbytes) == 1
    assert bands_untouched()


def test_fallbacks_take_the_definition():
    """hidden width 32, d_in 5 and float64 are not the kernels': summarize takes forward(x, counts=...), and agrees with each set alone."""
    import torch
    counts = (131, 64, 65, 1, 100)
    torch.manual_seed(9)
    for net, x in ((_net(2, hidden=32), torch.randn(5, 131, 2, device="cuda")), (_net(2, d_in=5), torch.randn(5, 131, 5, device="cuda")),
                   (_net(2).double(), torch.randn(5, 131, 2, device="cuda", dtype=torch.float64))):
        direct = torch.randn(5, 1, device="cuda", dtype=x.dtype)
        with torch.no_grad():
            assert net._summary_lib(x, direct) is None
            got = net.summarize(_poison(x, counts), counts, direct)
            assert torch.equal(got, net(x, counts=counts, direct=direct))
            alone = torch.cat([torch.cat([net(x[b:b + 1, :c]), direct[b:b + 1]], dim=-1) for b, c in enumerate(counts)])
        assert got.dtype == x.dtype and torch.allclose(got, alone, rtol=1e-4, atol=1e-5)
    net = _net(2)
    net.fused = False
    assert net._summary_lib(torch.randn(5, 131, 2, device="cuda"), None) is None


def _participants():
    """4 basic_ddm_dc data sets of 60, 64, 131 and 300 trials, an amortizer centred on the prior, the ragged dict"""
    import torch
    from bayesflow_nddms_amd import basic_ddm_dc
    from bayesflow_nddms_amd.amortizer import AmortizedPosterior, InvariantNetwork, InvertibleNetwork, observed_batch
    if "people" not in _cache:
        torch.manual_seed(0)
        rng = np.random.default_rng(2023)
        n = (60, 64, 131, 300)
        theta = np.stack([rng.normal(0.5, 1.0, 4), rng.uniform(0.9, 1.6, 4), rng.uniform(0.4, 0.6, 4), rng.uniform(0.2, 0.4, 4), rng.uniform(0.8, 1.2, 4)],
                         axis=1).astype(np.float32)
        sim = basic_ddm_dc.batch_simulate_trials(theta, 300, seed=2023, set_offset=0, with_summary=False)["sim_data"]
        sets = [np.asarray(sim[b, :k], dtype=np.float32) for b, k in enumerate(n)]
        am = AmortizedPosterior(InvertibleNetwork(num_params=5), InvariantNetwork()).cuda().eval()
        with torch.no_grad():                                 # an untrained flow, but centred on the prior: most draws inside its support
            width = torch.tensor([1.0, 0.3, 0.15, 0.1, 0.3], device="cuda")
            am.inference_net.an_scale[0].copy_(-torch.log(width))
            am.inference_net.an_bias[0].copy_(-torch.tensor([0.0, 1.0, 0.5, 0.15, 1.0], device="cuda") / width)
        _cache["people"] = (sets, am, observed_batch(sets, device="cuda"))
    return _cache["people"]


def test_end_to_end_one_call_for_participants_of_different_trial_counts():
    """sample(observed_batch(...), S, fused=True): set b's draws against the fused sampler on set b ALONE -- its own observed_batch,
    its slice of the same base normals -- at the bound of "padding is invisible" (rtol 1e-4, atol 1e-5; the conditions are equal
    bit for bit); posterior_moments, posterior_summary and log_posterior take the same dict."""
    import torch
    from bayesflow_nddms_amd.amortizer import observed_batch
    sets, am, ob = _participants()
    B, S, P = len(sets), 200, 5
    assert ob["summary_conditions"].shape == (4, 300, 2) and ob["summary_counts"].tolist() == [60, 64, 131, 300]
    torch.manual_seed(4)
    got = am.sample(ob, S, fused=True, to_numpy=False)
    torch.manual_seed(4)
    z = torch.randn(B * S, P, device="cuda").view(B, S, P)
    with torch.no_grad():
        cond = am._conditions(ob)
        for b, s in enumerate(sets):
            cond_b = am._conditions(observed_batch([s], device="cuda"))
            assert torch.equal(cond_b + 0.0, cond[b:b + 1] + 0.0)
            alone = am.inference_net.inverse_per_set(z[b:b + 1].contiguous(), cond_b)[0]
            assert torch.allclose(got[b], alone, rtol=1e-4, atol=1e-5)
            if b < 3:                                          # (the padding matters: the set summarised over all 300 rows is another condition)
                padded = am._conditions({k: v[b:b + 1] for k, v in ob.items() if k != "summary_counts"})
                assert not torch.allclose(padded, cond_b, rtol=1e-4, atol=1e-5)
    assert got.shape == (B, S, P) and torch.isfinite(got).all()
    m = am.posterior_moments(ob, S)
    q = am.posterior_summary(ob, S)
    assert all(np.isfinite(m[k]).all() and m[k].shape == (B, P) for k in ("mean", "sd"))
    assert all(np.isfinite(q[k]).all() and q[k].shape == (B, P) for k in ("mean", "std", "median", "95lower", "95upper"))
    lp = am.log_posterior(dict(ob, parameters=got), to_numpy=False)
    assert lp.shape == (B, S) and torch.isfinite(lp).all()


def test_the_likelihood_scores_zero_padding_as_nothing_so_importance_weights_need_no_counts():
    """engine.wiener_log_likelihood(BASIC_DDM_DC, ...) on the zero-padded sets equals the call on each unpadded set (float64 sums; rtol
    1e-12, a reordering of <= 300 terms being worth n 2^-53 of their magnitudes): a padding row (rt 0, choice 0) is a timeout censored
    at t = -tau <= 0, log 1 = 0.  Hence posterior_importance on the ragged dict is finite and gives every set what importance_weights
    gives for the same draws scored against the set's own trials."""
    import torch
    from bayesflow_nddms_amd import engine
    from bayesflow_nddms_amd.amortizer import importance_weights
    sets, am, ob = _participants()
    B, S, P = len(sets), 150, 5
    torch.manual_seed(6)
    r = am.posterior_importance(ob, S, keep_draws=True, keep_weights=True)
    assert np.isfinite(r["ess"]).all() and np.isfinite(r["log_evidence"]).all() and (r["ess"] >= 1.0).all()
    draws, log_q = torch.as_tensor(r["draws"], device="cuda"), torch.as_tensor(r["log_q"], device="cuda")
    ll_pad = engine.wiener_log_likelihood(engine.BASIC_DDM_DC, draws.view(B * S, P), ob["summary_conditions"], draws_per_dataset=S,
                                          device="cuda")["loglik"].view(B, S)
    for b, s in enumerate(sets):
        ll = engine.wiener_log_likelihood(engine.BASIC_DDM_DC, draws[b].contiguous(), torch.as_tensor(s, device="cuda")[None], draws_per_dataset=S,
                                          device="cuda")["loglik"]
        fin = torch.isfinite(ll)
        assert int(fin.sum()) > 0 and torch.equal(fin, torch.isfinite(ll_pad[b])) and torch.equal(torch.isnan(ll), torch.isnan(ll_pad[b]))
        assert torch.allclose(ll_pad[b][fin], ll[fin], rtol=1e-12, atol=0.0)
        assert torch.equal(ll_pad[b][fin], ll[fin])           # (to the last bit, in fact: the padding's terms are +0.0 at the end of each lane's sum)
        w = importance_weights(draws[b:b + 1].contiguous(), log_q[b:b + 1].contiguous(), ll.view(1, S), "basic")
        for k in ("ess", "log_evidence"):
            assert np.allclose(w[k].cpu().numpy()[0], r[k][b], rtol=1e-9, atol=1e-9), (k, b)       # (|d loglik| <= 1e-12 |loglik|, a few 1e-10 on the weights)
        assert int(w["n_nan"][0]) == r["n_nan"][b] and int(w["n_zero"][0]) == r["n_zero"][b]
    print(f"ragged posterior_importance: ess {r['ess']}, log evidence {r['log_evidence']}")
