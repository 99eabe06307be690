"""Sampling-importance-resampling on the device (csrc/train_resample.hip: one workgroup per set scans the integer weights in LDS in row
order and searches them per output; amortizer.py: resample_draws, posterior_importance(resample=...), sample_exact): held to the
definition as tests/resample_ref.py recomputes it in Python integers -- every ancestor, bit for bit, on the kernel's own integer
weights -- at the smallest shapes a scan and a search go wrong at, to the PyTorch evaluation on the same device tensors, to its
outputs' bounds, to independence of neighbours, through the public call, and end to end against an independent float64 posterior."""
import numpy as np
import pytest

from flow_importance_ref import GOLDEN, PROPOSAL_DRAWS, PROPOSAL_SEED, mean_bound, proposal_flow
from resample_ref import bits, check, crafted_cases, effective, properties, quantize, skewed_log_w
from test_flow_resample_cpu import MAXW, check_word_case, out_counts, word_cases
from test_flow_wquantile_cpu import OLD_KEYS
from test_gpu_flow_wquantile import _people, _same_bits

pytestmark = pytest.mark.gpu

KEYS = ("draws", "ancestors", "n_unique", "n_positive")


def _lib():
    from bayesflow_nddms_amd import _train_lib
    L = _train_lib.lib()
    assert L is not None, "libnddm_train.so did not build / load"
    return L


def _cap():
    return _lib().nddm_train_resample_max_draws()


def _same(a, b, keys=KEYS):
    return all(_same_bits(a[k], b[k]) for k in keys)


def _fallback(theta, M, **kw):
    """resample_draws with the kernel gated off: the PyTorch evaluation, on the same (device) tensors."""
    from bayesflow_nddms_amd import amortizer
    gate = amortizer._resample_lib
    amortizer._resample_lib = lambda *a: None
    try:
        return amortizer.resample_draws(theta, M, **kw)
    finally:
        amortizer._resample_lib = gate


@pytest.mark.parametrize("B,S,D", [(1, 1, 5), (2, 2, 1), (3, 63, 5), (2, 64, 8), (1, 65, 1), (2, 257, 5), (2, 1025, 8), (1, 4097, 1), (1, 10000, 5),
                                   (1, "cap", 1), (1, "cap + 1", 5)], ids=lambda v: str(v))
def test_exact_ancestors(B, S, D):
    """One draw, either side of a wave, S either side of the instantiations' sizes (... 257 take the 1024-item kernel, 1025 the 4096,
    4097, 10 000 -- the reference's -- and the cap the 16 384); cap + 1 takes the PyTorch evaluation and must give the same definition.
    M on both sides of a wave and of S.  The kernel equals the reference evaluated on its OWN returned integer weights, bit for bit;
    those are within 1 of NumPy's; and given those weights the kernel equals the PyTorch evaluation on the same device tensors."""
    import torch
    from bayesflow_nddms_amd import amortizer
    kernel = S != "cap + 1"
    S = {"cap": _cap(), "cap + 1": _cap() + 1}.get(S, S)
    rng = np.random.default_rng(S + D)
    theta = (rng.normal(size=(B, S, D)) * rng.choice([1e-3, 1.0, 1e4], size=(1, 1, D))).astype(np.float32)
    if S > 2:
        theta[0, 2, D - 1] = np.nan
    lw = skewed_log_w(rng, B, S)
    words = amortizer.resample_words(B, seed=S)
    t, w = torch.from_numpy(theta).cuda(), torch.from_numpy(lw).cuda()
    for M in sorted({1, 63, 65, S, 3 * S + 1}):
        assert (amortizer._resample_lib(t, M, w) is not None) == kernel
        res = amortizer.resample_draws(t, M, log_w=w, words=words, want_weights=True)
        assert all(v.is_cuda for v in res.values())
        W = res["weights"].cpu().numpy()
        assert W.dtype == np.int64 and W.shape == (B, S) and np.abs(W - quantize(lw)).max() <= 1 and W.min() >= 0
        check(res, theta, W, words, M)
        properties(res, theta, W, M)
        given = amortizer.resample_draws(t, M, weights=res["weights"], words=words)
        ref = _fallback(t, M, weights=res["weights"], words=words)
        assert _same(res, given) and _same(res, ref)
    assert np.array_equal(bits(t.cpu().numpy()), bits(theta)) and np.array_equal(bits(w.cpu().numpy()), bits(lw))      # (the inputs are only read)


def test_crafted_rows_and_words():
    import torch
    from bayesflow_nddms_amd import amortizer
    for name, theta, W, words in word_cases():
        t, wt = torch.from_numpy(theta).cuda(), torch.from_numpy(W).cuda()
        keep = t.clone()
        for M in out_counts(theta.shape[1]):
            assert amortizer._resample_lib(t, M, wt) is not None
            res = amortizer.resample_draws(t, M, weights=wt, words=words)
            check(res, theta, W, words, M)
            properties(res, theta, W, M)
            check_word_case(name, res, theta, W, words, M)
            assert _same(res, _fallback(t, M, weights=wt, words=words)), name
        assert _same_bits(t, keep), name
    for name, theta, lw in crafted_cases():
        words = np.random.default_rng(1).integers(0, 2 ** 64, size=theta.shape[0], dtype=np.uint64)
        t, w = torch.from_numpy(theta).cuda(), torch.from_numpy(lw).cuda()
        for M in out_counts(theta.shape[1]):
            assert amortizer._resample_lib(t, M, w) is not None
            res = amortizer.resample_draws(t, M, log_w=w, words=words, want_weights=True)
            W = res["weights"].cpu().numpy()
            assert np.abs(W - quantize(lw)).max() <= 1, name
            check(res, theta, W, words, M)
            properties(res, theta, W, M)
            assert _same(res, _fallback(t, M, weights=res["weights"], words=words)), name


@pytest.mark.parametrize("S", [1, 64, 65, 1000, 10000])
def test_equal_weights_and_as_many_outputs_return_the_draws(S):
    import torch
    from bayesflow_nddms_amd import amortizer
    theta = np.random.default_rng(S).normal(size=(3, S, 5)).astype(np.float32)
    t = torch.from_numpy(theta).cuda()
    words = np.array([0, MAXW, int(amortizer.resample_words(1, 3)[0])], dtype=np.uint64)
    for level in (0.0, -731.25):
        w = torch.full((3, S), level, dtype=torch.float64, device="cuda")
        assert amortizer._resample_lib(t, S, w) is not None
        res = amortizer.resample_draws(t, S, log_w=w, words=words)
        assert torch.equal(res["ancestors"], torch.arange(S, dtype=torch.int32, device="cuda").expand(3, S))
        assert _same_bits(res["draws"], t) and res["n_unique"].tolist() == [S] * 3 and res["n_positive"].tolist() == [S] * 3


def test_a_set_depends_on_its_own_rows_only():
    """A repeated launch repeats every bit; set 1 of a B = 3 launch is that set launched alone with its word; with rows and weights
    permuted together every row still appears floor or ceil of its expected number of times (the ancestors themselves may differ: the
    running sums are in row order)."""
    import torch
    from bayesflow_nddms_amd.amortizer import resample_draws, resample_words
    rng = np.random.default_rng(8)
    B, S, D, M = 3, 1000, 5, 1500
    theta = rng.normal(size=(B, S, D)).astype(np.float32)
    theta[1, 7, 2] = np.nan
    lw = skewed_log_w(rng, B, S)
    words = resample_words(B, seed=2)
    t, w = torch.from_numpy(theta).cuda(), torch.from_numpy(lw).cuda()
    a, b = (resample_draws(t, M, log_w=w, words=words, want_weights=True) for _ in range(2))
    alone = resample_draws(t[1:2].contiguous(), M, log_w=w[1:2].contiguous(), words=words[1:2], want_weights=True)
    for k in KEYS + ("weights",):
        assert _same_bits(a[k], b[k]) and _same_bits(a[k][1:2], alone[k]), k
    assert 0 < int(a["n_positive"].min()) and int(a["n_positive"].max()) < S
    perm = rng.permutation(S)
    pt = torch.from_numpy(perm).cuda()
    mixed = resample_draws(t[:, pt].contiguous(), M, log_w=w[:, pt].contiguous(), words=words, want_weights=True)
    assert _same_bits(a["weights"][:, pt], mixed["weights"]) and torch.equal(a["n_positive"], mixed["n_positive"])
    Wm = mixed["weights"].cpu().numpy()
    check(mixed, theta[:, perm], Wm, words, M)
    properties(mixed, theta[:, perm], Wm, M)
    V, back = effective(theta, a["weights"].cpu().numpy()), mixed["ancestors"].cpu().numpy()
    for s in range(B):
        T, n = sum(V[s]), np.bincount(perm[back[s]], minlength=S).tolist()               # counts by ORIGINAL row
        assert all(abs(nk * T - M * vk) < T for nk, vk in zip(n, V[s]))


@pytest.mark.parametrize("S,M", [(65, 63), (1025, 1500)])
def test_nothing_is_written_outside_the_outputs(S, M):
    """out, ancestors, n_unique, n_positive and w_out are interior pointers into larger buffers filled with a sentinel: the guards on
    both sides are unchanged and every output element was written; theta, log_w and the words keep their bits; null optional outputs
    are accepted, and so are integer weights in place of log_w."""
    import torch
    from bayesflow_nddms_amd.amortizer import resample_words
    L = _lib()
    B, D, G, sent = 3, 5, 4096, -12345
    rng = np.random.default_rng(S)
    theta_np = rng.normal(size=(B, S, D)).astype(np.float32)
    theta = torch.from_numpy(theta_np).cuda()
    lw = torch.from_numpy(rng.normal(size=(B, S))).cuda()                                # (finite: every weight >= 1, none equal to the sentinel)
    words_np = resample_words(B, seed=S)
    words = torch.from_numpy(words_np.view(np.int64)).cuda()
    keep, keep_w, keep_r = theta.clone(), lw.clone(), words.clone()
    big_o = torch.full((2 * G + B * M * D,), float(sent), dtype=torch.float32, device="cuda")
    big_a = torch.full((2 * G + B * M,), sent, dtype=torch.int32, device="cuda")
    big_u, big_n = (torch.full((2 * G + B,), sent, dtype=torch.int64, device="cuda") for _ in range(2))
    big_w = torch.full((2 * G + B * S,), sent, dtype=torch.int64, device="cuda")
    bigs = ((big_o, B * M * D), (big_a, B * M), (big_u, B), (big_n, B), (big_w, B * S))
    st = torch.cuda.current_stream().cuda_stream

    def launch(optional, log_w=lw.data_ptr(), w_in=None):
        ptrs = [big[G:].data_ptr() for big, _ in bigs[1:]] if optional else [None] * 4
        return L.nddm_train_resample(B, S, D, M, theta.data_ptr(), log_w, w_in, words.data_ptr(), big_o[G:].data_ptr(), *ptrs, st)

    assert launch(True) == 0
    torch.cuda.synchronize()
    for big, n in bigs:
        assert bool((big[:G] == sent).all()) and bool((big[G + n:] == sent).all())
        assert not bool((big[G:G + n] == sent).any())
    res = {"draws": big_o[G:G + B * M * D].view(B, M, D), "ancestors": big_a[G:G + B * M].view(B, M), "n_unique": big_u[G:G + B],
           "n_positive": big_n[G:G + B]}
    W = big_w[G:G + B * S].view(B, S).clone()
    check(res, theta_np, W.cpu().numpy(), words_np, M)
    first = big_o.clone()
    for with_weights in (False, True):
        for big, _ in bigs:
            big.fill_(sent)
        assert (launch(False, log_w=None, w_in=W.data_ptr()) if with_weights else launch(False)) == 0
        torch.cuda.synchronize()
        assert _same_bits(big_o, first) and all(bool((big == sent).all()) for big, _ in bigs[1:])
    assert _same_bits(theta, keep) and _same_bits(lw, keep_w) and _same_bits(words, keep_r)


@pytest.mark.parametrize("ragged", [False, True], ids=["equal counts", "ragged"])
def test_public_path(monkeypatch, ragged):
    """B = 3, S = 2000, 12 trials.  resample=None calls no new kernel and returns the old keys; with resample=M every old number keeps
    its bits under the same seed and torch's generator ends where it did; "resampled" is resample_draws' on keep_draws' /
    keep_weights' outputs with the call's words, and the reference's on those integer weights; the kernel is called once per launch;
    one set per launch (a small z_bytes) gives each set the bits of the one-launch call whose every launch is seeded alike;
    smooth=True resamples the smoothed weights; sample_exact returns the documented shape and fills last_exact."""
    import torch
    from bayesflow_nddms_amd.amortizer import resample_draws, resample_words
    B, S, P, M = 3, 2000, 5, 3000
    am, conf = _people(ragged)
    L = _lib()
    calls = []
    real = L.nddm_train_resample
    monkeypatch.setattr(L, "nddm_train_resample", lambda *a: calls.append(a[:4]) or real(*a))
    torch.manual_seed(21)
    old = am.posterior_importance(conf, S)
    after = torch.cuda.get_rng_state()
    assert set(old) == OLD_KEYS and not calls
    torch.manual_seed(21)
    new = am.posterior_importance(conf, S, resample=M, resample_seed=5, keep_draws=True, keep_weights=True)
    assert torch.equal(torch.cuda.get_rng_state(), after)
    assert calls == [(B, S, P, M)]
    assert set(new) == OLD_KEYS | {"resampled", "n_unique", "resample_seed", "draws", "log_q", "log_w"} and new["resample_seed"] == 5
    for k in OLD_KEYS - {"n_samples"}:
        assert np.array_equal(bits(old[k]), bits(new[k])), k
    assert new["resampled"].shape == (B, M, P) and new["resampled"].dtype == np.float32 and np.isfinite(new["resampled"]).all()
    words = resample_words(B, 5)
    draws, log_w = torch.as_tensor(new["draws"], device="cuda"), torch.as_tensor(new["log_w"], device="cuda")
    again = resample_draws(draws, M, log_w=log_w, words=words, want_weights=True)
    assert len(calls) == 2 and np.array_equal(bits(again["draws"].cpu().numpy()), bits(new["resampled"]))
    assert np.array_equal(again["n_unique"].cpu().numpy(), new["n_unique"])
    W = again["weights"].cpu().numpy()
    assert np.abs(W - quantize(new["log_w"])).max() <= 1 and int(again["n_positive"].min()) > 20 and int(new["n_unique"].min()) > 10
    check(again, new["draws"], W, words, M)
    properties(again, new["draws"], W, M)
    anc = again["ancestors"].cpu().numpy()
    assert np.array_equal(bits(new["resampled"]), bits(np.stack([new["draws"][b, anc[b]] for b in range(B)])))
    print("public path: ess", new["ess"], "n_positive", again["n_positive"].tolist(), "n_unique", new["n_unique"].tolist())
    # smooth=True resamples the smoothed weights; sample_exact is that call
    torch.manual_seed(21)
    sm = am.posterior_importance(conf, S, smooth=True, resample=M, resample_seed=5, keep_draws=True, keep_weights=True)
    ref_s = resample_draws(torch.as_tensor(sm["draws"], device="cuda"), M, log_w=torch.as_tensor(sm["log_w_smoothed"], device="cuda"), words=words)
    assert np.array_equal(bits(sm["resampled"]), bits(ref_s["draws"].cpu().numpy())) and np.array_equal(bits(sm["raw"]["mean"]), bits(old["mean"]))
    torch.manual_seed(21)
    got = am.sample_exact(conf, M, n_proposals=S, seed=5)
    assert isinstance(got, np.ndarray) and got.shape == (B, M, P) and np.array_equal(bits(got), bits(sm["resampled"]))
    assert np.array_equal(am.last_exact["n_unique"], sm["n_unique"]) and np.array_equal(bits(am.last_exact["ess"]), bits(sm["ess"]))
    assert np.array_equal(bits(am.last_exact["pareto_k"]), bits(sm["pareto_k"])) and am.last_exact["k_threshold"] == sm["k_threshold"]
    one = am.sample_exact({k: v[:1] for k, v in conf.items()}, 70, to_numpy=False)
    assert torch.is_tensor(one) and one.is_cuda and one.shape == (70, P) and am.last_exact["n_proposals"] == 70
    # two launches (2 + 1 sets) and three (one set each) against one launch, every launch's base normals seeded per set
    with torch.no_grad():
        cond = am._conditions(conf)
    monkeypatch.setattr(am, "_conditions", lambda d: cond)
    randn = torch.randn

    def seeded(n, *a, **kw):                                   # the base normals of a launch: set b's under seed 100 + b, whatever the launch
        parts = []
        for _ in range(n // S):
            torch.manual_seed(100 + seeded.b)
            parts.append(randn(S, *a, **kw))
            seeded.b += 1
        return torch.cat(parts, dim=0)

    results = []
    for z_bytes in (64 << 20, 2 * 4 * S * P, 4 * S * P):
        seeded.b = 0
        monkeypatch.setattr(torch, "randn", seeded)
        n_calls = len(calls)
        results.append(am.posterior_importance(conf, S, resample=M, resample_seed=5, z_bytes=z_bytes))
        monkeypatch.setattr(torch, "randn", randn)
        assert len(calls) - n_calls == {64 << 20: 1, 2 * 4 * S * P: 2, 4 * S * P: 3}[z_bytes]
    for other in results[1:]:
        for k in ("mean", "std", "ess", "log_evidence", "resampled", "n_unique"):
            assert np.array_equal(bits(other[k]), bits(results[0][k])), k


def test_end_to_end_against_an_independent_float64_posterior():
    """The setting of tests/test_gpu_flow_importance.py's end-to-end test: its data set and prior-proposal posterior (tests/golden/
    flow_importance.npz), its proposal flow -- half an sd off in beta -- and its base normals.  The draws are weighted on the device
    and resampled into as many equally weighted ones: all PROPOSAL_DRAWS = 20 000 (more than the kernel's cap: the torch evaluation on
    the device) and the first cap of them (the kernel; a prefix of independent draws is as good a sample).  The PLAIN mean of the
    resampled draws meets the golden mean within mean_bound(sd, 1 / (1 / ess + 1 / M), ess_ref): resampling adds at most sd^2 / M of
    variance to the weighted estimate, so the effective size of the resampled mean is the harmonic combination.  The unweighted mean
    of the same draws misses that bound in the beta column: without the resampling the test fails."""
    import torch
    from bayesflow_nddms_amd import amortizer, engine
    g = np.load(GOLDEN)
    net = proposal_flow(g["mean"], g["sd"]).cuda()
    z = torch.randn(1, PROPOSAL_DRAWS, 5, generator=torch.Generator().manual_seed(PROPOSAL_SEED)).cuda()
    cond = torch.zeros(1, 11, device="cuda")
    with torch.no_grad():
        assert net._sample_lib(z, cond) is not None
        th_all, lq_all = net.inverse_per_set(z, cond, log_density=True)
    trials = torch.as_tensor(g["trials"], device="cuda")[None]
    ll_all = engine.wiener_log_likelihood(engine.BASIC_DDM_DC, th_all.view(-1, 5), trials, draws_per_dataset=PROPOSAL_DRAWS)["loglik"].view(1, -1)
    ess_ref = float(g["ess"])
    for S in (PROPOSAL_DRAWS, _cap()):
        th, lq, ll = th_all[:, :S].contiguous(), lq_all[:, :S].contiguous(), ll_all[:, :S].contiguous()
        w = amortizer.importance_weights(th, lq, ll, "basic", want_log_w=True)
        ess, M = float(w["ess"][0]), S
        assert (amortizer._resample_lib(th, M, w["log_w"]) is not None) == (S <= _cap())
        res = amortizer.resample_draws(th, M, log_w=w["log_w"], seed=PROPOSAL_SEED)
        mean = res["draws"][0].double().mean(dim=0).cpu().numpy()
        bound = mean_bound(g["sd"], 1.0 / (1.0 / ess + 1.0 / M), ess_ref)
        err, err_plain = np.abs(mean - g["mean"]), np.abs(th[0].double().mean(dim=0).cpu().numpy() - g["mean"])
        print("S", S, "ess", ess, "n_unique", int(res["n_unique"][0]), "resampled |mean - ref| / bound", err / bound, "unweighted", err_plain / bound)
        assert ess >= 0.05 * S, ess
        assert np.all(err <= bound), (err, bound)
        assert err_plain[2] > bound[2], (err_plain, bound)
