"""Sampling-importance-resampling (csrc/train_resample.hip, amortizer.py: resample_words / resample_draws / posterior_importance(
resample=...) / AmortizedPosterior.sample_exact) as far as a machine without a GPU can hold it: the library's exports and host
refusals, and the PyTorch evaluation of the definition -- the path every CPU tensor takes and the one the kernel is held to bit for bit
(tests/test_gpu_flow_resample.py) -- against tests/resample_ref.py's recomputation in Python integers, the properties that follow
from the rule, exact unbiasedness over every offset, and the public call."""
import ctypes

import numpy as np
import pytest

from resample_ref import ONE, TWO64, bits, check, crafted_cases, effective, offset, properties, quantize, skewed_log_w, word_for
from test_flow_wquantile_cpu import OLD_KEYS, _host_likelihood, _small_amortizer

CAP = 16384
MAXW = TWO64 - 1


def out_counts(S):
    """M on both sides of S, and 1 and 2."""
    return sorted({1, 2, max(1, S - 1), S, 3 * S + 1})


def word_cases():
    """(name, theta float32 [B, S, D], integer weights [B, S], words uint64 [B]): the words and weights a comb goes wrong on."""
    rng = np.random.default_rng(29)
    cases = []
    theta = np.repeat(rng.normal(size=(1, 130, 3)).astype(np.float32), 2, axis=0)
    W = np.repeat(quantize(skewed_log_w(rng, 1, 130)), 2, axis=0)
    cases.append(("r = 0 and r = 2^64 - 1", theta, W, np.array([0, MAXW], dtype=np.uint64)))
    for name, th, lw in crafted_cases():
        if name in ("one dominating weight", "all-zero sets", "nan / inf components", "log_w -inf, +inf, nan"):
            cases.append((name, th, quantize(lw), rng.integers(0, TWO64, size=th.shape[0], dtype=np.uint64)))
    bad = rng.normal(size=(2, 97, 5)).astype(np.float32)
    bad_w = quantize(rng.normal(size=(2, 97)))
    bad[0, int(np.argmax(bad_w[0])), 2], bad[1, int(np.argmax(bad_w[1])), 0] = np.nan, np.inf
    cases.append(("the largest weight on a row that is not finite", bad, bad_w, np.array([MAXW, 12345], dtype=np.uint64)))
    full = rng.normal(size=(1, CAP, 1)).astype(np.float32)
    cases.append(("the largest T", full, np.full((1, CAP), ONE, dtype=np.int64), np.array([MAXW], dtype=np.uint64)))
    return cases


def check_word_case(name, res, theta, W, words, M):
    """What each crafted case must show, beyond equality with the reference."""
    anc, n_unique, n_positive = (res[k].cpu().numpy() for k in ("ancestors", "n_unique", "n_positive"))
    V = effective(theta, W)
    if name == "r = 0 and r = 2^64 - 1":
        T = sum(V[0])
        assert offset(0, T) == 0 and offset(MAXW, T) == T - 1
        pos = [k for k, v in enumerate(V[0]) if v >= 1]
        assert anc[0, 0] == pos[0]                                                       # t_0 = 0: the first row that weighs anything
        if M == 1:
            assert anc[1, 0] == pos[-1]                                                  # t_0 = T - 1: the last one
    if name == "one dominating weight":
        assert n_positive.tolist() == [1, 1] and n_unique.tolist() == [1, 1] and (anc[0] == 41).all() and (anc[1] == 199).all()
    if name == "all-zero sets":
        assert n_positive.tolist() == [0, 0] and n_unique.tolist() == [0, 0] and (anc == -1).all() and np.isnan(res["draws"].cpu().numpy()).all()
    if name == "the largest weight on a row that is not finite":
        assert n_positive.tolist() == [96, 96]
        for b in range(2):
            assert int(np.argmax(W[b])) not in set(anc[b].tolist())
    if name == "the largest T":
        assert sum(V[0]) == 2 ** 50
        if M == CAP:
            assert np.array_equal(anc[0], np.arange(CAP))


@pytest.mark.parametrize("S", [1, 2, 3, 64, 65, 257, 1000])
def test_resample_draws_on_cpu_tensors(S):
    """Random skewed weights: the torch evaluation equals the reference bit for bit, from log_w (torch's own quantisation) and from
    the integer weights; the properties hold."""
    import torch
    from bayesflow_nddms_amd.amortizer import quantize_weights, resample_draws, resample_words
    rng = np.random.default_rng(S)
    for D in (1, 5, 8):
        theta = (rng.normal(size=(2, S, D)) * 10.0 ** rng.integers(-3, 4)).astype(np.float32)
        if S > 2:
            theta[1, 1, D - 1] = np.nan
        lw = skewed_log_w(rng, 2, S)
        words = resample_words(2, seed=S + D)
        for M in out_counts(S):
            res = resample_draws(torch.from_numpy(theta), M, log_w=torch.from_numpy(lw), words=words, want_weights=True)
            assert all(not v.is_cuda for v in res.values()) and res["draws"].shape == (2, M, D)
            W = res["weights"].numpy()
            assert np.array_equal(W, quantize_weights(torch.from_numpy(lw)).numpy())
            check(res, theta, W, words, M)
            properties(res, theta, W, M)
            again = resample_draws(torch.from_numpy(theta), M, weights=torch.from_numpy(W), words=torch.from_numpy(words.view(np.int64)))
            assert "weights" not in again
            check(again, theta, W, words, M)
    one = resample_draws(torch.from_numpy(theta[0]), M, log_w=torch.from_numpy(lw[0]), words=words[:1])     # [S, D]: one set
    assert one["draws"].shape == (1, M, 8) and torch.equal(one["ancestors"][0], res["ancestors"][0])
    default = resample_draws(torch.from_numpy(theta), 4, log_w=torch.from_numpy(lw), seed=5)               # words=None: resample_words(B, seed)
    check(default, theta, W, resample_words(2, seed=5), 4)


def test_crafted_rows_and_words():
    import torch
    from bayesflow_nddms_amd.amortizer import resample_draws
    for name, theta, W, words in word_cases():
        for M in out_counts(theta.shape[1]):
            res = resample_draws(torch.from_numpy(theta), M, weights=torch.from_numpy(W), words=words)
            check(res, theta, W, words, M)
            properties(res, theta, W, M)
            check_word_case(name, res, theta, W, words, M)
    for name, theta, lw in crafted_cases():
        words = np.random.default_rng(1).integers(0, TWO64, size=theta.shape[0], dtype=np.uint64)
        for M in out_counts(theta.shape[1]):
            res = resample_draws(torch.from_numpy(theta), M, log_w=torch.from_numpy(lw), words=words, want_weights=True)
            W = res["weights"].numpy()
            assert np.abs(W - quantize(lw)).max() <= 1, name
            check(res, theta, W, words, M)
            properties(res, theta, W, M)


@pytest.mark.parametrize("S", [1, 7, 64, 1000])
def test_equal_weights_and_as_many_outputs_return_the_draws(S):
    import torch
    from bayesflow_nddms_amd.amortizer import resample_draws, resample_words
    theta = np.random.default_rng(S).normal(size=(3, S, 4)).astype(np.float32)
    words = np.array([0, MAXW, int(resample_words(1, 3)[0])], dtype=np.uint64)
    for level in (0.0, -731.25):
        res = resample_draws(torch.from_numpy(theta), S, log_w=torch.full((3, S), level, dtype=torch.float64), words=words)
        assert np.array_equal(res["ancestors"].numpy(), np.tile(np.arange(S, dtype=np.int32), (3, 1)))
        assert np.array_equal(bits(res["draws"].numpy()), bits(theta)) and res["n_unique"].tolist() == [S] * 3


@pytest.mark.parametrize("M", [1, 2, 5, 12, 31])
def test_exactly_unbiased_over_every_offset(M):
    """Small integer weights with zeros among them: over all T offsets U -- each through the word r = ceil(U 2^64 / T), which the
    reference and the torch evaluation both turn back into U -- row k is chosen exactly M V_k times."""
    import torch
    from bayesflow_nddms_amd.amortizer import resample_draws
    V = np.array([3, 0, 1, 7, 0, 0, 2, 11, 1, 0, 5], dtype=np.int64)
    S, T = len(V), int(V.sum())
    words = np.array([word_for(U, T) for U in range(T)], dtype=np.uint64)
    theta = np.tile(np.arange(S, dtype=np.float32)[None, :, None], (T, 1, 2))
    W = np.tile(V, (T, 1))
    res = resample_draws(torch.from_numpy(theta), M, weights=torch.from_numpy(W), words=words)
    check(res, theta, W, words, M)
    counts = np.bincount(res["ancestors"].numpy().reshape(-1), minlength=S)
    assert np.array_equal(counts, M * V), (counts, M * V)
    assert np.array_equal(res["draws"][:, :, 0].numpy(), res["ancestors"].numpy().astype(np.float32))


def test_resample_words_are_reproducible_and_leave_torch_alone():
    import torch
    from bayesflow_nddms_amd.amortizer import resample_words
    torch.manual_seed(9)
    state = torch.get_rng_state()
    a, b, c = resample_words(7, seed=3), resample_words(7, seed=3), resample_words(7, seed=4)
    assert torch.equal(torch.get_rng_state(), state)
    assert a.dtype == np.uint64 and a.shape == (7,) and np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.array_equal(resample_words(3, seed=3), a[:3])                              # set b's word does not depend on B
    assert np.array_equal(a, np.random.Generator(np.random.Philox(3)).integers(0, 2 ** 64, size=7, dtype=np.uint64))
    assert np.array_equal(resample_words(4), resample_words(4, seed=0))
    with pytest.raises(ValueError):
        resample_words(0)


def test_library_exports_the_entry_and_refuses_bad_arguments_on_the_host():
    """Called with null or dummy pointers, on the host: had the entry read or launched anything, this would not return."""
    from bayesflow_nddms_amd import _train_lib, amortizer, build
    raw = ctypes.CDLL(build.build_train())
    assert all(hasattr(raw, n) for n in ("nddm_train_resample", "nddm_train_resample_max_draws", "nddm_train_resample_max_out"))
    assert any(p.endswith("train_resample.hip") for p in build.TRAIN_SOURCES) and any(p.endswith("train_weight.h") for p in build.TRAIN_HEADERS)
    L = _train_lib.lib()
    assert L is not None, "libnddm_train.so did not build / load"
    cap = L.nddm_train_resample_max_draws()
    assert cap >= CAP and L.nddm_train_resample_max_out() == 2 ** 20 == amortizer.RESAMPLE_MAX_OUT
    buf = (ctypes.c_char * 64)()
    a = ctypes.addressof(buf)

    def rc(B=1, S=100, D=5, M=10, theta=a, log_w=a, w_in=None, words=a, out=a):
        return L.nddm_train_resample(B, S, D, M, theta, log_w, w_in, words, out, None, None, None, None, None)

    assert rc(S=cap + 1) == 1 and rc(D=9) == 1 and rc(M=2 ** 20 + 1) == 1
    assert rc(log_w=a, w_in=a) == 1 and rc(log_w=None, w_in=None) == 1
    assert rc(B=0) == 1 and rc(S=0) == 1 and rc(D=0) == 1 and rc(M=0) == 1
    assert rc(theta=None) == 1 and rc(words=None) == 1 and rc(out=None) == 1 and rc(theta=None, log_w=None, w_in=a) == 1


def test_python_validation():
    import torch
    from bayesflow_nddms_amd.amortizer import resample_draws
    th, lw, W = torch.zeros(2, 4, 3), torch.zeros(2, 4, dtype=torch.float64), torch.ones(2, 4, dtype=torch.int64)
    for kw in ({}, {"log_w": lw, "weights": W}):                                        # neither, both
        with pytest.raises(ValueError, match="exactly one"):
            resample_draws(th, 3, **kw)
    for M in (0, -1):
        with pytest.raises(ValueError, match="at least 1"):
            resample_draws(th, M, log_w=lw)
    with pytest.raises(ValueError):
        resample_draws(th, 3, log_w=lw[:, :3])
    with pytest.raises(ValueError):
        resample_draws(th, 3, weights=W[:1])
    with pytest.raises(ValueError, match="int64"):
        resample_draws(th, 3, weights=W.double())
    with pytest.raises(ValueError):
        resample_draws(torch.zeros(4), 3, log_w=lw)
    with pytest.raises(ValueError):
        resample_draws(torch.zeros(2, 0, 3), 3, log_w=torch.zeros(2, 0, dtype=torch.float64))
    with pytest.raises(ValueError, match="words"):
        resample_draws(th, 3, log_w=lw, words=np.zeros(3, dtype=np.uint64))
    with pytest.raises(ValueError, match="words"):
        resample_draws(th, 3, log_w=lw, words=np.zeros(2, dtype=np.float64))
    with pytest.raises(ValueError, match="words"):
        resample_draws(th, 3, log_w=lw, words=torch.zeros(2, dtype=torch.float64))


def test_posterior_importance_resample_on_the_cpu(monkeypatch):
    """resample=None returns exactly the old keys; with resample=M every old number keeps its bits under the same seed, torch's random
    stream is consumed alike, "resampled" is draws[ancestors] of resample_draws on keep_draws' / keep_weights' outputs with the call's
    words, one set per launch gives the same bits, smooth=True resamples the smoothed weights, and sample_exact returns them."""
    import torch
    from bayesflow_nddms_amd.amortizer import resample_draws, resample_words
    _host_likelihood(monkeypatch)
    B, S, M = 2, 300, 450
    am, conf = _small_amortizer(B)
    torch.manual_seed(3)
    old = am.posterior_importance(conf, S)
    after = torch.get_rng_state()
    assert set(old) == OLD_KEYS
    torch.manual_seed(3)
    new = am.posterior_importance(conf, S, resample=M, resample_seed=7, keep_draws=True, keep_weights=True)
    assert torch.equal(torch.get_rng_state(), after)
    assert set(new) == OLD_KEYS | {"resampled", "n_unique", "resample_seed", "draws", "log_q", "log_w"} and new["resample_seed"] == 7
    for k in OLD_KEYS - {"n_samples"}:
        assert np.array_equal(bits(old[k]), bits(new[k])), k
    assert new["resampled"].shape == (B, M, 5) and new["resampled"].dtype == np.float32 and new["n_unique"].dtype == np.int64
    words = resample_words(B, 7)
    ref = resample_draws(torch.from_numpy(new["draws"]), M, log_w=torch.from_numpy(new["log_w"]), words=words, want_weights=True)
    check(ref, new["draws"], ref["weights"].numpy(), words, M)
    anc = ref["ancestors"].numpy()
    assert np.array_equal(bits(new["resampled"]), bits(np.stack([new["draws"][b, anc[b]] for b in range(B)])))
    assert np.array_equal(new["n_unique"], ref["n_unique"].numpy()) and new["n_unique"].min() > 10
    torch.manual_seed(3)
    other = am.posterior_importance(conf, S, resample=M, resample_seed=8)
    assert not np.array_equal(other["resampled"], new["resampled"])
    # one set per launch: set b resampled with words[b]
    torch.manual_seed(3)
    first = am.posterior_importance(conf, S, resample=M, resample_seed=7, z_bytes=1, keep_draws=True, keep_weights=True)
    ref1 = resample_draws(torch.from_numpy(first["draws"]), M, log_w=torch.from_numpy(first["log_w"]), words=words)
    assert np.array_equal(bits(first["resampled"]), bits(ref1["draws"].numpy()))
    torch.manual_seed(3)
    assert np.array_equal(bits(first["mean"]), bits(am.posterior_importance(conf, S, z_bytes=1)["mean"]))
    # smoothed
    torch.manual_seed(3)
    sm = am.posterior_importance(conf, S, smooth=True, resample=M, resample_seed=7, keep_draws=True, keep_weights=True)
    ref_s = resample_draws(torch.from_numpy(sm["draws"]), M, log_w=torch.from_numpy(sm["log_w_smoothed"]), words=words)
    assert np.array_equal(bits(sm["resampled"]), bits(ref_s["draws"].numpy()))
    assert np.array_equal(bits(sm["raw"]["mean"]), bits(old["mean"]))
    torch.manual_seed(3)
    got = am.sample_exact(conf, M, n_proposals=S, seed=7)
    assert isinstance(got, np.ndarray) and np.array_equal(bits(got), bits(sm["resampled"]))
    assert set(am.last_exact) >= {"ess", "n_unique", "pareto_k", "k_threshold"} and am.last_exact["k_threshold"] == sm["k_threshold"]
    assert np.array_equal(am.last_exact["n_unique"], sm["n_unique"]) and np.array_equal(bits(am.last_exact["pareto_k"]), bits(sm["pareto_k"]))
    am1, conf1 = _small_amortizer(1)
    one = am1.sample_exact(conf1, 50, smooth=False, to_numpy=False)
    assert torch.is_tensor(one) and one.shape == (50, 5) and am1.last_exact["pareto_k"] is None and am1.last_exact["n_proposals"] == 50
    with pytest.raises(ValueError, match="resample"):
        am.posterior_importance(conf, S, resample=0)
    with pytest.raises(NotImplementedError, match="single_trial_logpdf"):
        am.posterior_importance(conf, S, model="single", resample=M)


def test_resampled_mean_is_the_weighted_mean():
    """A statistical check with its own yardstick: 2 000 standard-normal draws with skewed weights, resampled into 2 000 under 64
    different words.  The mean over the 64 resampled means lies within 4 standard errors of the weighted mean, the standard error
    being the empirical one across the 64 repetitions (systematic resampling is unbiased; nothing is assumed about its variance)."""
    import torch
    from bayesflow_nddms_amd.amortizer import resample_draws, resample_words
    rng = np.random.default_rng(64)
    S = M = 2000
    R, D = 64, 3
    theta = rng.normal(size=(S, D)).astype(np.float32)
    W = quantize(skewed_log_w(rng, 1, S))
    target = (W[0][:, None].astype(np.float64) * theta.astype(np.float64)).sum(axis=0) / float(W.sum())
    res = resample_draws(torch.from_numpy(np.tile(theta[None], (R, 1, 1))), M, weights=torch.from_numpy(np.tile(W, (R, 1))),
                         words=resample_words(R, seed=1))
    means = res["draws"].double().mean(dim=1).numpy()                                    # [R, D]
    se = means.std(axis=0, ddof=1) / np.sqrt(R)
    err = np.abs(means.mean(axis=0) - target)
    print("weighted mean", target, "|mean of means - it| / se", err / se, "plain mean", theta.mean(axis=0))
    assert len({tuple(a) for a in res["ancestors"].numpy().tolist()}) > R // 2           # (the words do move the comb)
    assert np.all(se > 0) and np.all(err <= 4.0 * se), (err, se)
