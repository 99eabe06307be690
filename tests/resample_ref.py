"""The definition of sampling-importance-resampling (amortizer.resample_draws, csrc/train_resample.hip) in pure Python integers, one
set at a time; independent of torch.  Test infrastructure only: nothing in the product imports it.

  reference    theta float32 [B, S, D], integer weights [B, S], words uint64 [B] and M -> (draws [B, M, D] float32, ancestors [B, M]
               int32, n_unique [B], n_positive [B]); the comb position as the 128-bit expression floor((j T + U) / M)
  check        resample_draws' dictionary against it: ancestors, n_unique, n_positive exactly, draws bit for bit
  properties   what follows from the rule, asserted on a result
  word_for     the word r = ceil(U 2^64 / T) that gives the offset U
"""
import bisect

import numpy as np

from wquantile_ref import bits, crafted_cases, quantize, skewed_log_w  # noqa: F401  (re-exported to the tests)

ONE = 2 ** 36
TWO64 = 2 ** 64


def effective(theta, weights):
    """V [B][S] as Python integers: W_i where every component of row i is finite, else 0."""
    fin = np.isfinite(np.asarray(theta, dtype=np.float32)).all(axis=-1)
    return [[int(w) if f else 0 for w, f in zip(wr, fr)] for wr, fr in zip(np.asarray(weights).tolist(), fin.tolist())]


def offset(r, T):
    return (int(r) * T) >> 64


def word_for(U, T):
    """The smallest word with offset(r, T) == U (0 <= U < T)."""
    r = -((-U * TWO64) // T)
    assert 0 <= r < TWO64 and offset(r, T) == U
    return r


def ancestors_of(V, r, M):
    """One set: V Python integers, r the word -> the list of M ancestors (-1 each if the total is 0)."""
    C, run = [], 0
    for v in V:
        run += v
        C.append(run)
    T = run
    if T == 0:
        return [-1] * M
    U = offset(r, T)
    assert 0 <= U < T <= 2 ** 50
    out = []
    for j in range(M):
        t = (j * T + U) // M
        q, rho, qU, rhoU = T // M, T % M, U // M, U % M
        assert t == j * q + qU + (j * rho + rhoU) // M < T and j * q + qU + j * rho + rhoU < 2 ** 63          # (the kernel's 64-bit form)
        out.append(bisect.bisect_right(C, t))                                            # the smallest k with C_k > t
    return out


def reference(theta, weights, words, M):
    theta = np.asarray(theta, dtype=np.float32)
    W = np.asarray(weights)
    assert W.dtype == np.int64 and W.shape == theta.shape[:2] and W.min() >= 0 and W.max() <= ONE
    B, S, D = theta.shape
    V = effective(theta, W)
    draws = np.full((B, M, D), np.nan, dtype=np.float32)
    anc = np.full((B, M), -1, dtype=np.int32)
    n_unique, n_positive = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    for b in range(B):
        n_positive[b] = sum(v >= 1 for v in V[b])
        a = ancestors_of(V[b], int(words[b]), M)
        if a[0] < 0:
            continue
        anc[b] = a
        draws[b] = theta[b, a]
        n_unique[b] = len(set(a))
    return draws, anc, n_unique, n_positive


def check(res, theta, weights, words, M):
    """res: resample_draws' dictionary (tensors) for theta (numpy float32), the integer weights and the words."""
    draws, anc, n_unique, n_positive = reference(theta, weights, words, M)
    got = {k: res[k].cpu().numpy() for k in ("draws", "ancestors", "n_unique", "n_positive")}
    assert got["draws"].dtype == np.float32 and got["ancestors"].dtype == np.int32
    assert got["n_unique"].dtype == np.int64 and got["n_positive"].dtype == np.int64
    assert got["draws"].shape == draws.shape and got["ancestors"].shape == anc.shape
    assert np.array_equal(got["n_positive"], n_positive), (got["n_positive"], n_positive)
    assert np.array_equal(got["ancestors"], anc), np.flatnonzero((got["ancestors"] != anc).any(axis=1))
    assert np.array_equal(got["n_unique"], n_unique), (got["n_unique"], n_unique)
    assert np.array_equal(bits(got["draws"]), bits(draws))


def properties(res, theta, weights, M):
    """a_j does not decrease in j; a row with V = 0 is never chosen; |n_k T - M V_k| < T for every row; a set with T = 0 is NaN, -1, 0;
    n_unique <= min(M, n_positive)."""
    anc, n_unique, n_positive = (res[k].cpu().numpy() for k in ("ancestors", "n_unique", "n_positive"))
    draws = res["draws"].cpu().numpy()
    V = effective(theta, weights)
    S = len(V[0])
    for b in range(len(V)):
        T = sum(V[b])
        if T == 0:
            assert (anc[b] == -1).all() and np.isnan(draws[b]).all() and n_unique[b] == 0 and n_positive[b] == 0
            continue
        assert np.all(np.diff(anc[b]) >= 0) and anc[b].min() >= 0 and anc[b].max() < S
        n = np.bincount(anc[b], minlength=S).tolist()
        assert all(abs(nk * T - M * vk) < T for nk, vk in zip(n, V[b])), b               # (so V_k = 0 gives n_k = 0)
        assert 1 <= n_unique[b] <= min(M, n_positive[b]) and np.isfinite(draws[b]).all()
