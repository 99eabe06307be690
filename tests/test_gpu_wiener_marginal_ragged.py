"""GPU tests of the marginal log-likelihood with a trial count per data set and rows of 7 or 8 columns (include/nddm.h:
nddm_wiener_marginal_log_likelihood_ragged; csrc/nddm_wiener_marginal.h, the RAGGED instantiations): every set's rows have the bits of
the plain entry point on that set alone at its own length, in both layouts; the padding is never read (it holds NaN) and its per-trial
values are 0; without counts and with 8 columns the bits are the plain entry point's, and a 7-column row is the 8-column row with gamma =
1.0f; a count outside [1, n_trials] gives NaN in its own set's rows only; stores stay inside the outputs; the status codes."""
import functools

import numpy as np
import pytest

import wiener_marginal_ref as M

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 65, 1025)        # one trial; a wave less one; a wave and one; WIENER_TILE = 1024 and one
N_PAD = 1030
K_TRIALS = 40                     # distinct trials per data set; a data set cycles through them
TC = M.PRIOR_T_CENSOR


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@functools.lru_cache(maxsize=None)
def _sets():
    """Four base rows of the prior set whose own trial is a timeout, and per row K_TRIALS trials drawn from it, the timeout first:
    (float32 rows [4, 8], float32 trials [4, K_TRIALS, 2])."""
    p32, y32, z32, tc = M.prior_rows(M.POOL)
    assert tc == TC
    base = np.flatnonzero(y32 == 0)[:len(COUNTS)]
    assert base.size == len(COUNTS)
    pb = p32[base]
    ym, zm = M.more_trials("prior_rows", pb, K_TRIALS - 1, seed=41)
    y, z = np.concatenate([y32[base, None], ym], 1), np.concatenate([z32[base, None], zm], 1)
    assert np.all(y[:, 0] == 0) and np.any(y[:, 1:] != 0)
    return pb, np.stack([y, z], -1).astype(np.float32)


def _case(S, counts=COUNTS, n_pad=N_PAD):
    """-> rows [D * S, 8] (a set's base row and S - 1 copies moved by up to 3 %, gamma = 1), data [D, n_pad, 2] with NaN from each set's
    count on."""
    pb, tr = _sets()
    D = len(counts)
    rng = np.random.default_rng(S)
    rows = np.repeat(pb[:D], S, 0).astype(np.float64)
    jit = 1.0 + 0.03 * rng.uniform(-1, 1, (D * S, 5))
    jit[::S] = 1.0
    rows[:, [0, 1, 4, 5, 6]] *= jit
    data = np.full((D, n_pad, 2), np.nan, np.float32)
    for d, n in enumerate(counts):
        n = max(0, min(n, n_pad))
        data[d, :n] = tr[d, np.arange(n) % K_TRIALS]
    return rows.astype(np.float32), data


def _plain(torch, rows, data, d, n, S):
    """The existing entry point on set d alone at n_trials = n."""
    from bayesflow_nddms_amd import engine
    return engine.wiener_marginal_log_likelihood(engine.SINGLE_TRIAL, rows[d * S:(d + 1) * S].contiguous(), data[d:d + 1, :n].contiguous(),
                                                 draws_per_dataset=S, t_censor=TC, per_trial=True)


def _raw(torch, p, cols, S, data, counts, tc=TC, flags=0, out_trial=None, out_sum=None, R=None):
    from bayesflow_nddms_amd import _lib, engine
    L = _lib.lib()
    ptr = lambda t: None if t is None else t.data_ptr()              # noqa: E731
    return L.nddm_wiener_marginal_log_likelihood_ragged(int(engine.SINGLE_TRIAL), ptr(p), cols, p.shape[0] if R is None else R, S, ptr(data),
                                                        data.shape[1], ptr(counts), tc, flags, ptr(out_trial), ptr(out_sum),
                                                        torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("S", [1, 4, 15, 16, 17, 33])
def test_every_set_has_the_bits_of_a_call_on_it_alone(S):
    """S < 16: the paired layout (S = 15: a ragged last workgroup); S >= 16: the broadcast layout (17, 33: a chunk tail of one row and
    three waves that only stage).  With 8 columns and with 7."""
    torch = _torch()
    from bayesflow_nddms_amd import engine
    rows_np, data_np = _case(S)
    rows, data = torch.as_tensor(rows_np).cuda(), torch.as_tensor(data_np).cuda()
    counts = torch.tensor(COUNTS, dtype=torch.int32, device="cuda")
    for p in (rows, rows[:, :7].contiguous()):
        r = engine.wiener_marginal_log_likelihood(engine.SINGLE_TRIAL, p, data, draws_per_dataset=S, t_censor=TC, per_trial=True, counts=counts)
        assert r["loglik"].shape == (len(COUNTS) * S,) and r["trial_logp"].shape == (len(COUNTS) * S, N_PAD)
        for d, n in enumerate(COUNTS):
            ref = _plain(torch, rows, data, d, n, S)
            assert torch.isfinite(ref["loglik"]).all(), (d, n)
            assert bool((data[d, :n, 0] == 0).any())                     # a timeout in every set
            assert torch.equal(r["loglik"][d * S:(d + 1) * S], ref["loglik"]), (p.shape[1], d, n)
            assert torch.equal(r["trial_logp"][d * S:(d + 1) * S, :n], ref["trial_logp"]), (p.shape[1], d, n)
            pad = r["trial_logp"][d * S:(d + 1) * S, n:]
            assert bool((pad == 0).all()) and not bool(torch.signbit(pad).any()), (p.shape[1], d, n)
    # host-side counts take the same route
    h = engine.wiener_marginal_log_likelihood(engine.SINGLE_TRIAL, rows, data, draws_per_dataset=S, t_censor=TC, counts=np.asarray(COUNTS))
    assert torch.equal(h["loglik"], r["loglik"])


@pytest.mark.parametrize("S", [3, 17])
def test_without_counts_the_bits_are_the_plain_entry_points(S):
    torch = _torch()
    from bayesflow_nddms_amd import engine
    rows_np, data_np = _case(S, counts=(130, 130), n_pad=130)
    rows, data = torch.as_tensor(rows_np).cuda(), torch.as_tensor(data_np).cuda()
    assert not bool(torch.isnan(data).any())
    ref = engine.wiener_marginal_log_likelihood(engine.SINGLE_TRIAL, rows, data, draws_per_dataset=S, t_censor=TC, per_trial=True)
    out_t, out_s = torch.full_like(ref["trial_logp"], 7.0), torch.full_like(ref["loglik"], 7.0)
    assert _raw(torch, rows, 8, S, data, None, out_trial=out_t, out_sum=out_s) == 0
    assert torch.equal(out_t, ref["trial_logp"]) and torch.equal(out_s, ref["loglik"]) and torch.isfinite(out_s).all()
    # 7 columns: the 8-column row with a 1.0 column (the engine's route for [R, 7])
    assert bool((rows[:, 7] == 1.0).all())
    seven = engine.wiener_marginal_log_likelihood(engine.SINGLE_TRIAL, rows[:, :7].contiguous(), data, draws_per_dataset=S, t_censor=TC, per_trial=True)
    assert torch.equal(seven["trial_logp"], ref["trial_logp"]) and torch.equal(seven["loglik"], ref["loglik"])
    # and the gamma column is read when there are 8: another gamma, other bits
    other = rows.clone()
    other[:, 7] = 0.5
    out_o = torch.empty_like(out_s)
    assert _raw(torch, other, 8, S, data, None, out_sum=out_o) == 0
    assert torch.isfinite(out_o).all() and not torch.equal(out_o, out_s)


@pytest.mark.parametrize("S", [2, 16])
def test_an_invalid_count_gives_nan_in_its_own_set_only(S):
    torch = _torch()
    from bayesflow_nddms_amd import engine
    n_pad = 70
    counts = (0, 5, n_pad + 1, 70)
    rows_np, data_np = _case(S, counts=(0, 5, 0, 70), n_pad=n_pad)        # the invalid sets' data are all NaN: nothing of them is read
    rows, data = torch.as_tensor(rows_np).cuda(), torch.as_tensor(data_np).cuda()
    r = engine.wiener_marginal_log_likelihood(engine.SINGLE_TRIAL, rows, data, draws_per_dataset=S, t_censor=TC, per_trial=True,
                                              counts=torch.tensor(counts, dtype=torch.int32, device="cuda"))
    for d, n in enumerate(counts):
        s, t = r["loglik"][d * S:(d + 1) * S], r["trial_logp"][d * S:(d + 1) * S]
        if 1 <= n <= n_pad:
            ref = _plain(torch, rows, data, d, n, S)
            assert torch.equal(s, ref["loglik"]) and torch.equal(t[:, :n], ref["trial_logp"]) and bool((t[:, n:] == 0).all()), d
        else:
            assert bool(torch.isnan(s).all()) and bool(torch.isnan(t).all()), d


@pytest.mark.parametrize("S", [3, 17])
def test_nothing_is_written_outside_the_outputs(S):
    """Both outputs are views into sentinel-filled buffers with 4096-element guards: the guards are intact after the launch and every
    element of the outputs was written (the padding's zeros included)."""
    torch = _torch()
    rows_np, data_np = _case(S)
    rows, data = torch.as_tensor(rows_np[:, :7].copy()).cuda(), torch.as_tensor(data_np).cuda()
    counts = torch.tensor(COUNTS, dtype=torch.int32, device="cuda")
    R, G, sent = rows.shape[0], 4096, -12345.0
    big_t = torch.full((2 * G + R * N_PAD,), sent, device="cuda")
    big_s = torch.full((2 * G + R,), sent, dtype=torch.float64, device="cuda")
    assert _raw(torch, rows, 7, S, data, counts, out_trial=big_t[G:G + R * N_PAD], out_sum=big_s[G:G + R]) == 0
    torch.cuda.synchronize()
    for big, n in ((big_t, R * N_PAD), (big_s, R)):
        assert bool((big[:G] == sent).all()) and bool((big[G + n:] == sent).all())
        assert not bool((big[G:G + n] == sent).any())
    assert bool(torch.isfinite(big_s[G:G + R]).all())


def test_status_codes():
    torch = _torch()
    from bayesflow_nddms_amd import _lib
    rows_np, data_np = _case(2, counts=(5, 5), n_pad=5)
    rows, data = torch.as_tensor(rows_np).cuda(), torch.as_tensor(data_np).cuda()
    out = torch.full((rows.shape[0],), 3.0, dtype=torch.float64, device="cuda")
    assert _raw(torch, rows, 6, 2, data, None, out_sum=out) == _lib.NDDM_ERR_PARAM
    assert _raw(torch, rows, 9, 2, data, None, out_sum=out) == _lib.NDDM_ERR_PARAM
    assert _raw(torch, rows, 8, 2, data, None, flags=1, out_sum=out) == _lib.NDDM_ERR_PARAM
    assert b"param_cols" in _lib.lib().nddm_last_error()
    assert _raw(torch, rows, 8, 2, data, None, out_sum=out, R=0) == _lib.NDDM_OK
    assert _raw(torch, rows, 8, 2, data, None) == _lib.NDDM_ERR_NULL       # no output
    assert _raw(torch, rows, 8, 3, data, None, out_sum=out) == _lib.NDDM_ERR_SHAPE      # 4 rows, 3 per set
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())                                     # nothing launched
    assert _raw(torch, rows, 8, 2, data, None, out_sum=out) == _lib.NDDM_OK
    assert bool(torch.isfinite(out).all())
