"""The shared front end of engine.py's entry points (simulate, simulratcliff, simulate_to_host, wiener_log_likelihood): parameter
ingestion, stream position and output buffers.  The CPU cases pin the private helpers; the GPU cases pin what the public calls do
with them -- the same bits from every representation of the same parameters, one take() per call, the order of the checks, and
caller-supplied buffers that are either used as they are or refused untouched."""
import re

import numpy as np
import pytest
import torch

from bayesflow_nddms_amd import engine

gpu = pytest.mark.gpu

B, N_TRIALS, DT, MAX_STEPS = 3, 5, .01, 400
# every value is a float32, so the float64 forms hold the same numbers
P_BASIC = np.array([[1.5, 1.2, .5, .35, 1.0], [-.75, .9, .4, .2, 1.1], [.25, 1.6, .6, .5, .8]], dtype=np.float32)
P_RATCLIFF = np.array([[1.0, 1.2, .5, .4, .3, 1.0], [-2.0, .9, .4, .2, 0.0, 1.1], [.5, 1.3, .6, .3, 1.5, .9]], dtype=np.float32)
LL_R, LL_D, LL_N = 4, 2, 3
P_LL = np.array([[1.5, 1.2, .5, .25, 1.0], [-.75, .9, .4, .125, 1.1], [.25, 1.6, .6, .25, .8], [2.0, 1.0, .5, .125, 1.0]], dtype=np.float32)
D_LL = np.array([[[.6, 1.0], [.7, -1.0], [.9, 0.0]], [[.45, -1.0], [1.2, 1.0], [.5, 1.0]]], dtype=np.float32)


# ---------------------------------------------------------------- CPU: the helpers

# (columns, the text the caller hands over): simulate / simulate_to_host, simulratcliff, wiener_log_likelihood
ROW_LABELS = [(5, "params must have shape [B, 5] for this model"), (8, "params must have shape [B, 8] for this model"),
              (6, "params must have shape [B, 6] (Nu, Alpha, Beta, Tau, Eta, Varsigma)"), (6, "params must have shape [R, 6]")]
DATA_ROWS = (3, 2, "data must have shape [D, n_trials, 2]")


def test_host_rows_promote_a_single_row_and_give_the_same_float64_from_every_host_form():
    spec = engine._SIM_ROWS[engine.BASIC_DDM_DC]
    one = engine._host_rows(P_BASIC[0], *spec)
    assert one.shape == (1, 5) and one.dtype == np.float64 and np.array_equal(one, P_BASIC[:1].astype(np.float64))
    want = P_BASIC.astype(np.float64)
    for form in (P_BASIC, want.tolist(), torch.from_numpy(P_BASIC), torch.from_numpy(want), np.asfortranarray(want)):
        got = engine._host_rows(form, *spec)
        assert got.dtype == np.float64 and got.shape == (3, 5) and got.flags.c_contiguous and np.array_equal(got, want)
    # the upload of host rows is float32 and contiguous (the CPU stands in for the device)
    up = engine._device_rows(None, want, torch.device("cpu"), *spec)
    assert up.dtype == torch.float32 and up.is_contiguous() and np.array_equal(up.numpy(), P_BASIC)


@pytest.mark.parametrize("cols,text", ROW_LABELS, ids=[t for _, t in ROW_LABELS])
def test_rows_refuse_other_shapes_with_the_callers_text(cols, text):
    spec = (2, cols, text)
    assert engine._SIM_ROWS[engine.BASIC_DDM_DC] == (2,) + ROW_LABELS[0] and engine._SIM_ROWS[engine.SINGLE_TRIAL_ALT] == (2,) + ROW_LABELS[1]
    for bad in (np.ones((3, cols - 1)), np.ones((2, 2, cols)), torch.ones(3, cols - 1)):
        with pytest.raises(ValueError, match=re.escape(f"{text}, got {tuple(bad.shape)}")):
            engine._host_rows(bad, *spec)
        if isinstance(bad, torch.Tensor):         # the same refusal where the tensor is the device's (the CPU stands in)
            with pytest.raises(ValueError, match=re.escape(f"{text}, got {tuple(bad.shape)}")):
                engine._device_rows(bad, None, torch.device("cpu"), *spec)
    one = engine._device_rows(torch.ones(cols, dtype=torch.float64), None, torch.device("cpu"), *spec)
    assert one.shape == (1, cols) and one.dtype == torch.float32 and one.is_contiguous()


def test_host_rows_of_likelihood_data():
    spec = DATA_ROWS
    assert engine._host_rows(D_LL[0], *spec).shape == (1, LL_N, 2)
    assert np.array_equal(engine._host_rows(torch.from_numpy(D_LL), *spec), D_LL.astype(np.float64))
    for bad in (np.zeros((1, 3, 3)), np.zeros((2, 0, 2)), np.zeros((2, 2, 3, 2))):
        with pytest.raises(ValueError, match=re.escape(f"data must have shape [D, n_trials, 2], got {bad.shape}")):
            engine._host_rows(bad, *spec)
    assert engine._host_rows(np.zeros((0, 3, 2)), *spec).shape == (0, 3, 2)          # no data sets is a shape, no trials is not


@pytest.mark.parametrize("seed,set_offset,n_sets,want,after", [
    (5, 9, 4, (5, 9), 100),                       # both given: the state is not touched
    (5, None, 4, (5, 100), 104),                  # the offset is taken
    (None, 9, 4, (7, 9), 104),                    # the seed is taken, and the stream still moves on
    (None, None, 4, (7, 100), 104),
    (None, None, 0, (7, 100), 100),               # an empty batch takes nothing, but asks
    (-1, 9, 4, (2 ** 64 - 1, 9), 100),
    (5, -2, 4, (5, 2 ** 64 - 2), 100),
])
def test_stream_position(seed, set_offset, n_sets, want, after):
    class Counting(engine.StreamState):
        takes = 0

        def take(self, n):
            self.takes += 1
            return super().take(n)

    st = Counting(seed=7, offset=100)
    assert engine._stream_position(seed, set_offset, st, n_sets) == want
    assert st.offset == after and st.seed == 7
    assert st.takes == (1 if seed is None or set_offset is None else 0)


def test_stream_position_falls_back_to_the_package_stream():
    saved = engine.GLOBAL_STREAM.get_state()
    try:
        engine.seed(3)
        assert engine._stream_position(None, None, None, 6) == (3, 0)
        assert engine._stream_position(None, None, None, 1) == (3, 6)
        assert engine._u64(2 ** 64 + 5) == 5 and engine._u64(np.int64(-1)) == 2 ** 64 - 1
    finally:
        engine.GLOBAL_STREAM.set_state(saved)


def test_out_buffer_allocates_when_wanted_and_refuses_what_it_cannot_use():
    cpu = torch.device("cpu")
    assert engine._out_buffer(False, None, (3, 10), cpu) is None
    made = engine._out_buffer(True, None, (3, 5, 2), cpu)
    assert tuple(made.shape) == (3, 5, 2) and made.dtype == torch.float32 and made.is_contiguous()
    # a host tensor is never a valid output buffer, so each of these is refused (for its own fault as well); the device cases below
    # separate the faults
    text = re.escape("output buffer must be a contiguous float32 device tensor of shape (3, 5, 2)")
    for bad in (torch.zeros(3, 5, 3), torch.zeros(3, 5, 2, dtype=torch.float64), torch.zeros(3, 5, 4)[..., :2], torch.zeros(3, 5, 2)):
        for want in (True, False):                # a buffer that was handed in is checked whether or not the output is "wanted"
            with pytest.raises(ValueError, match=text):
                engine._out_buffer(want, bad, (3, 5, 2), cpu)


# ---------------------------------------------------------------- GPU: the public calls

def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def _same(a, b):
    """Every tensor of two result dicts byte for byte (NaN summaries included), every other entry by value."""
    assert list(a) == list(b)
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(_bits(a[k]), _bits(b[k])), k
        else:
            assert a[k] == b[k], k


def _forms(p32):
    return [p32.astype(np.float64), p32, torch.from_numpy(p32.copy()), torch.from_numpy(p32.copy()).cuda()]


@gpu
def test_simulate_gives_the_same_bits_from_every_representation():
    run = lambda p: engine.simulate(engine.BASIC_DDM_DC, p, N_TRIALS, dt=DT, max_steps=MAX_STEPS, seed=11, set_offset=2)
    ref = run(_forms(P_BASIC)[0])
    assert list(ref) == ["seed", "set_offset", "params", "trials", "summary"]
    assert ref["trials"].shape == (B, N_TRIALS, 2) and ref["summary"].shape == (B, 10) and ref["params"].dtype == torch.float32
    for form in _forms(P_BASIC)[1:] + [torch.from_numpy(P_BASIC.astype(np.float64)).cuda()]:
        _same(ref, run(form))
    _same(run(P_BASIC[:1]), run(P_BASIC[0]))
    _same(run(torch.from_numpy(P_BASIC[:1].copy()).cuda()), run(torch.from_numpy(P_BASIC[0].copy()).cuda()))
    _same(run(P_BASIC[:1]), run(torch.from_numpy(P_BASIC[0].copy()).cuda()))


@gpu
def test_simulratcliff_gives_the_same_bits_from_every_representation():
    run = lambda p: engine.simulratcliff(p, N_TRIALS, seed=11, set_offset=2, want_ext=True)
    ref = run(_forms(P_RATCLIFF)[0])
    assert list(ref) == ["seed", "set_offset", "params", "trials", "summary", "ext"]
    assert ref["trials"].shape == (B, N_TRIALS, 2) and ref["summary"].shape == (B, 10) and ref["ext"].shape == (B,)
    for form in _forms(P_RATCLIFF)[1:]:
        _same(ref, run(form))
    _same(run(P_RATCLIFF[:1]), run(P_RATCLIFF[0]))
    _same(run(P_RATCLIFF[:1]), run(torch.from_numpy(P_RATCLIFF[0].copy()).cuda()))


@gpu
def test_wiener_log_likelihood_gives_the_same_bits_from_every_representation():
    run = lambda p, d: engine.wiener_log_likelihood(engine.BASIC_DDM_DC, p, d, draws_per_dataset=LL_R // LL_D, per_trial=True)
    ref = run(_forms(P_LL)[0], _forms(D_LL)[0])
    assert list(ref) == ["loglik", "trial_logp"]
    assert ref["loglik"].shape == (LL_R,) and ref["loglik"].dtype == torch.float64 and ref["trial_logp"].shape == (LL_R, LL_N)
    assert bool(torch.isfinite(ref["loglik"]).all())
    for p, d in zip(_forms(P_LL)[1:], _forms(D_LL)[1:]):
        _same(ref, run(p, d))
    _same(ref, run(_forms(P_LL)[3], _forms(D_LL)[0]))                  # device parameters against host data, and the other way round
    _same(ref, run(_forms(P_LL)[0], _forms(D_LL)[3]))
    one = lambda p, d: engine.wiener_log_likelihood(engine.BASIC_DDM_DC, p, d, per_trial=True)
    _same(one(P_LL[:1], D_LL[:1]), one(P_LL[0], D_LL[0]))
    _same(one(P_LL[:1], D_LL[:1]), one(torch.from_numpy(P_LL[0].copy()).cuda(), torch.from_numpy(D_LL[0].copy()).cuda()))


def _calls():
    return [("simulate", lambda **kw: engine.simulate(engine.BASIC_DDM_DC, P_BASIC, N_TRIALS, dt=DT, max_steps=MAX_STEPS, **kw)),
            ("simulratcliff", lambda **kw: engine.simulratcliff(P_RATCLIFF, N_TRIALS, **kw)),
            ("simulate_to_host", lambda **kw: engine.simulate_to_host(engine.BASIC_DDM_DC, P_BASIC, N_TRIALS, dt=DT, max_steps=MAX_STEPS, **kw)),
            # one parameter set per chunk: the batch still takes its position once, and the chunks are handed theirs
            ("simulate_to_host chunked", lambda **kw: engine.simulate_to_host(engine.BASIC_DDM_DC, P_BASIC, N_TRIALS, dt=DT, max_steps=MAX_STEPS,
                                                                                chunk_bytes=8 * N_TRIALS, **kw))]


@gpu
@pytest.mark.parametrize("name", [n for n, _ in _calls()])
def test_public_calls_take_their_stream_position_once(name):
    call = dict(_calls())[name]
    st = engine.StreamState(seed=7)
    glob = engine.GLOBAL_STREAM.get_state()
    r0 = call(stream_state=st)
    assert (r0["seed"], r0["set_offset"], st.offset) == (7, 0, B)
    r1 = call(stream_state=st)
    assert (r1["seed"], r1["set_offset"], st.offset) == (7, B, 2 * B)
    r2 = call(stream_state=st, seed=9, set_offset=B)                   # both given: nothing is taken
    assert (r2["seed"], r2["set_offset"], st.offset) == (9, B, 2 * B)
    r3 = call(stream_state=st, seed=9)                                 # one given: the other is taken, the stream moves on
    assert (r3["seed"], r3["set_offset"], st.offset) == (9, 2 * B, 3 * B)
    r4 = call(stream_state=st, set_offset=B)
    assert (r4["seed"], r4["set_offset"], st.offset) == (7, B, 4 * B)
    assert np.array_equal(np.asarray(engine.to_host(r1["trials"])), np.asarray(engine.to_host(r4["trials"])))      # same position, same trials
    assert not np.array_equal(np.asarray(engine.to_host(r0["trials"])), np.asarray(engine.to_host(r1["trials"])))
    r5 = call(stream_state=st, seed=-1, set_offset=2 ** 60 - B)        # the seed wraps to uint64; the library keys 60 bits of the set index
    assert (r5["seed"], r5["set_offset"], st.offset) == (2 ** 64 - 1, 2 ** 60 - B, 4 * B)
    assert engine.GLOBAL_STREAM.get_state() == glob                    # a private state keeps the package stream out of it


@gpu
def test_chunked_host_results_equal_the_one_launch():
    one, chunked = dict(_calls())["simulate_to_host"], dict(_calls())["simulate_to_host chunked"]
    a, b = one(seed=3, set_offset=2 ** 60 - B), chunked(seed=3, set_offset=2 ** 60 - B)      # the last set index the library takes
    assert list(a) == list(b) == ["seed", "set_offset", "trials", "summary"]
    assert np.array_equal(a["trials"].view(np.uint32), b["trials"].view(np.uint32))
    assert np.array_equal(a["summary"].view(np.uint32), b["summary"].view(np.uint32))


@gpu
def test_a_refusal_after_the_position_was_taken_has_moved_the_stream_and_one_before_has_not():
    st = engine.StreamState(seed=7)
    with pytest.raises(ValueError, match="n_trials must be positive"):
        engine.simulate(engine.BASIC_DDM_DC, P_BASIC, 0, stream_state=st)
    with pytest.raises(ValueError, match="n_trials must be positive"):
        engine.simulratcliff(P_RATCLIFF, 0, stream_state=st)
    assert st.offset == 0
    with pytest.raises(ValueError, match="Brownian-bridge"):
        engine.simulate(engine.BASIC_DDM_DC, P_BASIC, N_TRIALS, dt=DT, max_steps=MAX_STEPS, bridge=True, stream_state=st)
    assert st.offset == B
    with pytest.raises(ValueError, match="output buffer"):
        engine.simulate(engine.BASIC_DDM_DC, P_BASIC, N_TRIALS, dt=DT, max_steps=MAX_STEPS, stream_state=st,
                        out_trials=torch.empty((B, N_TRIALS, 3), device="cuda"))
    assert st.offset == 2 * B


@gpu
def test_order_of_checks():
    bad = P_BASIC.copy()
    bad[1, 1] = -1.0                                                   # a boundary below zero
    with pytest.raises(ValueError, match=r"\[B, 5\]"):
        engine.simulate(engine.BASIC_DDM_DC, bad[:, :4], 0, dt=-1)
    with pytest.raises(ValueError, match="parameter column 1"):
        engine.simulate(engine.BASIC_DDM_DC, bad, 0, dt=-1)
    with pytest.raises(ValueError, match="n_trials must be positive"):
        engine.simulate(engine.BASIC_DDM_DC, P_BASIC, 0, dt=-1)
    with pytest.raises(ValueError, match="dt must be finite"):
        engine.simulate(engine.BASIC_DDM_DC, P_BASIC, N_TRIALS, dt=-1, max_steps=-3)
    with pytest.raises(ValueError, match="max_steps"):
        engine.simulate(engine.EXPLICIT_BOUNDARY, P_BASIC[:, :4], N_TRIALS, dt=DT, max_steps=-3)
    with pytest.raises(ValueError, match="needs `bounds`"):
        engine.simulate(engine.EXPLICIT_BOUNDARY, P_BASIC[:, :4], N_TRIALS, dt=DT, bridge=True)
    with pytest.raises(ValueError, match="Brownian-bridge"):
        engine.simulate(engine.BASIC_DDM_DC, P_BASIC, N_TRIALS, dt=DT, bridge=True, out_codes=torch.empty((1, 1), device="cuda"))
    with pytest.raises(ValueError, match="out_codes"):
        engine.simulate(engine.BASIC_DDM_DC, P_BASIC, N_TRIALS, dt=DT, out_codes=torch.empty((1, 1), device="cuda"),
                        out_trials=torch.empty((1, 1), device="cuda"))
    with pytest.raises(ValueError, match="output buffer"):
        engine.simulate(engine.BASIC_DDM_DC, P_BASIC, N_TRIALS, dt=DT, out_trials=torch.empty((1, 1), device="cuda"),
                        set_offset_dev=torch.zeros(1, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="set_offset_dev"):
        engine.simulate(engine.BASIC_DDM_DC, P_BASIC, N_TRIALS, dt=DT, set_offset_dev=torch.zeros(1, dtype=torch.int32, device="cuda"))
    for wrong in (P_RATCLIFF[:, :5], torch.from_numpy(P_RATCLIFF[:, :5].copy()).cuda()):      # host and device rows are refused alike
        with pytest.raises(ValueError, match=r"\[B, 6\]"):
            engine.simulratcliff(wrong, 0)
        with pytest.raises(ValueError, match=r"\[B, 8\] for this model"):
            engine.simulate_to_host(engine.SINGLE_TRIAL, wrong, 0)
    # Beta / Eta ranges of the exact sampler come after the common value checks and before n_trials
    rat = P_RATCLIFF.copy()
    rat[0, 2], rat[1, 1] = 1.5, -1.0
    with pytest.raises(ValueError, match="parameter column 1"):
        engine.simulratcliff(rat, 0)
    rat[1, 1] = 1.0
    with pytest.raises(ValueError, match="Beta must lie"):
        engine.simulratcliff(rat, 0)
    # the likelihood: model, then parameters, then data, then the split
    with pytest.raises(ValueError, match="closed-form"):
        engine.wiener_log_likelihood(engine.SINGLE_TRIAL, P_LL[:, :3], np.zeros((1, 3, 3)))
    badp = P_LL.copy()
    badp[0, 2] = 1.0
    with pytest.raises(ValueError, match=r"\(0, 1\)"):
        engine.wiener_log_likelihood(engine.BASIC_DDM_DC, badp, np.zeros((1, 3, 3)))
    with pytest.raises(ValueError, match=r"\[D, n_trials, 2\]"):
        engine.wiener_log_likelihood(engine.BASIC_DDM_DC, P_LL, np.zeros((3, 3, 3)))
    with pytest.raises(ValueError, match="data sets"):
        engine.wiener_log_likelihood(engine.BASIC_DDM_DC, torch.from_numpy(P_LL[:3].copy()).cuda(), D_LL)


@gpu
@pytest.mark.parametrize("name", ["simulate", "simulratcliff"])
def test_caller_supplied_buffers_are_used_or_refused_untouched(name):
    call = dict(_calls())[name]
    tr, sm = torch.full((B, N_TRIALS, 2), 7.0, device="cuda"), torch.full((B, 10), 7.0, device="cuda")
    r = call(seed=1, set_offset=0, out_trials=tr, out_summary=sm)
    assert r["trials"] is tr and r["summary"] is sm
    _same(r, call(seed=1, set_offset=0))
    only = call(seed=1, set_offset=0, want_trials=False, want_summary=False, out_summary=sm)      # a buffer handed in is an output asked for
    assert "trials" not in only and only["summary"] is sm
    base = torch.full((B, N_TRIALS, 4), 7.0, device="cuda")
    for key, bad in (("out_trials", torch.full((B, N_TRIALS + 1, 2), 7.0, device="cuda")),
                     ("out_trials", torch.full((B, N_TRIALS, 2), 7.0, dtype=torch.float64, device="cuda")),
                     ("out_trials", base[..., :2]),
                     ("out_trials", torch.full((B, N_TRIALS, 2), 7.0)),
                     ("out_summary", torch.full((B, 9), 7.0, device="cuda")),
                     ("out_summary", torch.full((B, 10), 7.0, dtype=torch.float64, device="cuda"))):
        before = bad.clone()
        with pytest.raises(ValueError, match="output buffer must be a contiguous float32 device tensor of shape"):
            call(seed=1, set_offset=0, **{key: bad})
        assert torch.equal(bad, before)
    assert bool((base == 7.0).all())


@gpu
@pytest.mark.parametrize("fast", [False, True])
def test_the_wire_format_launch_returns_a_written_external_datum(fast):
    """nddm_simulate_codes has no output for alpha_not_scaled's per-set external datum; simulate(want_codes=True, want_ext=True) fills it
    with a launch of its own (one step-less trial per set).  The datum is the one a plain launch writes, bit for bit -- with and without
    the float pairs, with a device-resident part of the set offset -- and, in exact mode, the oracle's; the launch that last_launch()
    describes is the one that simulated."""
    import oracle
    p = np.concatenate([P_RATCLIFF] * 40)
    nb, n = len(p), 70
    kw = dict(dt=DT, max_steps=MAX_STEPS, seed=11, fast=fast, ext_sigma=0.25, ext_mode=0, want_ext=True)
    plain = engine.simulate(engine.ALPHA_NOT_SCALED, p, n, set_offset=(1 << 34) + 5, **kw)
    engine.simulate(engine.ALPHA_NOT_SCALED, p, n, set_offset=(1 << 34) + 5, want_codes=True, **dict(kw, want_ext=False))
    geo = engine.last_launch()
    both = engine.simulate(engine.ALPHA_NOT_SCALED, p, n, set_offset=(1 << 34) + 5, want_codes=True, **kw)
    assert engine.last_launch() == geo
    only = engine.simulate(engine.ALPHA_NOT_SCALED, p, n, set_offset=(1 << 34) + 5, want_codes=True, want_trials=False, want_summary=False, **kw)
    off = torch.tensor([1 << 34], dtype=torch.int64, device="cuda")
    ind = engine.simulate(engine.ALPHA_NOT_SCALED, p, n, set_offset=5, set_offset_dev=off, want_codes=True, **kw)
    for r in (both, only, ind):
        assert r["ext"].shape == (nb,) and torch.equal(r["ext"].view(torch.int32), plain["ext"].view(torch.int32))
        assert torch.equal(r["codes"], both["codes"])
    assert torch.equal(both["trials"], plain["trials"])
    mode1 = engine.simulate(engine.ALPHA_NOT_SCALED, p, n, set_offset=3, want_codes=True, **dict(kw, ext_mode=1))
    assert torch.equal(mode1["ext"], engine.simulate(engine.ALPHA_NOT_SCALED, p, n, set_offset=3, **dict(kw, ext_mode=1))["ext"])
    if not fast:
        o = oracle.philox_simulate(oracle.M_ALPHA_NS, p, n, dt=DT, max_steps=MAX_STEPS, seed=11, set_offset=(1 << 34) + 5, ext_sigma=0.25,
                                   ext_mode=0, want_ext=True, want_trials=False, want_summary=False)
        assert np.array_equal(both["ext"].cpu().numpy().view(np.uint32), o["ext"].view(np.uint32))
    basic = engine.simulate(engine.BASIC_DDM_DC, P_BASIC, n, dt=DT, max_steps=MAX_STEPS, seed=1, set_offset=0, want_codes=True, want_ext=True)
    assert "ext" not in basic                       # (a model without the datum: nothing to fill, nothing returned)


@gpu
def test_an_empty_batch_returns_empty_tensors_and_launches_nothing():
    engine.simulate(engine.BASIC_DDM_DC, P_BASIC, N_TRIALS, dt=DT, max_steps=MAX_STEPS, seed=1, set_offset=0)
    last = engine.last_launch()
    st = engine.StreamState(seed=7, offset=5)
    r = engine.simulate(engine.ALPHA_NOT_SCALED, np.zeros((0, 6)), N_TRIALS, dt=DT, max_steps=MAX_STEPS, want_ext=True, want_codes=True, stream_state=st)
    assert engine.last_launch() == last
    assert list(r) == ["seed", "set_offset", "params", "trials", "summary", "ext", "codes"]
    assert (r["seed"], r["set_offset"], st.offset) == (7, 5, 5)
    assert r["params"].shape == (0, 6) and r["trials"].shape == (0, N_TRIALS, 2) and r["summary"].shape == (0, 10)
    assert r["ext"].shape == (0,) and r["codes"].shape == (0, N_TRIALS) and r["codes"].dtype == torch.int16
    r = engine.simulate(engine.BASIC_DDM_DC, torch.zeros((0, 5), device="cuda"), N_TRIALS, dt=DT, max_steps=MAX_STEPS, stream_state=st)
    assert engine.last_launch() == last and r["trials"].shape == (0, N_TRIALS, 2) and r["trials"].is_cuda and st.offset == 5
    r = engine.simulratcliff(np.zeros((0, 6)), N_TRIALS, want_ext=True, stream_state=st)
    assert engine.last_launch() == last
    assert r["trials"].shape == (0, N_TRIALS, 2) and r["summary"].shape == (0, 10) and r["ext"].shape == (0,) and st.offset == 5
    h = engine.simulate_to_host(engine.BASIC_DDM_DC, np.zeros((0, 5)), N_TRIALS, dt=DT, max_steps=MAX_STEPS, stream_state=st)
    assert h["trials"].shape == (0, N_TRIALS, 2) and h["summary"].shape == (0, 10) and st.offset == 5
    ll = engine.wiener_log_likelihood(engine.BASIC_DDM_DC, np.zeros((0, 5)), np.zeros((0, LL_N, 2)), per_trial=True)
    assert ll["loglik"].shape == (0,) and ll["trial_logp"].shape == (0, LL_N)
