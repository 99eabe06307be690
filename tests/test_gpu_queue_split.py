"""The two-ended chunk queue of the simulator kernels (csrc/nddm_queue.h, csrc/nddm_sim.h: open_tiles; nddm_set_queue_split): the last
waves of the grid pull their chunks from the back of the processing order.  The random stream is keyed by (set, trial), so WHO simulates a
set changes nothing: every launch here is compared, as 32-bit integers (the NaN positions count), with the same launch under
nddm_set_queue_split(0) -- small grids with many chunks, fewer chunks than waves, one and two chunks, sets split into tiles, trials that
reach the cap, repeated and captured launches (the queue words come back to zero), and the automatic rule."""
import numpy as np
import pytest

import prior_util

MODELS = {"basic": 0, "single": 1, "alpha_ns_bridge": 3, "explicit": 4}
GRID64 = (0, 0, 0, 0, 64, 0)                    # nddm_set_tuning: a grid of 64 waves, everything else by the library's rule


def _params(model, B, seed=41):
    if model == "basic":
        return prior_util.basic_prior(B, seed)
    if model == "single":
        return prior_util.single_prior(B, seed, gamma=1.0)
    if model == "alpha_ns_bridge":
        return prior_util.alpha_ns_prior(B, seed)
    return prior_util.basic_prior(B, seed)[:, [0, 2, 3, 4]]          # explicit boundary: drift, beta, ter, dc


class Knobs:
    """The developer knobs for the length of a `with`, back to the library's rules afterwards."""

    def __init__(self, tune=None):
        self.tune = tune

    def __enter__(self):
        from bayesflow_nddms_amd import _lib
        self.L = _lib.lib()
        if self.tune:
            _lib.check(self.L.nddm_set_tuning(*self.tune))
        return self

    def split(self, n):
        from bayesflow_nddms_amd import _lib
        _lib.check(self.L.nddm_set_queue_split(n))

    def __exit__(self, *exc):
        self.L.nddm_set_queue_split(-1)
        self.L.nddm_set_tuning(0, 0, 0, 0, 0, 0)
        return False


def _launch(model, p, N, bounds=None, **kw):
    """One launch -> (trials, summary, ext) as uint32 arrays, and its geometry."""
    from bayesflow_nddms_amd import engine
    g = engine.simulate(MODELS[model], p, N, seed=2020, set_offset=5, bounds=bounds, bridge=model == "alpha_ns_bridge",
                        ext_sigma=0.1, want_ext=model == "alpha_ns_bridge", **kw)
    out = [g["trials"].cpu().numpy().view(np.uint32), g["summary"].cpu().numpy().view(np.uint32)]
    if "ext" in g:
        out.append(g["ext"].cpu().numpy().view(np.uint32))
    return out, engine.last_launch()


def _same(a, b, what):
    for x, y in zip(a, b):
        assert x.shape == y.shape and np.array_equal(x, y), what


@pytest.mark.gpu
@pytest.mark.parametrize("N", [7, 300])
@pytest.mark.parametrize("model", list(MODELS))
def test_small_grid_many_chunks(model, N):
    B = 2049                                                         # >= 2048: a sorted launch
    p = _params(model, B)
    bounds = np.abs(np.random.default_rng(5).normal(1.2, 0.4, size=(B, N))).astype(np.float32) if model == "explicit" else None
    with Knobs(GRID64) as k:
        for fast in (True, False):
            kw = dict(dt=0.01, max_steps=400.0, fast=fast, bounds=bounds)
            k.split(0)
            ref, geo = _launch(model, p, N, **kw)
            assert geo["grid_waves"] == 64 and B * geo["tiles_per_set"] // geo["sets_per_chunk"] >= 4 * 64, geo
            for back in (16, 64):                                    # a quarter of the grid; every wave pulls from the back
                k.split(back)
                got, geo2 = _launch(model, p, N, **kw)
                assert geo2 == geo
                _same(got, ref, (model, N, fast, back))


@pytest.mark.gpu
def test_fewer_chunks_than_waves():
    p = _params("basic", 2049)
    with Knobs((64, 0, 0, 0, 64, 0)) as k:                           # 64 sets per chunk: 33 chunks, the last one of a single set
        for fast in (True, False):
            kw = dict(dt=0.01, max_steps=400.0, fast=fast)
            k.split(0)
            ref, geo = _launch("basic", p, 300, **kw)
            assert geo["sets_per_chunk"] == 64 and geo["tiles_per_set"] == 1 and geo["grid_waves"] == 33, geo
            k.split(16)
            _same(_launch("basic", p, 300, **kw)[0], ref, ("33 chunks", fast))


@pytest.mark.gpu
@pytest.mark.parametrize("B,n_chunks", [(3, 1), (5, 2)])
def test_one_and_two_chunks(B, n_chunks):
    """Unsorted launches (B < 2048) with the split forced on by the knob: the last wave of a grid of at most 4 pulls from the back."""
    p = _params("basic", B)
    with Knobs((3, 0, 0, 0, 4, 300)) as k:                           # 3 sets per chunk, a grid of 4 waves, one tile per set
        for fast in (True, False):
            kw = dict(dt=0.01, max_steps=400.0, fast=fast)
            k.split(0)
            ref, geo = _launch("basic", p, 300, **kw)
            assert geo["sets_per_chunk"] == 3 and geo["tiles_per_set"] == 1 and geo["grid_waves"] == n_chunks, geo
            k.split(1)
            _same(_launch("basic", p, 300, **kw)[0], ref, (B, fast))


@pytest.mark.gpu
def test_split_sets():
    p = _params("basic", 2100)
    with Knobs(GRID64) as k:
        for fast in (True, False):
            kw = dict(dt=0.01, max_steps=400.0, fast=fast)
            k.split(0)
            ref, geo = _launch("basic", p, 1300, **kw)
            assert geo["tiles_per_set"] == 3 and geo["grid_waves"] == 64, geo
            k.split(16)
            _same(_launch("basic", p, 1300, **kw)[0], ref, ("three tiles per set", fast))


@pytest.mark.gpu
def test_cap_reached():
    p = _params("basic", 2049)
    with Knobs(GRID64) as k:
        for fast in (True, False):
            kw = dict(dt=0.001, max_steps=4000.0, fast=fast)
            k.split(0)
            ref, geo = _launch("basic", p, 64, **kw)
            assert geo["grid_waves"] == 64, geo
            timeouts = int((ref[0][..., 1] == 0).sum())               # choice 0.0: the trial ran to the cap
            print(f"fast={fast}: {timeouts} of {ref[0].shape[0] * ref[0].shape[1]} trials reach the cap")
            assert timeouts > 100
            k.split(16)
            _same(_launch("basic", p, 64, **kw)[0], ref, ("cap 4000", fast))


@pytest.mark.gpu
def test_repeat_launches_and_a_replayed_graph():
    """The queue words -- the 64-bit (front, back) pair and the exit counter -- are zero again after every launch: a second launch on the
    same stream, and a captured launch replayed twice, reproduce the split-off result."""
    import torch
    from bayesflow_nddms_amd import engine
    B, N = 2049, 100
    p = torch.as_tensor(_params("basic", B)).cuda()
    out = torch.empty((B, N, 2), device="cuda")
    summ = torch.empty((B, 10), device="cuda")
    kw = dict(dt=0.01, max_steps=400.0, seed=3, set_offset=7, fast=True, out_trials=out, out_summary=summ)

    def bits():
        torch.cuda.synchronize()
        return out.cpu().numpy().view(np.uint32).copy(), summ.cpu().numpy().view(np.uint32).copy()

    with Knobs(GRID64) as k:
        k.split(0)
        engine.simulate(engine.BASIC_DDM_DC, p, N, **kw)
        ref = bits()
        k.split(16)
        for launch in range(2):                                      # back to back on one stream
            out.zero_(); summ.fill_(-7.0)
            engine.simulate(engine.BASIC_DDM_DC, p, N, **kw)
            if launch == 0:
                first = (out.clone(), summ.clone())                  # (stream-ordered copies: no synchronisation between the two launches)
        _same(bits(), ref, "second launch")
        torch.cuda.synchronize()
        _same((first[0].cpu().numpy().view(np.uint32), first[1].cpu().numpy().view(np.uint32)), ref, "first launch")
        g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        with torch.cuda.stream(side):
            engine.simulate(engine.BASIC_DDM_DC, p, N, **kw)
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=side):
                engine.simulate(engine.BASIC_DDM_DC, p, N, **kw)
        for replay in range(2):
            out.zero_(); summ.fill_(-7.0)
            g.replay()
            _same(bits(), ref, ("replay", replay))
        del g
        engine.release_graph_memory()


def _pull_ticks(p, N, **kw):
    """The tick at which each chunk of one launch was pulled (nddm_set_debug_trace), by chunk id."""
    import torch
    from bayesflow_nddms_amd import engine
    with engine.debug_trace(waves=16384, chunks=1 << 16) as tr:
        engine.simulate(engine.BASIC_DDM_DC, p, N, **kw)
    geo = engine.last_launch()
    n_chunks = -(-p.shape[0] * geo["tiles_per_set"] // geo["sets_per_chunk"])
    assert n_chunks <= 1 << 16
    ticks = tr.buf.cpu().numpy()[8 * 16384:][:n_chunks]
    assert (ticks > 0).all()
    return ticks - ticks.min(), geo


@pytest.mark.gpu
def test_the_automatic_rule_is_off_on_a_cut_grid_and_comes_back_after_a_forced_value():
    """4096 x 300 is a sorted launch, but its grid is cut: every wave pulls from the front, so the chunks are pulled in the order of their
    ids and the last chunk of the queue is pulled last.  With the split forced on, the last chunk is the first one a back wave pulls, at the
    start of the launch.  nddm_set_queue_split(-1) then restores the rule."""
    import torch
    p = torch.as_tensor(_params("basic", 4096)).cuda()
    kw = dict(dt=0.01, max_steps=400.0, seed=9, set_offset=0, fast=True)
    with Knobs() as k:
        for split, back_first in ((-1, False), (16, True), (-1, False)):
            k.split(split)
            ticks, geo = _pull_ticks(p, 300, **kw)
            assert geo["grid_waves"] < 8192 and len(ticks) > 2 * geo["grid_waves"], geo
            mid, last = int(ticks[3 * len(ticks) // 4]), int(ticks[-1])
            print(f"split {split}: grid {geo['grid_waves']}, {len(ticks)} chunks, chunk at 3/4 of the queue pulled at tick {mid}, last chunk at {last}")
            assert (last < mid) == back_first, (split, mid, last)
