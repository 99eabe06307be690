"""The step counter of the CAP4 step block (csrc/nddm_sim.h): k is counted two steps at a time and corrected for the lanes that
leave at an odd step, and the step cap is tested only in a refill phase in which a lane can reach it (within 16 blocks = 64
steps of the cap).  k IS the response time, so every mistake there shows as a trial off by one step, or as a trial that runs
past the cap.

Exact transform: bit for bit against oracle.philox_simulate, on a parameter mixture in which trials end at every step
residue mod 4 and a visible share runs to the cap (both asserted from the oracle's output, so the comparison cannot pass
vacuously), for caps on both sides of the near-cap rule and for the refill thresholds that change how long a phase is.

Fast transform: tests/golden/fast_steps_parent.npz holds the 2-byte result codes (step index | choice << 14, uint16 [256, 300])
that the library built from commit 11ecea7 ("Add a batched Wiener first-passage log-likelihood kernel (dwiener)": the last
one with one increment per step and the cap test after every block) wrote on an MI355X for basic_prior(256, 2023), dt = .001,
4000 steps, seed 2023, set_offset 0; the counter does not touch arithmetic, so the codes must be reproduced exactly."""
import os

import numpy as np
import pytest

import prior_util

MODELS = {"basic": 0, "single": 1}
CAPS = [4, 8, 60, 64, 68, 128, 400, 4000]
# refill thresholds (nddm_set_tuning): the library's rule, 1, 8, and lockstep (>= 64: a phase has no bound, the cap test stays on)
THRESHOLDS = [0, 1, 8, 64]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fast_steps_parent.npz")


def _dt(cap):
    return 0.001 if cap > 400 else 0.01


def mixture(model, B=96):
    """A third of the rows from the prior, a third with boundaries of a few single-step standard deviations (trials of 1 .. ~20
    steps: every residue mod 4, also under a cap of 4), a third that cannot reach its boundary before any of the caps."""
    p = (prior_util.basic_prior(B, 77) if model == "basic" else prior_util.single_prior(B, 77, gamma=1.0)).copy()
    short, never = np.arange(B) % 3 == 1, np.arange(B) % 3 == 2
    n_s, n_n = int(short.sum()), int(never.sum())
    dc = 5 if model == "single" else 4
    p[short, 0] = np.linspace(-2.0, 2.0, n_s)                  # drift
    p[short, 1] = np.linspace(0.03, 0.6, n_s)                  # boundary (single: its mean)
    p[short, 2] = 0.5
    p[short, dc] = np.linspace(0.8, 2.0, n_s)
    p[never, 0] = np.linspace(-0.05, 0.05, n_n)
    p[never, 1] = 8.0
    p[never, 2] = 0.5
    p[never, dc] = 0.1
    if model == "single":
        p[short, 4] = 0.01                                     # std_alpha
        p[never, 4] = 0.1
    return np.ascontiguousarray(p, dtype=np.float32)


def reference(model, cap, N=300, B=96):
    """The oracle's output on the mixture, with the coverage the comparison relies on asserted from it."""
    import oracle
    p = mixture(model, B)
    o = oracle.philox_simulate(MODELS[model], p, N, dt=_dt(cap), max_steps=float(cap), seed=2023, set_offset=11, want_k=True, threads=8)
    k = o["k"]
    # (a trial that ran to the cap: choice 0 of the basic model's (rt, choice), choicert 0 of the single-trial model's (choicert, z1))
    timeout = o["trials"][..., 1 if model == "basic" else 0] == 0
    capped, ended = (k == cap) & timeout, ~timeout
    assert k.max() == cap and capped.mean() > 0.05, (cap, k.max(), capped.mean())
    res = np.bincount(k[ended] % 4, minlength=4)
    # (under a cap of 4 a residue is one single step; 30 trials of 28,800 is what "every residue" asks)
    assert res.min() >= 30, (cap, res)
    return p, o


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("cap", CAPS)
def test_mixture_covers_every_residue_and_the_cap(model, cap, oracle_mod):
    """The reference side alone (no GPU): the mixture ends trials at every residue and at the cap, for every cap of the list."""
    reference(model, cap)


@pytest.mark.gpu
@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("cap", CAPS)
def test_step_count_bit_parity(model, cap, oracle_mod):
    from bayesflow_nddms_amd import _lib, engine
    p, o = reference(model, cap)
    try:
        for thresh in THRESHOLDS:
            _lib.check(_lib.lib().nddm_set_tuning(0, 0, thresh, 0, 0, 0))
            g = engine.simulate(MODELS[model], p, 300, dt=_dt(cap), max_steps=float(cap), seed=2023, set_offset=11, fast=False)
            t = g["trials"].cpu().numpy()
            same = t.view(np.uint32) == o["trials"].view(np.uint32)
            print(f"{model} cap {cap} threshold {thresh}: {int((~same.all(axis=-1)).sum())} of {same.shape[0] * same.shape[1]} trials differ")
            assert same.all(), (model, cap, thresh)
            gs = g["summary"].cpu().numpy()
            assert np.array_equal(np.nan_to_num(gs).view(np.uint32), np.nan_to_num(o["summary"]).view(np.uint32)), (model, cap, thresh)
    finally:
        _lib.lib().nddm_set_tuning(0, 0, 0, 0, 0, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [68, 400])
def test_step_count_in_the_other_kernels_that_share_the_block(cap, oracle_mod):
    """The general kernels (more than 512 trials per tile: SMALL = 0) and the variant with the round keys in VGPRs."""
    from bayesflow_nddms_amd import _lib, engine
    import oracle
    p = mixture("basic", 24)
    o = oracle.philox_simulate(0, p, 700, dt=0.01, max_steps=float(cap), seed=5, set_offset=2, want_k=True, threads=8)
    assert np.bincount(o["k"][o["trials"][..., 1] != 0] % 4, minlength=4).min() >= 30 and (o["k"] == cap).mean() > 0.05
    try:
        for variant in (1, 2):
            _lib.check(_lib.lib().nddm_set_tuning(0, 0, 0, variant, 0, 0))
            for N in (700, 300):
                g = engine.simulate(0, p, N, dt=0.01, max_steps=float(cap), seed=5, set_offset=2, fast=False)["trials"].cpu().numpy()
                ref = o["trials"] if N == 700 else oracle.philox_simulate(0, p, N, dt=0.01, max_steps=float(cap), seed=5, set_offset=2, threads=8)["trials"]
                assert np.array_equal(g.view(np.uint32), ref.view(np.uint32)), (cap, variant, N)
    finally:
        _lib.lib().nddm_set_tuning(0, 0, 0, 0, 0, 0)


@pytest.mark.gpu
def test_step_count_in_the_codes(oracle_mod):
    """out_codes: the kernel variant that also stores (step index | code << 14); a cap on the far side of the near-cap rule."""
    from bayesflow_nddms_amd import engine
    p, o = reference("basic", 400)
    g = engine.simulate(0, p, 300, dt=0.01, max_steps=400.0, seed=2023, set_offset=11, fast=False, want_codes=True)
    c = g["codes"].cpu().numpy().view(np.uint16).astype(np.int64)
    choice = o["trials"][..., 1]
    code = np.where(choice == 0, 0, np.where(choice > 0, 1, 2))
    assert np.array_equal(c & 0x3fff, o["k"]) and np.array_equal(c >> 14, code)
    assert np.array_equal(g["trials"].cpu().numpy().view(np.uint32), o["trials"].view(np.uint32))


@pytest.mark.gpu
def test_fast_mode_reproduces_the_parent_build():
    from bayesflow_nddms_amd import engine
    gold = np.load(GOLDEN)
    p = prior_util.basic_prior(256, 2023)
    assert np.array_equal(p.view(np.uint32), gold["params"].view(np.uint32))
    g = engine.simulate(0, p, 300, dt=0.001, max_steps=4000.0, seed=2023, set_offset=0, fast=True, want_codes=True)
    c = g["codes"].cpu().numpy().view(np.uint16)
    assert gold["codes"].dtype == np.uint16 and gold["codes"].shape == (256, 300)
    k = gold["codes"] & 0x3fff
    # (the recorded run itself ends trials at every residue and at the cap)
    assert np.bincount(k[(gold["codes"] >> 14) != 0] % 4, minlength=4).min() > 1000 and (k == 4000).any()
    differ = int((c != gold["codes"]).sum())
    print(f"fast mode: {differ} of {c.size} codes differ from the parent build's")
    assert differ == 0
