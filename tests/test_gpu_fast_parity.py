"""The fast Gaussian mode -- the product default, what bench.py times -- held to the oracle TRIAL BY TRIAL.

Fast mode differs from exact mode in one place: the Box-Muller factors (r, cos, sin) come from the transcendental unit.  The device
is asked for its own factors at the Philox counters a case will use (engine.debug_normals(raw=True): the step loop's form of the
pair for the path stream, the auxiliary stream's form for the latents and the external datum, the packed layout's), the oracle reads
them in place of its exact transform and applies the noise unit sqrt(2 ln 2) where the kernels do (tests/fast_parity_ref.py,
oracle/ddm_oracle.c: xform_tab) -- and every trial, summary column, external datum and code must then be equal BIT FOR BIT.

The one operation no table can hold is the bridge correction's v_exp_f32, whose argument depends on the path.  The oracle forms
2^x in float64 and reports a trial whose crossing test lies within 2 x the instruction's error bound (+ 1 ulp) of it as UNDECIDED;
such trials (and, for summaries, their sets) are left out, and at most 1e-4 of a case's trials may be -- asserted.

engine.simulate admits state_f64=True with fast=True, so that pair is covered as well (oracle_philox_simulate_f64 with the same table).
nddm_simulratcliff's fast mode is out of scope: its transcendentals act on path-dependent values throughout.

Every case prints one `FASTPARITY` line: trials, undecided share, and -- for the record only -- the share of trials on which the fast
mode agrees with the EXACT transform's oracle (profiles/r26_fast_parity.txt)."""
import numpy as np
import pytest

import fast_parity_ref as fp

pytestmark = pytest.mark.gpu


def _np(d):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items()}


def _oracle(model, p, N, dt, max_steps, seed, set_offset=0, bounds=None, bridge=False, packed=False, state_f64=False):
    return fp.oracle_on_table(fp.device_dump, model, p, N, dt=dt, max_steps=max_steps, seed=seed, set_offset=set_offset, bounds=bounds,
                              ext_sigma=0.1, ext_mode=0, bridge=bridge, packed=packed, state_f64=state_f64)


def _assert_equal(tag, model, g, o, want_trials=True):
    """Bits of everything the launch wrote against the oracle-on-table; returns the undecided share."""
    und = o.get("undecided")
    und = np.zeros(o["trials"].shape[:2], bool) if und is None else und
    share = float(und.mean())
    assert share <= fp.UNDECIDED_CAP, (tag, share)
    if want_trials:
        gt, ot = fp.bits(g["trials"]), fp.bits(o["trials"])
        bad = (gt != ot).any(axis=-1) & ~und
        assert not bad.any(), (tag, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    if "summary" in g:
        rows = ~und.any(axis=1)
        assert fp.same_bits_nan_aware(g["summary"][rows], o["summary"][rows]), tag
    if model == "alpha_ns" and "ext" in g:
        assert np.array_equal(fp.bits(g["ext"]), fp.bits(o["ext"])), tag
    return share


def _record(tag, model, p, N, dt, max_steps, seed, set_offset, o, share, bounds=None, bridge=False, packed=False, state_f64=False):
    import oracle
    m = fp.MODELS[model]
    if state_f64:
        ex = oracle.philox_simulate_f64(m, p, N, dt=dt, max_steps=max_steps, seed=seed, set_offset=set_offset, threads=8, want_outputs=True)
    else:
        ex = oracle.philox_simulate(m, p, N, dt=dt, max_steps=max_steps, seed=seed, set_offset=set_offset, bounds=bounds, ext_sigma=0.1,
                                    bridge=bridge, packed=packed, want_summary=False, threads=8)
    agree = float((fp.bits(ex["trials"][..., 0]) == fp.bits(o["trials"][..., 0])).mean())
    capped = int((o["k"] >= int(np.ceil(max_steps))).sum())
    print(f"FASTPARITY {tag} trials={o['trials'].shape[0] * N} capped={capped} undecided={share:.2e} agree_exact={agree:.5f}")


def _case(tag, model, B, N, dt, max_steps, seed, set_offset=0, bridge=False, packed=False, state_f64=False, params=None):
    from bayesflow_nddms_amd import engine
    p = fp.case_params(model, B, 1234 + B) if params is None else np.ascontiguousarray(params, np.float32)
    bounds = fp.case_bounds(B, N) if model == "explicit" else None
    g = _np(engine.simulate(fp.MODELS[model], p, N, dt=dt, max_steps=max_steps, seed=seed, set_offset=set_offset, fast=True, bounds=bounds,
                            ext_sigma=0.1, ext_mode=0, want_ext=(model == "alpha_ns"), bridge=bridge, packed=packed, state_f64=state_f64))
    o = _oracle(model, p, N, dt, max_steps, seed, set_offset, bounds, bridge, packed, state_f64)
    share = _assert_equal(tag, model, g, o)
    _record(tag, model, p, N, dt, max_steps, seed, set_offset, o, share, bounds, bridge, packed, state_f64)
    return p, g, o


@pytest.mark.parametrize("model", list(fp.MODELS))
@pytest.mark.parametrize("dt,max_steps", [(0.01, 400.0), (0.001, 4000.0)])
def test_every_model(model, dt, max_steps):
    _case(f"model-{model}-dt{dt}", model, 24, 300, dt, max_steps, seed=2023)


@pytest.mark.parametrize("max_steps", [1.0, 2.0, 3.0, 5.0, 399.0, 401.0])
def test_step_caps_that_leave_cap4(max_steps):
    """Step caps that are not a multiple of 4: the cap is tested per step, in the C form of the step."""
    p, g, o = _case(f"cap-{int(max_steps)}", "basic", 24, 100, 0.01, max_steps, seed=3)
    assert o["k"].max() == int(max_steps)


@pytest.mark.parametrize("N", [1, 63, 64, 65, 513])
def test_trial_counts_at_lane_and_tile_edges(N):
    """A one-trial set, one lane short of a wave, a wave, one lane more, a set split into two tiles."""
    _case(f"ntrials-{N}", "basic", 40, N, 0.01, 400.0, seed=7)


@pytest.mark.parametrize("model", ["basic", "single"])
def test_wide_step_cap_32bit_staging(model):
    """Step caps from 2^14 on stage a trial's result as a 32-bit word instead of a 16-bit one."""
    p, g, o = _case(f"cap20000-{model}", model, 16, 40, 0.0005, 20000.0, seed=77)
    assert o["k"].max() > 16383            # the case does hold step indices beyond 14 bits


@pytest.mark.parametrize("dt,max_steps", fp.BRIDGE_CASES)
def test_bridge(dt, max_steps):
    """The Brownian-bridge step: as inline assembly (caps that are a multiple of 8) with its two v_fmaak literals and the 32-bit /
    16-bit split of the uniform word, and its C form (cap 1001).  Compared on every decided trial; summaries on the sets without an
    undecided one; the undecided share is asserted <= 1e-4 (tests/test_fast_parity_host.py checks the same cases without a GPU)."""
    _case(f"bridge-dt{dt}-cap{int(max_steps)}", "alpha_ns", fp.BRIDGE_B, fp.BRIDGE_N, dt, max_steps, seed=fp.BRIDGE_SEED, bridge=True)


@pytest.mark.parametrize("model", ["basic", "single"])
@pytest.mark.parametrize("dt,max_steps", [(0.01, 400.0), (0.01, 403.0)])
def test_packed_layout(model, dt, max_steps):
    """polar_pair_packed<true>: 8 steps per Philox block, also with a cap that is not a multiple of 8."""
    _case(f"packed-{model}-cap{int(max_steps)}", model, 24, 300, dt, max_steps, seed=2024, packed=True)


@pytest.mark.parametrize("model", ["basic", "single"])
@pytest.mark.parametrize("dt,max_steps", [(0.001, 4000.0), (0.01, 403.0)])
def test_float64_state(model, dt, max_steps):
    """NDDM_STATE_F64 with the fast transform: sdc *= sqrt(2 ln 2) in double, the normal the exact double product of the table's
    float32 factors (oracle_philox_simulate_f64 with the same table)."""
    _case(f"f64-{model}-cap{int(max_steps)}", model, 24, 300, dt, max_steps, seed=2025, set_offset=7, state_f64=True)


@pytest.mark.parametrize("model", ["basic", "single"])
def test_tuning_overrides(model):
    """Both key variants of the kernel (round keys from LDS / in VGPRs), refill thresholds 4 and 64 (lockstep) and a ring of 2: the fast
    mode's bits do not depend on them, and they are the oracle's."""
    from bayesflow_nddms_amd import _lib, engine
    B, N, dt, ms, seed = 24, 300, 0.001, 4000.0, 5
    p = fp.case_params(model, B, 1234 + B)
    o = _oracle(model, p, N, dt, ms, seed, set_offset=99)
    seen = set()
    try:
        for tune in ((0, 0, 0, 1, 0, 0), (0, 0, 0, 2, 0, 0), (0, 0, 4, 0, 0, 0), (0, 0, 64, 0, 0, 0), (0, 2, 0, 0, 0, 0)):
            _lib.check(_lib.lib().nddm_set_tuning(*tune))
            g = _np(engine.simulate(fp.MODELS[model], p, N, dt=dt, max_steps=ms, seed=seed, set_offset=99, fast=True))
            ll = engine.last_launch()
            seen.add(ll["vgpr_keys"])
            if tune[3] and model == "basic":           # (the single-trial kernels have no variant with the keys in VGPRs)
                assert ll["vgpr_keys"] == tune[3] - 1
            if tune[1]:
                assert ll["ring"] == 2
            _assert_equal(f"tuning-{model}-{tune}", model, g, o)
    finally:
        _lib.lib().nddm_set_tuning(0, 0, 0, 0, 0, 0)
    assert seen == ({0, 1} if model == "basic" else {0})
    _record(f"tuning-{model}", model, p, N, dt, ms, seed, 99, o, 0.0)


@pytest.mark.parametrize("model", ["single", "alt"])
def test_rejection_heavy_rows(model):
    """std of the per-trial latent about its mean: one draw in six is rejected, so AuxStream<true>::normal(a) beyond the first pair runs."""
    B = 24
    p = fp.case_params(model, B, 1234 + B)
    if model == "single":
        p[:, 4] = p[:, 1]                  # std_alpha = mu_alpha
    else:
        p[:, 4] = p[:, 5]                  # std_dc = mu_dc
    _case(f"rejection-{model}", model, B, 300, 0.01, 400.0, seed=4, params=p)


@pytest.mark.parametrize("model", ["single", "alt"])
def test_rejection_cap_fallback_row(model):
    """The row of test_gpu_parity.py::test_rejection_cap_fallback: the rejection loop runs to its 64 draws and falls back to |last draw|."""
    p = np.array([[1.0, -3.0, 0.5, 0.3, 0.5, 1.0, 0.2, 1.0]] * 3, dtype=np.float32)
    if model == "alt":
        p[:, 1], p[:, 5] = 1.0, -3.0
    p_, g, o = _case(f"rejection-cap-{model}", model, 3, 70, 0.01, 400.0, seed=4, params=p)
    assert np.all(np.isfinite(o["trials"]))


def test_set_offset_beyond_32_bits():
    _case("set-offset-2^36", "single", 24, 100, 0.01, 400.0, seed=2026, set_offset=(1 << 36) + 11)


def test_summary_only_and_codes():
    """want_trials=False: the same summary bits; nddm_simulate_codes: codes that are the oracle's (step, choice) and decode to its floats."""
    import torch
    from bayesflow_nddms_amd import engine
    B, N, dt, ms, seed = 24, 300, 0.01, 400.0, 17
    for model in ("basic", "single"):
        p = fp.case_params(model, B, 1234 + B)
        o = _oracle(model, p, N, dt, ms, seed, set_offset=3)
        g = _np(engine.simulate(fp.MODELS[model], p, N, dt=dt, max_steps=ms, seed=seed, set_offset=3, fast=True, want_trials=False))
        assert "trials" not in g
        share = _assert_equal(f"summary-only-{model}", model, g, o, want_trials=False)
        _record(f"summary-only-{model}", model, p, N, dt, ms, seed, 3, o, share)
    for model in ("basic", "alpha_ns"):
        p = fp.case_params(model, B, 1234 + B)
        o = _oracle(model, p, N, dt, ms, seed, set_offset=3)
        r = engine.simulate(fp.MODELS[model], p, N, dt=dt, max_steps=ms, seed=seed, set_offset=3, fast=True, want_codes=True, ext_sigma=0.1,
                            want_ext=(model == "alpha_ns"))
        only = engine.simulate(fp.MODELS[model], p, N, dt=dt, max_steps=ms, seed=seed, set_offset=3, fast=True, want_codes=True, want_trials=False,
                               want_summary=False, ext_sigma=0.1, want_ext=(model == "alpha_ns"))
        assert torch.equal(only["codes"], r["codes"]) and ("ext" in r) == (model == "alpha_ns")
        if model == "alpha_ns":             # the codes entry has no ext output: the front end fills the datum with a launch of its own
            assert torch.equal(only["ext"], r["ext"])
        dec = engine.decode_codes(fp.MODELS[model], only["codes"], r["params"], dt).cpu().numpy()
        g = _np(r)
        share = _assert_equal(f"codes-{model}", model, g, o)
        assert np.array_equal(fp.bits(dec), fp.bits(o["trials"]))
        c = g["codes"].view(np.uint16).astype(np.int64)
        choice = o["trials"][..., 1] if model == "basic" else 2.0 * o["trials"][..., 1] - 1.0
        timeout = (o["trials"][..., 0] == 0.0) if model == "alpha_ns" else (choice == 0)
        assert np.array_equal(c & 0x3fff, o["k"]) and np.array_equal(c >> 14, np.where(timeout, 0, np.where(choice > 0, 1, 2)))
        _record(f"codes-{model}", model, p, N, dt, ms, seed, 3, o, share)


def test_polar_pair_forms(oracle_mod):
    """The step loop's form of polar_pair (HOT: the angle spliced by v_bitop3_b32) and the auxiliary stream's (shift + v_alignbit_b32)
    build the same bits; the raw dump is what the normals of flags 0 / 1 are made of, (r * unit) * cos|sin; and the raw dump of the
    EXACT transform, in all three forms, is the oracle's."""
    from bayesflow_nddms_amd import engine
    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 2**32, size=(1 << 20, 4), dtype=np.uint64).astype(np.uint32)
    ctr[:8] = [[0, 0, 0, 0], [1, 0, 0, 0], [0xffffffff] * 4, [0, 1, 2, 3], [0, 0, 0, 0x10000000],
               [5, 0xffffffff, 7, 0x1fffffff], [123, 456, 789, 0x20000000], [2**31, 2**31, 2**31, 2**27]]
    k0, k1 = 2023, 0xdeadbeef
    for fast in (True, False):
        hot = engine.debug_normals(ctr, k0, k1, fast=fast, raw=True, form="hot")
        aux = engine.debug_normals(ctr, k0, k1, fast=fast, raw=True, form="aux")
        assert hot.shape == (len(ctr), 6) and np.array_equal(fp.bits(hot), fp.bits(aux)), fast
        z = engine.debug_normals(ctr, k0, k1, fast=fast)
        unit = oracle_mod.FAST_UNIT if fast else np.float32(1.0)
        r0, r1 = aux[:, 0] * unit, aux[:, 3] * unit
        made = np.stack([r0 * aux[:, 1], r0 * aux[:, 2], r1 * aux[:, 4], r1 * aux[:, 5]], axis=1)
        assert np.array_equal(fp.bits(made), fp.bits(z)), fast
    n = 20000
    assert np.array_equal(fp.bits(aux[:n]), fp.bits(oracle_mod.philox_raw(ctr[:n], k0, k1)))
    pk = engine.debug_normals(ctr[:n], k0, k1, fast=False, raw=True, form="packed")
    assert pk.shape == (n, 12) and np.array_equal(fp.bits(pk), fp.bits(oracle_mod.philox_raw(ctr[:n], k0, k1, packed=True)))
    # The FAST transform's auxiliary and packed forms are dumped by the code the kernels run, so the trial comparisons cannot see a
    # wrong mask or shift in them (the step loop's form is tied to the auxiliary one above).  Hold them to a float64 evaluation of the
    # same function of the same words (oracle.philox_raw(standin=True)), with tolerances that come from the layout, not from the device:
    # the coarsest field a fault can move is one bit of the packed layout's 16-bit angle or 16-bit radius uniform, and the bound is a
    # quarter of what that bit moves.
    #   angle : one bit = 2^-16 turns = 2 pi 2^-16 rad, which moves cos / sin by up to as much: bound 2 pi 2^-18 = 2.4e-5 (absolute)
    #   radius: compared as L = r^2 = -log2 u, where the unit's error stays small next to u = 1 (the root would magnify it there).
    #           One bit of u = 2^-16 moves L by 2^-16 / (u ln 2) >= 2.2e-5, and by far more than L itself for small u:
    #           bound 5.5e-6 * max(1, L) -- 46 float32 ulp where L > 1, against the few ulp the log, the root and the squaring add
    n = 1 << 18
    for form in ("aux", "packed"):
        dev = engine.debug_normals(ctr[:n], k0, k1, fast=True, raw=True, form=form).astype(np.float64).reshape(n, -1, 3)
        ref = oracle_mod.philox_raw(ctr[:n], k0, k1, packed=(form == "packed"), standin=True).astype(np.float64).reshape(n, -1, 3)
        L = ref[..., 0] ** 2
        err_l = float((np.abs(dev[..., 0] ** 2 - L) / np.maximum(1.0, L)).max())
        err_a = float(np.abs(dev[..., 1:] - ref[..., 1:]).max())
        print(f"FASTFORM {form}: max |r^2 - L| / max(1, L) = {err_l:.2e} (bound 5.5e-6), max |cos, sin - ref| = {err_a:.2e} (bound 2.4e-5)")
        assert err_l <= 5.5e-6 and err_a <= 2.0 * np.pi * 2.0 ** -18, (form, err_l, err_a)
    with pytest.raises(ValueError):
        engine.debug_normals(ctr[:4], k0, k1, form="hot")
    from bayesflow_nddms_amd import _lib
    import torch
    d = torch.zeros(64, device="cuda")
    for flags in (4, 8, 1 | 4, 2 | 4 | 8, 16):
        with pytest.raises(ValueError, match="nddm_debug_normals"):
            _lib.check(_lib.lib().nddm_debug_normals(d.data_ptr(), 1, 1, 2, flags, d.data_ptr(), None))
