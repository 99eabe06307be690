"""The fused summaries of every simulator launch held to an exact recomputation from THAT launch's own trials (tests/summary_ref.py), so
the fast transform -- which has no oracle -- is held as tightly as the exact one: counts and column 9 equal, the time moments (columns
3-6) within 1 float32 ulp of the exact rational value, the z moments within the bounds of their fixed-point format, no variance below 0.

Every epilogue variant of flush_set (csrc/nddm_sim.h): the 16-bit DPP path and the 32-bit one (bridge, max_steps >= 16384), sets split
into tiles and a padded last tile, tiles of fewer than 64 trials and of 512 (a 10-bit counter holding 512; the sums of squares of row
e, summary_ref.edge_rows, within 2 % of a lane's 32 bits), the codes kernels, the packed layout, NDDM_STATE_F64, both key placements,
summary-only launches.  In exact mode the summary bits also equal the oracle's.

Worst values measured on an MI355X (profiles/r25_summary_exact.txt), fast and exact mode alike: columns 3-6 0.500 ulp in every variant
(0.499 for single packed and under the tuning overrides); mean_z 1.000 (rounded; single), 0.999 (single_alt) of its bound; var_z 0.951
fast / 0.945 exact (single), 0.971 / 0.967 (single_alt), 0.979 (3000 sets x 7 trials, exact) of its bound; no negative variance.  The
CPU oracle's figures (tests/test_summary_host.py): 0.500 ulp, mean_z 0.999, var_z 0.955."""
import numpy as np
import pytest

import prior_util
import summary_ref as sr

pytestmark = pytest.mark.gpu

N_ALL = (1, 2, 63, 64, 65, 300, 512, 513, 1025)
SEED, OFFSET = 20251, 2**32 - 5          # (the sets of a launch straddle a 32-bit boundary of the global set index)
TILE_512 = (0, 0, 0, 0, 0, 512)


def _tuning(t):
    from bayesflow_nddms_amd import _lib
    _lib.check(_lib.lib().nddm_set_tuning(*t))


def _bits(a):
    return np.nan_to_num(np.asarray(a, np.float32)).view(np.uint32)


def _launch(model, N, dt, ms, fast, invalid=False, rows=None, **kw):
    """One launch of the model's rows; the device results as NumPy arrays, plus the parameters and bounds."""
    import torch
    from bayesflow_nddms_amd import engine
    p, bounds = sr.rows_and_bounds(model, N, invalid=invalid) if rows is None else rows
    dev_bounds = None if bounds is None else torch.as_tensor(bounds).cuda()      # (a device tensor: invalid bounds pass unread)
    g = engine.simulate(model, p, N, dt=dt, max_steps=ms, seed=SEED, set_offset=OFFSET, fast=fast, bounds=dev_bounds, **kw)
    out = {k: v.cpu().numpy() for k, v in g.items() if k in ("trials", "summary", "codes")}
    out["p"], out["bounds"] = p, bounds
    return out


_ORACLE = {}          # the oracle's result does not depend on the launch geometry: one run serves every tuning of a shape


def _oracle_summary(model, g, N, dt, ms, bridge=False, packed=False, state_f64=False):
    """The oracle on the launch's rows.  The slow rows (a, d, e run to the cap or near it) sit side by side, so the rows go to the
    oracle a few at a time from a thread pool (a set's stream is keyed by set_offset + row: the split changes nothing)."""
    from concurrent.futures import ThreadPoolExecutor
    import oracle
    p = g["p"]
    bounds = None if g["bounds"] is None else np.abs(g["bounds"])       # (the oracle has no invalid trials: those rows are left out)
    key = (model, N, dt, ms, bridge, packed, state_f64, p.tobytes())
    if key not in _ORACLE:
        if len(_ORACLE) >= 8:
            _ORACLE.clear()
        step = max(2, -(-len(p) // 16))
        oracle.lib()

        def part(i):
            if state_f64:
                return oracle.philox_simulate_f64(model, p[i:i + step], N, dt=dt, max_steps=ms, seed=SEED, set_offset=OFFSET + i,
                                                  want_outputs=True)
            return oracle.philox_simulate(model, p[i:i + step], N, dt=dt, max_steps=ms, seed=SEED, set_offset=OFFSET + i,
                                          bounds=None if bounds is None else bounds[i:i + step], bridge=bridge, packed=packed)
        with ThreadPoolExecutor(8) as pool:
            parts = list(pool.map(part, range(0, len(p), step)))
        _ORACLE[key] = {k: np.concatenate([q[k] for q in parts]) for k in ("trials", "summary")}
    return _ORACLE[key]


class Worst:
    def __init__(self, label):
        self.label, self.f = label, {"ulp": 0.0, "mean_z": 0.0, "var_z": 0.0}

    def add(self, f):
        self.f = {k: max(v, f[k]) for k, v in self.f.items()}

    def report(self):
        print(f"summary-exact gpu {self.label}: ulp {self.f['ulp']:.3f} mean_z {self.f['mean_z']:.3f} var_z {self.f['var_z']:.3f}")


def _hold(w, model, N, dt, ms, fast, invalid=False, bridge=False, packed=False, state_f64=False, want_codes=False, rows=None):
    """Launch, recompute, compare; exact mode: the oracle's bits as well.  Returns the launch."""
    kw = {k: True for k, v in (("bridge", bridge), ("packed", packed), ("state_f64", state_f64), ("want_codes", want_codes)) if v}
    g = _launch(model, N, dt, ms, fast, invalid=invalid, rows=rows, **kw)
    ctx = (w.label, N, dt, ms, "fast" if fast else "exact")
    ref = sr.summary_from_trials(model, g["p"], g["trials"], dt, bridge, N, codes=g.get("codes"))
    w.add(sr.check_summary(model, g["summary"], ref, ctx))
    if invalid:
        assert ref[3, 2] >= len(range(0, N, 7)) and np.isnan(g["trials"][3, ::7, 0]).all(), ctx
    if rows is None and dt == 0.001 and ms >= 16383 and N == 512:         # row e really loads the sums
        assert ref[sr.ROW_E, 0] + ref[sr.ROW_E, 1] >= 500, ctx
    if not fast:
        o = _oracle_summary(model, g, N, dt, ms, bridge=bridge, packed=packed, state_f64=state_f64)
        keep = np.ones(len(g["p"]), bool)
        keep[3] = not invalid
        assert np.array_equal(np.isnan(g["summary"][keep]), np.isnan(o["summary"][keep])), ctx
        assert np.array_equal(_bits(g["summary"][keep]), _bits(o["summary"][keep])), ctx
        assert np.array_equal(_bits(g["trials"][keep]), _bits(o["trials"][keep])), ctx
    return g


def _sweep(w, model, fast, shapes, n_all=N_ALL, **kw):
    """Every N x shape at the library's own geometry (a launch this small is cut into tiles of <= 64 trials: partial waves, split
    sets), and the sets of 512 and more trials again in tiles of up to 512 (N = 513: two tiles of 257; 1025: three of 342)."""
    from bayesflow_nddms_amd import engine
    try:
        for N in n_all:
            for dt, ms in shapes:
                _hold(w, model, N, dt, ms, fast, **kw)
                assert engine.last_launch()["tile_trials"] <= 64
                if N >= 512:
                    _tuning(TILE_512)
                    _hold(w, model, N, dt, ms, fast, **kw)
                    assert engine.last_launch()["tile_trials"] == {512: 512, 513: 257, 1025: 342}[N]
                    _tuning((0,) * 6)
    finally:
        _tuning((0,) * 6)
    w.report()


@pytest.mark.parametrize("fast", [True, False], ids=["fast", "exact"])
@pytest.mark.parametrize("model", list(sr.MODEL_NAMES), ids=list(sr.MODEL_NAMES.values()))
def test_summary_equals_exact_recomputation(model, fast):
    """All five models, both transforms, N x (dt, max_steps) -- 16383 is the last cap with 16-bit results, 16384 the first with 32-bit
    ones, max_steps = 0 ends every trial at once; the explicit-boundary model with every 7th boundary of one row negative."""
    w = Worst(f"{sr.MODEL_NAMES[model]} {'fast' if fast else 'exact'}")
    _sweep(w, model, fast, sr.SHAPES, invalid=(model == sr.M_EXPLICIT))


@pytest.mark.parametrize("fast", [True, False], ids=["fast", "exact"])
def test_summary_bridge(fast):
    """alpha_not_scaled with the bridge: 32-bit results in units of 1/256 step, tscale = float32(dt) * float32(1/256)."""
    w = Worst(f"alpha_ns bridge {'fast' if fast else 'exact'}")
    _sweep(w, sr.M_ALPHA_NS, fast, sr.BRIDGE_SHAPES, bridge=True)


@pytest.mark.parametrize("fast", [True, False], ids=["fast", "exact"])
@pytest.mark.parametrize("model", [sr.M_BASIC, sr.M_SINGLE], ids=["basic", "single"])
def test_summary_packed(model, fast):
    w = Worst(f"{sr.MODEL_NAMES[model]} packed {'fast' if fast else 'exact'}")
    _sweep(w, model, fast, [s for s in sr.SHAPES if s[1] < 16384], packed=True)


@pytest.mark.parametrize("fast", [True, False], ids=["fast", "exact"])
@pytest.mark.parametrize("model", [sr.M_BASIC, sr.M_SINGLE], ids=["basic", "single"])
def test_summary_state_f64(model, fast):
    w = Worst(f"{sr.MODEL_NAMES[model]} state_f64 {'fast' if fast else 'exact'}")
    _sweep(w, model, fast, sr.SHAPES, state_f64=True)


@pytest.mark.parametrize("fast", [True, False], ids=["fast", "exact"])
@pytest.mark.parametrize("model", [sr.M_BASIC, sr.M_ALPHA_NS], ids=["basic", "alpha_ns"])
def test_summary_codes_kernels(model, fast):
    """The kernels that also store the 2-byte wire format: the codes say what the float pairs say (k = codes & 0x3fff, code =
    codes >> 14), and the summary is the exact one."""
    w = Worst(f"{sr.MODEL_NAMES[model]} codes {'fast' if fast else 'exact'}")
    _sweep(w, model, fast, [s for s in sr.SHAPES if s[1] < 16384], want_codes=True)


@pytest.mark.parametrize("fast", [True, False], ids=["fast", "exact"])
def test_summary_only_launch_has_the_same_bits(fast):
    """want_trials=False (the training feed's launch) writes the summary bits of the launch that also writes the trials."""
    try:
        for model in sr.MODEL_NAMES:
            for N, tune in ((300, (0,) * 6), (512, TILE_512), (1025, (0,) * 6)):
                for dt, ms in ((0.001, 16383.0), (0.001, 16384.0), (0.01, 400.0)):
                    _tuning(tune)
                    a = _launch(model, N, dt, ms, fast)
                    b = _launch(model, N, dt, ms, fast, want_trials=False)
                    assert "trials" not in b and np.array_equal(np.isnan(a["summary"]), np.isnan(b["summary"]))
                    assert np.array_equal(_bits(a["summary"]), _bits(b["summary"])), (model, N, dt, ms)
    finally:
        _tuning((0,) * 6)


@pytest.mark.parametrize("fast", [True, False], ids=["fast", "exact"])
def test_summary_under_tuning_overrides(fast):
    """Both key placements (variant 1: LDS, 2: VGPRs), a padded last tile (N = 250 in tiles of 64 -> 4 x 63, in tiles of 100 -> 3 x 84,
    the last one short), one wave for the whole launch: the summary is the exact one under each."""
    from bayesflow_nddms_amd import engine
    w = Worst(f"tuning {'fast' if fast else 'exact'}")
    try:
        for model in sr.MODEL_NAMES:
            for tune, N, tile in (((0, 0, 0, 1, 0, 0), 300, None), ((0, 0, 0, 2, 0, 0), 300, None), ((0, 0, 0, 1, 0, 512), 512, 512),
                                  ((0, 0, 0, 2, 0, 512), 512, 512), ((0, 0, 0, 0, 0, 64), 250, 63), ((0, 0, 0, 0, 0, 100), 250, 84),
                                  ((0, 0, 0, 0, 1, 0), 300, None), ((0, 0, 0, 0, 1, 512), 512, 512)):
                for dt, ms in ((0.001, 16383.0), (0.001, 16384.0)):
                    _tuning(tune)
                    _hold(w, model, N, dt, ms, fast)
                    ll = engine.last_launch()
                    assert tile is None or ll["tile_trials"] == tile, ll
                    has_vgpr_keys = model in (sr.M_BASIC, sr.M_ALPHA_NS, sr.M_EXPLICIT) and ms < 16384      # (the 16-bit kernels of these)
                    assert tune[3] == 0 or ll["vgpr_keys"] == int(tune[3] == 2 and has_vgpr_keys), ll
                    assert tune[4] == 0 or ll["grid_waves"] == 1, ll
    finally:
        _tuning((0,) * 6)
    w.report()


@pytest.mark.parametrize("fast", [True, False], ids=["fast", "exact"])
def test_summary_many_small_sets(fast):
    """3000 sets of 7 trials from the priors: many sets per wave, 7 of 64 lanes per flush."""
    w = Worst(f"3000 x 7 {'fast' if fast else 'exact'}")
    B, N = 3000, 7
    for model, p in ((sr.M_BASIC, prior_util.basic_prior(B, 3)), (sr.M_SINGLE, prior_util.single_prior(B, 3, gamma=1.5)),
                     (sr.M_ALPHA_NS, prior_util.alpha_ns_prior(B, 3))):
        _hold(w, model, N, 0.001, 4000.0, fast, rows=(p, None))
    w.report()
