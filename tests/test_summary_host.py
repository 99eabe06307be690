"""CPU tests of the summary reference (tests/summary_ref.py) and its bounds: the oracle's fused summaries (oracle/ddm_oracle.c, the
restatement the device equals bit for bit in exact mode) against an exact recomputation from the oracle's own trials -- every model,
the packed layout, the bridge, the float64 state -- on the rows and shapes tests/test_gpu_summary.py runs on the device.  Measured here:
columns 3-6 within 0.500 float32 ulp of the exact value at every shape (bound 1), mean_z within 0.999 and var_z within 0.955 of their
bounds (profiles/r25_summary_exact.txt)."""
import numpy as np
import pytest

import summary_ref as sr

N_HOST = (1, 2, 64, 65, 300, 513)


def _oracle_run(oracle_mod, model, N, dt, ms, bridge=False, packed=False, seed=5):
    p, bounds = sr.rows_and_bounds(model, N)
    r = oracle_mod.philox_simulate(model, p, N, dt=dt, max_steps=ms, seed=seed, set_offset=3, bounds=bounds, bridge=bridge, packed=packed,
                                   want_k=True, threads=8)
    return p, r


def _hold(oracle_mod, model, shapes, label, **kw):
    worst = {"ulp": 0.0, "mean_z": 0.0, "var_z": 0.0}
    for N in N_HOST:
        for dt, ms in shapes:
            p, r = _oracle_run(oracle_mod, model, N, dt, ms, **kw)
            ref = sr.summary_from_trials(model, p, r["trials"], dt, kw.get("bridge", False), N)
            if not kw.get("bridge", False):       # the recovered integer time is the step index the oracle reports
                k, code, known = sr.recover(model, p, r["trials"], dt, False)
                resp = (code == sr.C_UPPER) | (code == sr.C_LOWER)
                assert np.array_equal(k[resp], r["k"][resp])
            f = sr.check_summary(model, r["summary"], ref, (label, N, dt, ms))
            worst = {key: max(worst[key], f[key]) for key in worst}
    print(f"summary-exact cpu {label}: ulp {worst['ulp']:.3f} mean_z {worst['mean_z']:.3f} var_z {worst['var_z']:.3f}")
    return worst


@pytest.mark.parametrize("model", list(sr.MODEL_NAMES))
def test_oracle_summary_is_the_exact_summary_of_its_trials(oracle_mod, model):
    _hold(oracle_mod, model, sr.SHAPES, sr.MODEL_NAMES[model])


@pytest.mark.parametrize("model", [sr.M_BASIC, sr.M_SINGLE])
def test_oracle_summary_packed_layout(oracle_mod, model):
    _hold(oracle_mod, model, [s for s in sr.SHAPES if s[1] < 16384], sr.MODEL_NAMES[model] + " packed", packed=True)


def test_oracle_summary_bridge(oracle_mod):
    """The bridge's time unit is 1/256 step: tscale = float32(dt) * float32(1/256)."""
    _hold(oracle_mod, sr.M_ALPHA_NS, sr.BRIDGE_SHAPES, "alpha_ns bridge", bridge=True)


@pytest.mark.parametrize("model", [sr.M_BASIC, sr.M_SINGLE])
def test_oracle_summary_state_f64(oracle_mod, model):
    worst = 0.0
    for N in N_HOST:
        for dt, ms in sr.SHAPES:
            p, _ = sr.rows_and_bounds(model, N)
            r = oracle_mod.philox_simulate_f64(model, p, N, dt=dt, max_steps=ms, seed=5, set_offset=3, threads=8, want_outputs=True)
            ref = sr.summary_from_trials(model, p, r["trials"], dt, False, N)
            worst = max(worst, sr.check_summary(model, r["summary"], ref, ("f64", model, N, dt, ms))["ulp"])
    print(f"summary-exact cpu {sr.MODEL_NAMES[model]} state_f64: ulp {worst:.3f}")


def test_row_e_loads_the_packed_sums(oracle_mod):
    """The worst case of the 16-bit flush path is what it is meant to be: at dt = .001, cap 16383, 512 trials, every trial of row e
    answers late, and a lane's sum of squares (trials j, j + 64, ...: 8 per lane) comes close to the 2^31 its accumulator holds."""
    for model in sr.MODEL_NAMES:
        p, r = _oracle_run(oracle_mod, model, 512, 0.001, 16383.0)
        k, code, _ = sr.recover(model, p, r["trials"], 0.001, False)
        resp = (code[sr.ROW_E] == sr.C_UPPER) | (code[sr.ROW_E] == sr.C_LOWER)
        assert resp.sum() >= 500, (model, int(resp.sum()))
        lane = ((k[sr.ROW_E] * resp) ** 2).reshape(8, 64).sum(axis=0)
        assert 0.9 * 2**31 < lane.max() < 2**31, (model, int(lane.max()))


def test_reference_on_made_up_trials():
    """The reference itself on a hand-made set: invalid trials (NaN) of the explicit model count as missing, an empty selection is NaN,
    a single response has variance exactly 0, and a summary that is off by 2 float32 ulps, has a wrong count or a negative variance is
    refused."""
    dt, tau = np.float32(0.01), np.float32(0.25)
    ks = np.array([3, 7, 7, 12])
    rt = np.array([sr._fma32_exact(k, dt, tau) for k in ks], np.float32)
    t = np.zeros((1, 7, 2), np.float32)
    t[0, :4, 0] = rt * np.array([1, -1, -1, -1], np.float32)
    t[0, 4, 0] = np.nan
    t[0, :, 1] = 1.5
    p = np.array([[1.0, 0.5, tau, 1.0]], np.float32)
    ref = sr.summary_from_trials(sr.M_EXPLICIT, p, t, dt, False, 7)
    assert ref[0, :3].tolist() == [1, 3, 3] and ref[0, 6] == 0 and ref[0, 9] == np.float32(2.5 / 7)
    assert abs(ref[0, 3] - (0.25 + 0.01 * 7.25)) < 1e-8 and abs(ref[0, 4] - 1e-4 * np.var(ks)) < 1e-10
    good = ref.astype(np.float32)
    sr.check_summary(sr.M_EXPLICIT, good, ref)
    for col, val in ((4, np.nextafter(np.nextafter(good[0, 4], np.float32(1)), np.float32(1))), (0, 2.0), (6, np.float32(1e-12)), (8, -1e-9)):
        bad = good.copy()
        bad[0, col] = val
        with pytest.raises(AssertionError):
            sr.check_summary(sr.M_EXPLICIT, bad, ref)
    t[0, 5, 0] = np.float32(0.2512345)                                  # no integer time gives this float
    with pytest.raises(AssertionError, match="no integer time"):
        sr.summary_from_trials(sr.M_EXPLICIT, p, t, dt, False, 7)


def test_var_z_is_never_negative(oracle_mod):
    """The fixed-point sums truncate every term, so sum z^2 / N - mean^2 can come out below 0 (one trial; sigma1 = 1e-5, gamma = 0,
    where z^2 2^24 truncates to 0): the summary clamps it at 0, and values that were not negative keep their bits."""
    for model in (sr.M_SINGLE, sr.M_ALT):
        for N in (1, 2, 3, 300):
            p, _ = sr.rows_and_bounds(model, N)
            s = oracle_mod.philox_simulate(model, p, N, dt=0.01, max_steps=400.0, seed=1, threads=8)["summary"]
            assert np.all(s[:, 8] >= 0) and not np.signbit(s[:, 8]).any(), (model, N, s[:, 8].min())
    assert s[3, 8] == 0 and s[1, 8] > 1
