"""The oracle's injected transform (oracle/ddm_oracle.c: xform_tab; tests/fast_parity_ref.py) checked without a GPU:
  - a table filled with the oracle's OWN exact factors, with unit 1, gives the bits of the table-free oracle -- every model, both
    layouts, the bridge, the float64 state: the injection changes nothing but where the factors come from;
  - with a float64 stand-in for the fast transform in the table, the bridge cases of tests/test_gpu_fast_parity.py leave at most 1e-4
    of their trials undecided (a crossing test within the error of the device's exp2), so that test's comparison is not hollow."""
import numpy as np
import pytest

import fast_parity_ref as fp

CASES = [(m, packed, False) for m in fp.MODELS for packed in (False, True)] + [("alpha_ns", False, True)]


@pytest.mark.parametrize("model,packed,bridge", CASES)
@pytest.mark.parametrize("dt,max_steps", [(0.01, 400.0), (0.004, 403.0)])
def test_exact_table_with_unit_one_changes_nothing(oracle_mod, model, packed, bridge, dt, max_steps):
    B, N, seed, so = 7, 41, 2023, (1 << 33) + 5
    p = fp.case_params(model, B, 1234 + B)
    bounds = fp.case_bounds(B, N) if model == "explicit" else None
    kw = dict(dt=dt, max_steps=max_steps, seed=seed, set_offset=so, bounds=bounds, ext_sigma=0.1, ext_mode=0, bridge=bridge, packed=packed)
    ref = oracle_mod.philox_simulate(fp.MODELS[model], p, N, want_k=True, want_ext=(model == "alpha_ns"), threads=4, **kw)
    got = fp.oracle_on_table(fp.exact_dump, model, p, N, unit=1.0, fast=False, threads=4, **kw)
    assert not got["undecided"].any()
    assert np.array_equal(fp.bits(got["trials"]), fp.bits(ref["trials"])) and np.array_equal(got["k"], ref["k"])
    assert fp.same_bits_nan_aware(got["summary"], ref["summary"])
    if model == "alpha_ns":
        assert np.array_equal(fp.bits(got["ext"]), fp.bits(ref["ext"]))


@pytest.mark.parametrize("model", ["basic", "single"])
def test_exact_table_with_unit_one_changes_nothing_f64_state(oracle_mod, model):
    B, N = 7, 41
    p = fp.case_params(model, B, 1234 + B)
    kw = dict(dt=0.004, max_steps=403.0, seed=2025, set_offset=7)
    ref = oracle_mod.philox_simulate_f64(fp.MODELS[model], p, N, want_outputs=True, **kw)
    got = fp.oracle_on_table(fp.exact_dump, model, p, N, state_f64=True, unit=1.0, fast=False, threads=4, **kw)
    assert np.array_equal(got["k"], ref["k"]) and np.array_equal(got["choice"], ref["choice"])
    assert np.array_equal(fp.bits(got["trials"]), fp.bits(ref["trials"])) and fp.same_bits_nan_aware(got["summary"], ref["summary"])


def test_a_table_that_is_too_short_is_an_error(oracle_mod):
    p = fp.case_params("basic", 2, 3)
    tab = fp.build_table(fp.exact_dump, 2, 20, 400.0, 1, 0, unit=1.0, fast=False)
    tab["path"] = np.ascontiguousarray(tab["path"][:, :, :3])
    with pytest.raises(ValueError, match="beyond the transform table"):
        oracle_mod.philox_simulate(0, p, 20, dt=0.01, max_steps=400.0, seed=1, set_offset=0, table=tab)


def test_fast_bridge_crossing_test_restated(oracle_mod):
    """The fast kernels' crossing test on a stand-in table against a NumPy restatement of it (x = fma(-4, m, K) in float32, 2^x in
    float64): the oracle's k / choice of every decided trial follow from the same (w, d0, d1) recurrence."""
    B, N, dt, ms, seed = 3, 40, 0.01, 400.0, 5
    p = fp.case_params("alpha_ns", B, 9)
    tab = fp.build_table(fp.standin_dump, B, N, ms, seed, 0)
    o = oracle_mod.philox_simulate(3, p, N, dt=dt, max_steps=ms, seed=seed, set_offset=0, bridge=True, want_k=True, table=tab)
    f = np.float32
    unit = oracle_mod.FAST_UNIT
    for b in range(B):
        inv_s = f(1.0) / ((np.sqrt(f(dt)) * p[b, 5]) * unit)
        hv = f(0.5) * p[b, 1]
        h = hv * inv_s
        for t in range(0, N, 7):
            z = (tab["aux"][b, t, 0, 0] * unit) * tab["aux"][b, t, 0, 1]
            drift = f(np.float64(p[b, 4]) * np.float64(z) + np.float64(p[b, 0]))        # fmaf: one rounding
            mu = (drift * f(dt)) * inv_s
            w = (p[b, 1] * p[b, 2] - hv) * inv_s
            d0 = h - abs(w)
            k, crossed = 0, False
            while k < int(ms) and not crossed and d0 > 0:
                blk = k // 8
                ub = oracle_mod.philox_block((b) & 0xffffffff, t, 0, (8 * blk) | 0x80000000, seed, 0)
                for j in range(8):
                    q = tab["path"][b, t, 2 * blk + j // 4]
                    r, c = q[3 * ((j % 4) // 2)], q[3 * ((j % 4) // 2) + 1 + (j & 1)]
                    w = f(np.float64(r) * np.float64(c) + np.float64(w)) + mu
                    d1 = h - abs(w)
                    m = d0 * d1
                    word = int(ub[j // 2])
                    uf = f(word & 0xffff) if j & 1 else f(word)
                    K = f(16.0) if j & 1 else np.array([0x42000001], np.uint32).view(np.float32)[0]
                    x = f(np.float64(-4.0) * np.float64(m) + np.float64(K))
                    if not float(uf) >= 2.0 ** float(x):
                        crossed = True
                        break
                    k += 1
                    d0 = d1
                    if k >= int(ms):
                        break
            if not o["undecided"][b, t]:
                assert o["k"][b, t] == k + (1 if crossed else 0), (b, t)
                assert np.sign(o["trials"][b, t, 0]) == (np.sign(w) if crossed else 0), (b, t)


@pytest.mark.parametrize("dt,max_steps", fp.BRIDGE_CASES)
def test_undecided_share_of_the_bridge_cases(oracle_mod, dt, max_steps):
    """The device test leaves a trial out when one of its crossing tests cannot be decided on the CPU; at most 1e-4 of a case may be."""
    p = fp.case_params("alpha_ns", fp.BRIDGE_B, 1234 + fp.BRIDGE_B)
    o = fp.oracle_on_table(fp.standin_dump, "alpha_ns", p, fp.BRIDGE_N, dt=dt, max_steps=max_steps, seed=fp.BRIDGE_SEED, set_offset=0,
                           ext_sigma=0.1, bridge=True)
    share = o["undecided"].mean()
    print(f"undecided share dt={dt} cap={max_steps}: {o['undecided'].sum()} of {o['undecided'].size} = {share:.2e}")
    assert share <= fp.UNDECIDED_CAP
