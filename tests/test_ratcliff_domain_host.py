"""CPU tests of oracle section D (oracle/ddm_oracle.c: simulratcliff on the device stream, which the kernel's exact mode equals bit for
bit): the rows the sampler cannot sample are flagged, and inside the generator's box its law is the first-passage law in float64
(tests/wiener_cdf_ref.py).  tests/test_gpu_ratcliff_domain.py holds the kernel to the same checks."""
import numpy as np
import pytest

import oracle
import ratcliff_domain_cases as rc

SEED, N_SMALL = 2031, 8


def test_invalid_rows_are_flagged_not_simulated():
    p, bad, ok = rc.mixed_invalid_batch()
    so = (1 << 33) + 5
    r = oracle.philox_ratcliff(p, N_SMALL, seed=SEED, set_offset=so, ext_sigma=0.1, ext_mode=0, want_ext=True)
    rc.assert_rule_1(r, bad, N_SMALL)
    rc.assert_missing_is_nan_count(r)
    assert np.all(r["summary"][ok, 2] == 0) and not np.any(np.isnan(r["trials"][ok]))
    rc.assert_ext_formula(lambda q, mode: oracle.philox_ratcliff(q, N_SMALL, seed=SEED, set_offset=so, ext_sigma=0.1, ext_mode=mode,
                                                                 want_ext=True)["ext"], p, bad)
    # a good row does not see its neighbours: alone, at its own set index, it gives the same bits
    for b in ok:
        one = oracle.philox_ratcliff(p[b], N_SMALL, seed=SEED, set_offset=so + int(b), ext_sigma=0.1, ext_mode=0, want_ext=True)
        for k in ("trials", "summary", "ext"):
            assert rc.same_bits(one[k][0], r[k][b]), (b, k)


def test_boundary_starts_stay_valid():
    """Beta = 0 or 1: the trial ends at once on that boundary with a decision time of 0."""
    p = np.array([[8.0, 1.0, 0.0, 0.3, 0.0, 1.0], [-9.0, 1.0, 1.0, 0.3, 0.0, 1.0]], np.float32)
    r = oracle.philox_ratcliff(p, N_SMALL, seed=SEED)
    assert np.all(r["trials"][0] == (-np.float32(0.3), 0.0)) and np.all(r["trials"][1] == (np.float32(0.3), 1.0))
    assert np.array_equal(r["summary"][:, :3], [[0, N_SMALL, 0], [N_SMALL, 0, 0]])


def test_cap_hits_are_missing_on_the_ladder():
    """Nu 5, Eta 0, Alpha and Varsigma such that G on the first sphere is 6.2, 7.1, 8.0, 8.8 and 12.7: from ~7 on no attempt can be
    accepted (a = F (-ln s1) with -ln s1 <= 22.9), and the trial that runs into the attempt cap is missing, not a number."""
    N = 2000
    r = oracle.philox_ratcliff(rc.LADDER_ROWS, N, seed=5, set_offset=0, threads=8)
    rc.assert_missing_is_nan_count(r)
    miss = dict(zip(rc.LADDER_G, r["summary"][:, 2]))
    print("n_missing of", N, "by G:", miss)
    assert miss[6.2] == 0
    assert miss[8.0] > 0 and miss[8.8] > 0 and miss[12.7] > 0
    # what is left is a sample of trials that took no capped step: every one of them a number, at or after Tau
    y = r["trials"][..., 0]
    assert np.all(np.abs(y[~np.isnan(y)]) >= np.float32(0.3))
    # the moments are those of the trials that ended (float64 recomputation; the device sums the decision time in 2^-16 s)
    for b in range(len(rc.LADDER_ROWS)):
        rt = np.abs(y[b][~np.isnan(y[b])]).astype(np.float64)
        if len(rt):
            assert abs(r["summary"][b, 3] - rt.mean()) < 2e-5
        else:
            assert np.isnan(r["summary"][b, 3])


@pytest.mark.parametrize("seed", [5, 6])
def test_corner_law(seed):
    """The 48 corners of the generator's box, 20 000 trials each: no trial meets a cap (which is what keeps the KS honest), every row's
    KS distance from the float64 law is below 2.2 / sqrt(N), and the control -- the law of 1.03 Alpha -- is not."""
    r = oracle.philox_ratcliff(rc.CORNER_ROWS, rc.CORNER_N, seed=seed, set_offset=0, threads=8)
    assert np.all(r["summary"][:, 2] == 0) and not np.any(np.isnan(r["trials"]))
    rc.assert_corner_law(r["trials"][..., 0])
