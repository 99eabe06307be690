#!/usr/bin/env python3
"""Writes tests/golden/wiener_survival.npz: log P(T > t) of basic_ddm_dc rows at 16 increasing times each, for the censoring tests
(tests/test_wiener_host.py without a GPU, tests/test_gpu_wiener_priors.py on one).  Where S >= 1e-3 the value is
wiener_cdf_ref.log_survival (log1p(-(F_lower + F_upper)) in float64); below it the survival series at the precision it needs
(wiener_ref.mp_log_survival, mpmath -- which the tests themselves do not import; `mp` marks those entries).

Rows: the four rows of the defect's report (wiener_cdf_ref.REPORTED_ROWS, k / 16 of their time) and the first ROWS_PER_SET rows of each set
of wiener_cdf_ref.censor_sets (the basic prior at a 1 s and a 4 s horizon, the shipped box at u in [1e-3, 50]).

Usage: python tests/golden/make_wiener_survival.py        (needs mpmath; about two minutes)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import wiener_cdf_ref as C  # noqa: E402
import wiener_ref as W  # noqa: E402

ROWS_PER_SET = 120


def main():
    k = np.arange(1, C.CENSOR_TIMES + 1, dtype=np.float64)[None, :] / C.CENSOR_TIMES
    params = [C.REPORTED_ROWS]
    rts = [C._times(C.REPORTED_ROWS, C.REPORTED_T[:, None] * k)[0]]
    rts[0][:, -1] = C.REPORTED_RT
    for name, (p32, rt32, _) in C.censor_sets(with_fixture=False).items():
        params.append(p32[:ROWS_PER_SET])
        rts.append(rt32[:ROWS_PER_SET])
    params, rt = np.concatenate(params).astype(np.float32), np.concatenate(rts).astype(np.float32)
    t = (rt - params[:, 3:4]).astype(np.float32).astype(np.float64)
    a, v, beta, _, s, _ = C.row_columns(params, True)
    log_s, ok = C.log_survival(t, a[:, None], v[:, None], beta[:, None], s[:, None])
    for i, j in zip(*np.nonzero(~ok)):
        log_s[i, j] = W.mp_log_survival(t[i, j], a[i], v[i], beta[i], s[i])
    assert np.all(np.isfinite(log_s)) and np.all(log_s <= 0) and np.all(np.diff(log_s, axis=1) <= 0)
    assert np.all(log_s[~ok] < np.log(C.S_FLOOR) + 1e-9)
    assert np.max(np.abs(log_s[np.arange(4), -1] - C.REPORTED_LOG_S)) < 1e-5
    np.savez(os.path.join(HERE, "wiener_survival.npz"), params=params, rt=rt, log_s=log_s, mp=~ok)
    print(f"{params.shape[0]} rows x {C.CENSOR_TIMES} times, {int((~ok).sum())} of {ok.size} from mpmath; most negative log S {log_s.min():.1f}")


if __name__ == "__main__":
    main()
