"""Shared reference of the fast-mode parity tests (tests/test_gpu_fast_parity.py on the device, tests/test_fast_parity_host.py on the
CPU): the oracle run on an INJECTED Gaussian transform.

The fast mode differs from the exact mode in the Box-Muller factors (r, cos, sin) alone -- they come from the transcendental unit,
the radius in the unit sqrt(2 ln 2).  So a case's counters are built here, the factors at those counters are asked of a `dump`
(the device: engine.debug_normals(raw=True); without one: oracle.philox_raw), and oracle.philox_simulate reads them from the table
in place of its exact transform.  What comes back is what the fast kernels must write, bit for bit.

Counter layout (oracle/ddm_oracle.c: philox_one_set, aux_init): (set_lo, trial, set_hi28 | stream << 28, draw) -- stream 0 the path
noise with draw = index of the block's first step, stream 1 the auxiliary normals with draw = block index, trial 0xffffffff the set's
external datum."""
import numpy as np

MODELS = {"basic": 0, "single": 1, "alt": 2, "alpha_ns": 3, "explicit": 4}
AUX_BLOCKS = 17                  # MAX_REJECT = 64 rejection draws + the datum's: normals 0..64 = blocks 0..16
TABLE_BYTES = 256 << 20          # a case is split by sets so that one table stays below this


# the bridge cases: shared by the device test and by the CPU check of their undecided share.  48 x 300 = 14 400 trials: one undecided
# trial is 7e-5 of a case, below the 1e-4 the tests allow; two would not be
BRIDGE_CASES = [(0.01, 400.0), (0.001, 4000.0), (0.004, 1001.0)]
BRIDGE_B, BRIDGE_N, BRIDGE_SEED = 48, 300, 77
UNDECIDED_CAP = 1e-4


def case_params(model, B, seed):
    """Parameter rows of a case: the exact-mode parity tests' recipe (draws from the prior), and -- from 3 rows on -- the last two rows
    slow ones (no drift, boundary 2.5, diffusion coefficient 0.5: a mean first passage of 6 s), so that every case holds trials that run
    to the step cap, where a prior draw does so in under 1 % of its trials."""
    import prior_util
    if model == "basic":
        p, slow = prior_util.basic_prior(B, seed), {0: 0.0, 1: 2.5, 4: 0.5}
    elif model == "single":
        p, slow = prior_util.single_prior(B, seed, gamma=1.0), {0: 0.0, 1: 2.5, 4: 0.1, 5: 0.5}
    elif model == "alt":
        p, slow = prior_util.single_prior(B, seed, gamma=1.0), {0: 0.0, 1: 2.5, 4: 0.05, 5: 0.5}
        p[:, 4] = np.minimum(p[:, 4], 1.0)   # std_dc
    elif model == "alpha_ns":
        p, slow = prior_util.alpha_ns_prior(B, seed), {0: 0.0, 1: 2.5, 4: 0.1, 5: 0.5}
    else:
        p, slow = prior_util.basic_prior(B, seed)[:, [0, 2, 3, 4]], {0: 0.0, 3: 0.25}      # explicit: drift, beta, ter, dc (boundaries ~1.2)
    p = np.ascontiguousarray(p, np.float32)
    if B >= 3:
        for col, v in slow.items():
            p[-2:, col] = v
    return p


def case_bounds(B, N):
    return np.abs(np.random.default_rng(5).normal(1.2, 0.4, size=(B, N))).astype(np.float32)


def path_counters(set_offset, B, N, n_blocks, steps_per_block):
    """u32 [B * N * n_blocks, 4]: block j of trial t of set b."""
    sets = np.uint64(set_offset) + np.arange(B, dtype=np.uint64)
    c = np.empty((B, N, n_blocks, 4), np.uint32)
    c[..., 0] = (sets & np.uint64(0xffffffff)).astype(np.uint32)[:, None, None]
    c[..., 1] = np.arange(N, dtype=np.uint32)[None, :, None]
    c[..., 2] = ((sets >> np.uint64(32)) & np.uint64(0x0fffffff)).astype(np.uint32)[:, None, None]
    c[..., 3] = (np.arange(n_blocks, dtype=np.uint32) * np.uint32(steps_per_block))[None, None, :]
    return c.reshape(-1, 4)


def aux_counters(set_offset, B, N, n_blocks):
    """u32 [B * (N + 1) * n_blocks, 4]: block j of the auxiliary stream of trial t; row N of a set is trial 0xffffffff."""
    sets = np.uint64(set_offset) + np.arange(B, dtype=np.uint64)
    c = np.empty((B, N + 1, n_blocks, 4), np.uint32)
    c[..., 0] = (sets & np.uint64(0xffffffff)).astype(np.uint32)[:, None, None]
    c[..., 1] = np.concatenate([np.arange(N, dtype=np.uint32), np.array([0xffffffff], np.uint32)])[None, :, None]
    c[..., 2] = (((sets >> np.uint64(32)) & np.uint64(0x0fffffff)).astype(np.uint32) | np.uint32(0x10000000))[:, None, None]
    c[..., 3] = np.arange(n_blocks, dtype=np.uint32)[None, None, :]
    return c.reshape(-1, 4)


def device_dump(counters, k0, k1, form):
    """The device's fast transform at the counters: form 'hot' (the step loop's polar_pair), 'aux' (AuxStream's) or 'packed'."""
    from bayesflow_nddms_amd import engine
    return engine.debug_normals(counters, k0, k1, fast=True, raw=True, form=form)


def standin_dump(counters, k0, k1, form):
    """A float64 evaluation of the fast transform, for CPU checks of fast-mode arithmetic."""
    import oracle
    return oracle.philox_raw(counters, k0, k1, packed=(form == "packed"), standin=True)


def exact_dump(counters, k0, k1, form):
    """The oracle's own exact transform (with unit 1 the table run must reproduce the table-free oracle)."""
    import oracle
    return oracle.philox_raw(counters, k0, k1, packed=(form == "packed"), standin=False)


def build_table(dump, B, N, max_steps, seed, set_offset, packed=False, unit=None, fast=True):
    """The transform table of B sets from set_offset (oracle._table_args)."""
    import oracle
    k0, k1 = seed & 0xffffffff, (seed >> 32) & 0xffffffff
    ns = 8 if packed else 4
    n_path = max(1, -(-int(np.ceil(max_steps)) // ns))
    path = dump(path_counters(set_offset, B, N, n_path, ns), k0, k1, "packed" if packed else "hot")
    aux = dump(aux_counters(set_offset, B, N, AUX_BLOCKS), k0, k1, "aux")
    return {"path": path.reshape(B, N, n_path, 12 if packed else 6), "aux": aux.reshape(B, N + 1, AUX_BLOCKS, 6),
            "unit": oracle.FAST_UNIT if unit is None else np.float32(unit), "fast": fast}


def oracle_on_table(dump, model, params, N, dt, max_steps, seed, set_offset, bounds=None, ext_sigma=0.0, ext_mode=0, bridge=False,
                    packed=False, state_f64=False, unit=None, fast=True, threads=8):
    """oracle.philox_simulate (state_f64: philox_simulate_f64) of the case on the table `dump` gives, set chunk by set chunk.
    dict(trials, k, summary, [ext], [undecided]) over all B sets."""
    import oracle
    m = MODELS[model] if isinstance(model, str) else int(model)
    p = np.ascontiguousarray(params, np.float32)
    B = p.shape[0]
    ns = 8 if packed else 4
    n_path = max(1, -(-int(np.ceil(max_steps)) // ns))
    per_set = N * n_path * (12 if packed else 6) * 4 + N * n_path * 16          # table + counters, bytes
    chunk = max(1, min(B, TABLE_BYTES // per_set))
    parts = []
    for lo in range(0, B, chunk):
        hi = min(B, lo + chunk)
        tab = build_table(dump, hi - lo, N, max_steps, seed, set_offset + lo, packed=packed, unit=unit, fast=fast)
        if state_f64:
            r = oracle.philox_simulate_f64(m, p[lo:hi], N, dt=dt, max_steps=max_steps, seed=seed, set_offset=set_offset + lo, threads=threads,
                                           want_outputs=True, table=tab)
        else:
            r = oracle.philox_simulate(m, p[lo:hi], N, dt=dt, max_steps=max_steps, seed=seed, set_offset=set_offset + lo,
                                       bounds=None if bounds is None else bounds[lo:hi], ext_sigma=ext_sigma, ext_mode=ext_mode, bridge=bridge,
                                       packed=packed, want_k=True, want_ext=(m == 3), threads=threads, table=tab)
        parts.append(r)
        del tab
    return {k: np.concatenate([r[k] for r in parts]) for k in parts[0]}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits_nan_aware(a, b):
    """Summary columns as the exact-mode parity tests compare them: NaN where NaN, else equal bits."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(bits(np.nan_to_num(a)), bits(np.nan_to_num(b)))
