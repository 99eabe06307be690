/*
 * nddm.h -- C ABI of libnddm_hip.so: the MI355X (gfx950) Euler-Maruyama drift-diffusion
 * trial simulators that replace the numba/NumPy simulators of mdnunez/bayesflow_nddms.
 *
 * Each entry point is what a ctypes (or cffi / cgo / JNI) binding for the reference's
 * simulator path would bind.  File:line citations are relative to the reference repo.
 *
 * Conventions (all entry points):
 *   - every data pointer is a DEVICE pointer (hipMalloc / torch ROCm tensor .data_ptr());
 *     the caller allocates and frees all buffers; the library keeps no pointer after the
 *     call's work on `stream` has completed.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls are
 *     asynchronous with respect to the host: they enqueue work on `stream` and return.
 *     The handle is VALIDATED at entry (ABI 3): a destroyed stream, a stream created by another copy of the HIP runtime
 *     in the process, or an integer that never was a stream is refused with NDDM_ERR_HIP before anything is enqueued,
 *     and a stream of another device than the current one with NDDM_ERR_PARAM.  (HIP itself dereferences such a handle
 *     in hipStreamIsCapturing / hipEventRecord / the launch calls: a SIGSEGV in the caller's thread.)
 *   - parameter rows are row-major float32 [B, P] in the REFERENCE'S parameter order.
 *   - trial output is row-major float32 [B, n_trials, 2]; summary output float32 [B, NDDM_SUMMARY_K].
 *     Either may be NULL (summary-only mode never writes the 8 bytes per trial).
 *   - randomness is a pure function of (seed, set_offset + row, trial, draw): output does not
 *     depend on launch geometry, on how rows are sharded over GPUs, or on call order.
 *   - timeouts are data (choice 0 / choicert 0), never errors.
 *   - return value: NDDM_OK or an nddm_status; nddm_last_error() gives thread-local text.
 *   - re-entrant and thread-safe given distinct output buffers: any number of host threads may call on any streams
 *     concurrently.  The device memory a launch needs besides the caller's buffers (work-queue words, scratch) is owned by
 *     that launch until the work it enqueued has COMPLETED (reuse is keyed on stream order or on a completion event, never
 *     on a launch count); the developer knobs (nddm_set_tuning, nddm_set_debug_trace) are read once, atomically, at entry.
 *   - hipGraph: a call made while `stream` is capturing is recorded as kernels only; the memory such a launch needs is
 *     allocated for that launch alone and belongs to the GRAPH ARENA bound to the capturing thread (nddm_graph_arena_*;
 *     released with its owner, and with nothing else) or, with no arena bound, to an ownerless list that
 *     nddm_release_graph_memory() frees.  Seed and set_offset are baked in;
 *     nddm_simulate_indirect / nddm_draw_prior_indirect add a 64-bit offset read from DEVICE memory when the kernels run,
 *     so a replayed graph moves along the random stream (a captured `*dev += B` between replays).
 *
 * Deliberate deviations from the boundary sketched for this path:
 *   - arithmetic is float32 on the device (state w, the Gaussian transform) with an INTEGER step index, so
 *     rt = k*dt + tau is exact in k; the reference integrates in float64.  Parity with the reference is therefore
 *     distributional (KS < 0.01 on the integer step grid), and bit-for-bit only against the float32 oracle (oracle/).
 *     The deviation as a number: fed the SAME normals, the float32 integrator and the reference's float64 recurrence
 *     (basic_ddm_dc.py:91-103) end a trial on another (step index, choice) in 7.6e-5 of 2 000 000 prior-mixture trials at
 *     dt=.001 / max_steps 4000 (1.5e-4 on the 18 fixed parameter sets) and in 4e-6 at the reference default dt=.01 / 400;
 *     the choice differed in none of them; a differing trial is a grazed boundary one arithmetic counts as crossed and the
 *     other does not, after which it runs on (largest step-index difference seen: 652)
 *     (oracle/ddm_oracle.c: oracle_philox_simulate_f64; tests/test_oracle_golden.py::test_f32_integrator_against_the_reference_f64_recurrence).
 *     Since ABI 4 the deviation is an option rather than a given: with NDDM_STATE_F64 (enum nddm_flags) the basic and single-trial
 *     simulators carry the evidence in float64 exactly as the reference's recurrence does, and their (step, choice) equal that
 *     function's bit for bit.
 *     Parameters are taken as float32 [B, P]; there is no float64 input form.
 *   - there are no `*_cpu` twins in this library: the CPU restatement of the same stream is test infrastructure
 *     (oracle/ddm_oracle.c) and is never linked into, or reachable from, the product.  Without a ROCm device every entry
 *     point fails with NDDM_ERR_HIP / NDDM_ERR_NO_DEVICE.
 */
#ifndef NDDM_H
#define NDDM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: the default Gaussian stream takes the angle from the LOW 23 bits of its word (round 2), the bridge-uniform stream
 *    serves 8 steps per block (round 3), nddm_set_debug_counters became nddm_set_debug_trace, and the *_indirect entry
 *    points, nddm_simulate_codes / nddm_decode_codes and nddm_source_hash exist.  The same (seed, set_offset) gives different bits under ABI 1. */
/* 3: memory behind captured launches has an owner (nddm_graph_arena_create / _bind / _info / _release); nddm_release_graph_memory
 *    frees only what was captured with no arena bound (up to ABI 2: every captured launch's memory on the device, whoever's graph
 *    replayed into it); a `stream` the HIP runtime does not know is refused with NDDM_ERR_HIP (validated with hipStreamGetDevice at entry).  The random stream is ABI 2's. */
/* 4: NDDM_STATE_F64 (flag 8), nddm_build_info, nddm_simulratcliff.  The random stream and every ABI-3 entry point are unchanged. */
/* 4 (additive): nddm_wiener_log_likelihood.  No existing entry point changes. */
/* 4 (additive): nddm_wiener_cdf.  No existing entry point changes. */
/* 4 (additive): nddm_wiener_quantile. */
/* 4 (additive): nddm_wiener_log_likelihood_grad.  No existing entry point changes. */
/* 4 (additive): nddm_wiener_marginal_log_likelihood.  No existing entry point changes. */
/* 4 (additive): nddm_wiener_marginal_log_likelihood_grad.  No existing entry point changes. */
/* 4 (additive): nddm_wiener_hmc.  No existing entry point changes. */
/* 4 (additive): nddm_wiener_hmc_joint.  No existing entry point changes. */
/* 4 (additive): NDDM_WIENER_CENSORED (flag 4 of nddm_wiener_log_likelihood_grad, nddm_wiener_hmc and nddm_wiener_hmc_joint).  With the
 *    flag clear no output changes. */
/* 4 (additive): nddm_wiener_marginal_log_likelihood_ragged.  No existing entry point changes. */
#define NDDM_ABI_VERSION 4
#define NDDM_SUMMARY_K 10

/* summary_stats[b, :] (single_trial_alpha_not_scaled.py:205-211,
 * simulations/mean_RT_accuracy_effects.py:88-90, simulations/Basic_DDM_simulations.py:137-145) */
enum nddm_summary_col {
    NDDM_S_N_UPPER = 0,       /* trials that hit the upper boundary (choice  1) */
    NDDM_S_N_LOWER = 1,       /* trials that hit the lower boundary (choice -1) */
    NDDM_S_N_MISSING = 2,     /* trials that reached max_steps (choice 0) */
    NDDM_S_MEAN_RT = 3,       /* mean RT (incl. non-decision time) of responded trials; NaN if none */
    NDDM_S_VAR_RT = 4,        /* population variance (ddof=0) of the same */
    NDDM_S_MEAN_RT_UPPER = 5, /* EZ-diffusion MRT: mean RT of upper-boundary trials; NaN if none */
    NDDM_S_VAR_RT_UPPER = 6,  /* EZ-diffusion VRT */
    /* The two z columns come from fixed-point sums -- sum z in units of 2^-32, sum z^2 in units of 2^-24, every term truncated towards
     * zero, z clamped at +-2^18 -- so that they are bit-reproducible whatever the launch geometry.  With ref the float64 value over the
     * float32 z1 that are written:  |mean_z - ref| <= 2^-32 + ulp32(ref) / 2,  |var_z - ref| <= 2^-24 + 2 |mean_z| 2^-32 + ulp32(ref) / 2.
     * A var_z below about 1e-5 is therefore only good to a few percent (and below 6e-8 to nothing).  Variances are never negative:
     * var_z is clamped at 0 (the truncation can leave sum z^2 / N below mean^2: one trial, or sigma1 ~ 1e-5 and gamma = 0); the RT
     * variances are formed in float64 from exact integer sums and are within 1 float32 ulp of the exact value of the trials written
     * (tests/test_gpu_summary.py), an exact 0 included. */
    NDDM_S_MEAN_Z = 7,        /* mean external datum z1 over all trials (0 for models without z1) */
    NDDM_S_VAR_Z = 8,         /* population variance of z1, >= 0 */
    NDDM_S_CHOICE_MEAN = 9    /* mean(.5 + .5*sign(choicert)) over all trials */
};

enum nddm_model {
    NDDM_BASIC_DDM_DC = 0,     /* basic_ddm_dc.py:85-125; P=5: drift, boundary, beta, tau, dc */
    NDDM_SINGLE_TRIAL = 1,     /* single_trial_alpha_not_scaled.py:107-155 (+_scale :1237-1285, _scale2 :1471-1519);
                                  P=8: drift, mu_alpha, beta, ter, std_alpha, dc, sigma1, gamma (gamma=1 for the base model) */
    NDDM_SINGLE_TRIAL_ALT = 2, /* single_trial_alpha_not_scaled.py:926-974; P=8: drift, alpha, beta, ter, std_dc, mu_dc, sigma1, gamma */
    NDDM_ALPHA_NOT_SCALED = 3, /* alpha_not_scaled.py:52-128 as an Euler-Maruyama process; P=6: Nu, Alpha, Beta, Tau, Eta, Varsigma */
    NDDM_EXPLICIT_BOUNDARY = 4 /* imputation_from_stahl_not_scaled.py:120-148; P=4: drift, beta, ter, dc; bounds[B, n_trials] */
};

enum nddm_status {
    NDDM_OK = 0,
    NDDM_ERR_NULL = 1,        /* a required pointer is NULL */
    NDDM_ERR_SHAPE = 2,       /* B < 0, n_trials <= 0, max_steps < 0, or B * ceil(n_trials / 512) >= 2^31 */
    NDDM_ERR_PARAM = 3,       /* non-finite or non-positive dt; unknown model / flag */
    NDDM_ERR_HIP = 4,         /* a HIP runtime call failed; text in nddm_last_error() */
    NDDM_ERR_NO_DEVICE = 5
};

enum nddm_flags {
    NDDM_GAUSS_EXACT = 0,     /* Box-Muller from IEEE add/mul/fma/sqrt only: bit-reproducible on a CPU (oracle) */
    NDDM_GAUSS_FAST = 1,      /* Box-Muller on v_log_f32 / v_sqrt_f32 / v_sin_f32 / v_cos_f32 */
    NDDM_GAUSS_PACKED = 4,    /* opt-in, with either transform, not with NDDM_BRIDGE, max_steps < 2^14: one 32-bit Philox word per
                                 Box-Muller pair (16-bit radius uniform + 16-bit angle) instead of two, i.e. 8 normals per
                                 Philox block instead of 4 -- ~25 % faster.  The path noise then has |z| <= 5.65 and a 2^-16
                                 grid in the radius; a different (equally reproducible) random stream than the default */
    NDDM_STATE_F64 = 8,       /* (ABI 4; NDDM_BASIC_DDM_DC and NDDM_SINGLE_TRIAL, not with NDDM_BRIDGE / NDDM_GAUSS_PACKED / the wire format)
                                 the REFERENCE'S state arithmetic: the evidence is a float64 in its natural units,
                                 evidence += drift*dt + sqrt(dt)*dc*normal (basic_ddm_dc.py:91-103; single_trial_alpha_not_scaled.py:113-128),
                                 every operation a separate IEEE double operation in the reference's order, the loop condition
                                 (evidence > 0) && (evidence < boundary) on doubles; `normal` is the exact double product of the float32
                                 Box-Muller radius and cosine / sine of the same random stream.  With NDDM_GAUSS_EXACT the (step index,
                                 choice) of every trial equals oracle_philox_simulate_f64's bit for bit (oracle/ddm_oracle.c), i.e. the
                                 float32-state deviation stated at the top of this file becomes a measured option; the single-trial
                                 model's boundary is formed in double from the same auxiliary normals, its external datum z1 stays the
                                 float32 expression.  Costs ~25-30 % of the rate (4 extra double operations per step). */
    NDDM_BRIDGE = 2           /* (alpha_not_scaled only) Brownian-bridge boundary correction: between two grid points
                                 inside (0, a) the path crosses a boundary with probability exp(-2 d0 d1 / (sigma^2 dt));
                                 removes the O(sqrt(dt)) late-detection bias of plain Euler-Maruyama against the exact
                                 first-passage sampler the reference uses for this model (pyhddmjagsutils.py:47-176);
                                 RTs get a uniform sub-step jitter, (k - U) dt, instead of k dt */
};

/* ---- library / device ------------------------------------------------------------- */
int nddm_abi_version(void);
const char *nddm_last_error(void);
int nddm_device_count(int *count);
int nddm_set_device(int device);
int nddm_summary_k(void);
int nddm_model_nparams(int model); /* P of enum nddm_model, -1 if unknown */
/* ---- memory behind launches captured into hipGraphs ---------------------------------------------------------------------
 * A captured launch cannot borrow the library's per-launch memory (the graph replays at times the library cannot see): it gets
 * an allocation of its own (two queue words + its scratch, <= 64 MB).  That allocation is charged to the graph arena that is
 * bound to the CAPTURING THREAD at the time of the call:
 *     uint64_t a;  nddm_graph_arena_create(&a);
 *     nddm_graph_arena_bind(a, &prev);  ... hipStreamBeginCapture / nddm_* calls / hipStreamEndCapture ...  nddm_graph_arena_bind(prev, NULL);
 *     ... replay the graphs ...;  destroy them;  nddm_graph_arena_release(a);
 * The caller of nddm_graph_arena_release asserts that every graph that captured a launch under THIS arena has been destroyed
 * (or will not be replayed); graphs captured under other arenas -- a second trainer (the checkpointed, re-entered training of
 * basic_ddm_dc.py:169-176, 199-207 keeps more than one alive in a notebook), a user's own graph -- are not affected.
 * The binding is per host thread; arena 0 = no owner.  A capture made while a RELEASED arena is still bound is refused
 * (NDDM_ERR_PARAM).  nddm_graph_arena_info: bytes / allocations currently charged to an arena (0 = the ownerless list). */
int nddm_graph_arena_create(uint64_t *arena);
int nddm_graph_arena_bind(uint64_t arena, uint64_t *previous /* may be NULL */);
int nddm_graph_arena_info(uint64_t arena, uint64_t *bytes /* may be NULL */, int32_t *n_allocations /* may be NULL */);
int nddm_graph_arena_release(uint64_t arena);
/* frees the OWNERLESS memory of the current device: what launches captured with no arena bound were given; call only when every
 * such graph has been destroyed.  Never touches an arena's memory. */
int nddm_release_graph_memory(void);
/* testing aid (not part of the drop-in surface): cap the number of launch slots per device, so that a test can drive the
 * library into queueing a launch behind an in-flight one */
int nddm_debug_set_slot_limit(int n);
/* developer aid: geometry of the calling thread's last simulator launch, out[8] = {grid waves, 1 if the kernel variant with
 * the Philox round keys in VGPRs ran, ring slots, trials per tile, tiles per set, sets per chunk, refill threshold, dynamic
 * LDS bytes}.  bench.py uses it to run its lockstep ceiling on the same kernel variant and grid as the timed workload. */
int nddm_debug_last_launch(int32_t *out8);
/* developer knobs of the launch geometry (0 = the library's rule): sets per queue chunk, ring slots (>= 2),
 * refill threshold (lanes holding a finished trial; >= 64 = refill only when no lane is stepping), kernel variant (1 =
 * Philox round keys from LDS, 2 = in VGPRs, taken modulo 3), grid in waves, trials per tile.  Results never depend on
 * them (tests/test_gpu_fuzz.py randomises all six). */
int nddm_set_tuning(int sets_per_chunk, int ring, int refill_thresh, int variant, int grid_waves, int tile_trials);
/* 0 switches the longest-first ordering pre-pass off (sets are processed in the given order) */
int nddm_set_ordering(int enabled);
/* benchmarking aid: the two-ended work queue.  The waves of a launch pull chunks of sets from one queue; the last waves of the
 * grid (the ones a full SIMD serves last) may pull from its BACK -- the shortest expected trials of a sorted launch -- so that
 * none of them is left holding a chunk of long trials when the queue runs dry.  back_waves: -1 = the library's rule (a fraction
 * of the grid, for sorted launches on the full resident grid with enough chunks per wave), 0 = every wave pulls from the front,
 * n > 0 = the last n waves of whatever grid is launched, clamped to the grid.  Results never depend on it. */
int nddm_set_queue_split(int back_waves);
/* profiling aid: while set, every wave of the simulator kernels stores -- plain stores, no atomics -- one 8-word record
 * at buf[8 w ..], w = workgroup < wave_capacity: {step-loop blocks, refill phases, s_memtime cycles, lifetime, start, "found
 * the queue empty", end in s_memrealtime ticks (100 MHz), 1}; and the tick at which chunk c < chunk_capacity was pulled
 * at buf[8 wave_capacity + c].  buf: device u64 [8 wave_capacity + chunk_capacity], zeroed by the caller; NULL = off. */
int nddm_set_debug_trace(void *dev_u64, int wave_capacity, int chunk_capacity);

/* ---- simulators --------------------------------------------------------------------
 * Common arguments:
 *   params      device f32 [B, P]
 *   B           number of parameter sets (rows)
 *   n_trials    trials per set (the batch-shared N of basic_ddm_dc.py:50-52, 131); any size: sets with more than
 *               512 trials are split into tiles internally, with results independent of the split
 *   dt          Euler-Maruyama step (reference default .01, basic_ddm_dc.py:87; fine study .001, single_trial_alpha_not_scaled.py:1719)
 *   max_steps   step cap (reference default 400; 4000 in the fine study)
 *   seed        64-bit stream key
 *   set_offset  global index of row 0 (makes shards of one logical batch reproducible); set_offset + row must stay
 *               below 2^60 (the random stream is keyed by the low 60 bits of the global set index)
 *   flags       enum nddm_flags
 *   out_trials  device f32 [B, n_trials, 2] or NULL
 *   out_summary device f32 [B, NDDM_SUMMARY_K] or NULL
 */

/* replaces simulate_trials(params, n_trials), basic_ddm_dc.py:114-125 (batched over B sets).
 * out_trials[b, i, :] = (rt, choice); choice in {1, -1, 0 (timeout; the reference's unbound-variable
 * bug at basic_ddm_dc.py:110-111 is resolved to 0)}; rt = n_steps*dt + tau. */
int nddm_basic_ddm_dc_simulate(const float *params, int64_t B, int32_t n_trials, float dt, int32_t max_steps,
                               uint64_t seed, uint64_t set_offset, uint32_t flags, float *out_trials,
                               float *out_summary, void *stream);

/* replaces simulate_trials / simulate_trials_fine / simulate_trials_scale / _scale2,
 * single_trial_alpha_not_scaled.py:144-155, :1710-1722, :1274-1285, :1508-1519.
 * out_trials[b, i, :] = (choicert, z1); choicert = +-(ter + rt) or 0; z1 ~ N(gamma*bound_trial, sigma1). */
int nddm_single_trial_simulate(const float *params, int64_t B, int32_t n_trials, float dt, int32_t max_steps,
                               uint64_t seed, uint64_t set_offset, uint32_t flags, float *out_trials,
                               float *out_summary, void *stream);

/* replaces simulate_trials_alt, single_trial_alpha_not_scaled.py:963-974 (per-trial diffusion coefficient).
 * out_trials[b, i, :] = (choicert, z1); z1 ~ N(gamma*dc_trial, sigma1). */
int nddm_single_trial_alt_simulate(const float *params, int64_t B, int32_t n_trials, float dt, int32_t max_steps,
                                   uint64_t seed, uint64_t set_offset, uint32_t flags, float *out_trials,
                                   float *out_summary, void *stream);

/* the data generator of alpha_not_scaled.py:52-128 as an Euler-Maruyama process: per-trial drift
 * ~ N(Nu, Eta) (pyhddmjagsutils.py:124-125), noise Varsigma, one external datum per set
 * out_extdata[b] = (ext_mode == 0 ? Alpha[b] : 1) + ext_sigma * N(0,1)  (alpha_not_scaled.py:103-106).
 * out_trials[b, i, :] = (y, acc): y = +-rt signed by the response (:98-100), acc = (sign(y)+1)/2 (:102).
 * out_extdata: device f32 [B] or NULL. */
int nddm_alpha_not_scaled_simulate(const float *params, int64_t B, int32_t n_trials, float dt, int32_t max_steps,
                                   uint64_t seed, uint64_t set_offset, uint32_t flags, float ext_sigma,
                                   int32_t ext_mode, float *out_trials, float *out_summary, float *out_extdata,
                                   void *stream);

/* replaces simulratcliff(N, Alpha, Tau, Nu, Beta, Eta=, Varsigma=), pyhddmjagsutils.py:47-176, as alpha_not_scaled.py:95-108 calls it
 * (rangeTau = rangeBeta = 0): the EXACT first-passage sampler of the diffusion model with per-trial drift ~ N(Nu, Eta) and diffusion
 * coefficient Varsigma (Tuerlinckx et al. 2001: random walk on spheres with rejection) -- the generator config 3's reference actually
 * runs.  No step size: nothing to discretise, no KS caveat.  (ABI 4)
 *   params       device f32 [B, 6] = Nu, Alpha, Beta, Tau, Eta, Varsigma (Nu is clipped to +-5 as :102-103 does)
 *   flags        NDDM_GAUSS_EXACT (every rounding spelled out, the reference's series term by term: equal bit for bit to
 *                oracle/ddm_oracle.c section D) or NDDM_GAUSS_FAST (v_log_f32 / v_exp_f32 / v_rcp_f32, and the SAME acceptance function
 *                from three terms of its series or of the series' Jacobi-dual form, whichever converges: no loop; on 6e6 trials no
 *                response differs from the exact mode's and no response time by more than 1e-6 s); nothing else
 *   out_trials   [B, n_trials, 2] = (y, acc): y = +-(Tau + decision time) signed by the response, acc = (sign + 1) / 2  (:98-102)
 *   out_summary  [B, NDDM_SUMMARY_K] from integer sums of the decision time in 2^-16 s; n_missing counts the trials written (NaN, NaN)
 *   out_extdata  [B]: (ext_mode == 0 ? Alpha[b] : 1) + ext_sigma * N(0,1)  (alpha_not_scaled.py:103-106), as nddm_alpha_not_scaled_simulate
 * Randomness: per-trial drift = auxiliary normal 0 of (set, trial) -- the draw the Euler-Maruyama form uses -- and stream 3 of the
 * trial for the sampler's uniforms; a pure function of (seed, set_offset + row, trial).  Sets of more than 512 trials are tiled
 * (same bits); with summaries such a launch cannot be captured into a hipGraph.
 * What cannot be sampled is flagged, never returned as a number (both modes):
 *   1. an invalid row -- a non-finite column, Alpha <= 0, Varsigma <= 0, Beta outside [0, 1], Eta < 0 -- is not simulated: every trial
 *      (NaN, NaN), n_upper = n_lower = 0, n_missing = n_trials, moments NaN; out_extdata keeps its formula.  Beta = 0 or 1 is valid;
 *   2. a trial that reaches one of the sampler's loop caps (4096 rejection attempts on a sphere, 4096 spheres) is (NaN, NaN) and counted
 *      in n_missing only.  The rejection step cannot accept once G = r mu / (D pi) passes ~7 (r = Alpha min(Beta, 1 - Beta), mu the
 *      trial's drift, D = Varsigma^2 / 2): rows with G below ~6 -- the generator's box but for its extreme corner's drift tail -- are
 *      the domain; Nu 5, Alpha 2, Varsigma .6 (G 8.8) loses 62 % of its trials.  csrc/nddm_ratcliff.h, DESIGN.md 5.5. */
int nddm_simulratcliff(const float *params, int64_t B, int32_t n_trials, uint64_t seed, uint64_t set_offset, uint32_t flags,
                       float ext_sigma, int32_t ext_mode, float *out_trials, float *out_summary, float *out_extdata, void *stream);

/* ---- likelihood ---------------------------------------------------------------------------------------------------------
 * replaces the Wiener first-passage density the reference's likelihood-based fits evaluate per trial: JAGS
 * dwiener(alpha/varsigma, ndt, beta, delta/varsigma) (basic_ddm_dc_pyjags.py:129-133, alpha_not_scaled.py:170-176, jagscode/*.jags) and
 * Stan wiener_lpdf inside diffusion_lpdf(Y | boundary, ter, bias, drift, dc) (basic_ddm_dc_pystan2.py:119-131, :170-175,
 * stancode/basic_ddm_dc_test.stan) -- the per-trial log density, not the samplers around it.  (ABI 4, additive)
 *   model              NDDM_BASIC_DDM_DC (P=5) or NDDM_ALPHA_NOT_SCALED (P=6, drift ~ N(Nu, Eta) integrated out, Nu clipped to +-5);
 *                      any other model: NDDM_ERR_PARAM
 *   params             device f32 [R, P] in the simulator's parameter order; R = D * draws_per_dataset
 *   draws_per_dataset  S: row r is scored against data set r / S (S = 1: a simulator batch under its own parameters; D = 1 and S large:
 *                      posterior draws against one observed data set -- the data set is staged in LDS once per 16 rows)
 *   data               device f32 [D, n_trials, 2] in the simulator's own output format: (rt, choice) for basic (choice 0 = a timeout,
 *                      scored RIGHT-CENSORED as log P(T > rt - tau)), (y, acc) for alpha_not_scaled (y == 0 carries no time: NaN)
 *   flags              0 (reserved)
 *   out_trial_logp     device f32 [R, n_trials] or NULL: log f of every trial (natural log; rt <= tau gives -inf)
 *   out_loglik         device f64 [R] or NULL (not both NULL): the row's sum, accumulated in float64 in an order that depends on n_trials
 *                      alone -- the same bits for a row whatever the layout, launch, stream or capture
 * A row with a non-finite parameter, boundary or diffusion coefficient <= 0, beta outside (0, 1), tau < 0 or eta < 0 gives NaN for its
 * trials and its sum; the other rows are unaffected.  No scratch memory: a call made while `stream` is capturing is one kernel node.
 * Errors (checked before any HIP call): NDDM_ERR_SHAPE for R < 0, n_trials <= 0, draws_per_dataset <= 0 or not dividing R;
 * NDDM_ERR_NULL for a NULL params / data or both outputs NULL; R = 0 is NDDM_OK.  The math: csrc/nddm_wiener.h, DESIGN.md section 11. */
int nddm_wiener_log_likelihood(int32_t model, const float *params, int64_t R, int64_t draws_per_dataset, const float *data,
                               int32_t n_trials, uint32_t flags, float *out_trial_logp /* [R, n_trials] or NULL */,
                               double *out_loglik /* [R] or NULL */, void *stream);

/* The same log-likelihood AND its gradient in the model's parameter columns, one fused launch: what a gradient-based fit consumes per
 * step (Stan's NUTS over wiener_lpdf, MAP refinement, Laplace / variational fits, HMC or MALA on many data sets at once).  (ABI 4, additive)
 *   model, params, draws_per_dataset, data, n_trials: exactly as nddm_wiener_log_likelihood takes them
 *   flags              0 or NDDM_WIENER_CENSORED (basic_ddm_dc only: with NDDM_ALPHA_NOT_SCALED, whose y == 0 carries no time, it is
 *                      NDDM_ERR_PARAM); any other value: NDDM_ERR_PARAM
 *   out_loglik         device f64 [R] or NULL: the row's log-likelihood, BIT FOR BIT nddm_wiener_log_likelihood's out_loglik
 *   out_grad           device f64 [R, P] (NULL: NDDM_ERR_NULL): d out_loglik[r] / d params[r, j], in params' column order; alpha_not_scaled's Nu
 *                      is clipped to +-5: where the clip is active the Nu column is 0 and the others are those of the clipped value
 * Special values (none an error): an invalid row (nddm_wiener_log_likelihood's conditions) gives NaN in out_loglik and in every gradient
 * column, the other rows unaffected; a trial with rt <= tau (-inf in the value) or an alpha_not_scaled y == 0 (NaN in the value) gives NaN
 * in every gradient column of its row.
 * NOT IMPLEMENTED: the gradient of basic_ddm_dc's censored timeouts (choice 0) under flags 0.  out_loglik scores them exactly as
 * nddm_wiener_log_likelihood does (log P(T > rt - tau)), whatever the flags; with flags 0 the row's gradient is NaN in EVERY column,
 * never a partial gradient.  IMPLEMENTED, opt-in, under NDDM_WIENER_CENSORED (the default keeps every bit it had): there a
 * timeout adds the gradient of log P(T > rt - tau) -- in tau it is +(f_lower + f_upper) / S -- and the row's gradient is finite; a timeout
 * with rt <= tau is log 1 = 0 with a zero gradient; a non-finite rt, or a choice other than 1, -1 and 0, gives NaN in every gradient
 * column of its row.  Where no trial is a timeout the flag changes no bit of either output.
 * The bits of both outputs are a function of (the row's parameters, its data set, n_trials) alone: the same whatever the layout, the
 * draws_per_dataset factorisation, the stream or a capture.  No scratch memory, no atomics: a call made while `stream` is capturing is one
 * kernel node.  Error checks, their order and their status codes are nddm_wiener_log_likelihood's; R = 0 is NDDM_OK.  The math:
 * csrc/nddm_wiener_grad.h, DESIGN.md section 14. */
int nddm_wiener_log_likelihood_grad(int32_t model, const float *params, int64_t R, int64_t draws_per_dataset, const float *data,
                                    int32_t n_trials, uint32_t flags /* 0 or NDDM_WIENER_CENSORED */, double *out_loglik /* [R] or NULL */,
                                    double *out_grad /* [R, P] */, void *stream);

/* nddm_wiener_log_likelihood_grad, nddm_wiener_hmc, nddm_wiener_hmc_joint: score basic_ddm_dc's censored timeouts in the gradient and
 * in the samplers' posterior.  (4: the one value free in the flags of all three, whose 1, 2 and 3 are taken or refused by name.) */
#define NDDM_WIENER_CENSORED 4u

/* Batched Hamiltonian Monte Carlo over the basic_ddm_dc posterior of the reference's JAGS fit (basic_ddm_dc_pyjags.py:103-137), one wave per
 * chain, all the iterations of the call in one launch.  (ABI 4, additive)
 *   model              NDDM_BASIC_DDM_DC only (NDDM_ERR_PARAM otherwise); columns (drift, boundary, beta, tau, dc)
 *   data               device f32 [D, n_trials, 2] = (rt, choice), n_trials <= 2048; chain c samples data set c / chains_per_dataset,
 *                      C = D * chains_per_dataset
 *   state              device f64 [C, 12], in and out: q[5] (unconstrained: drift = q0, a bounded column theta = lo + (hi - lo) sigmoid(q);
 *                      a FIXED column's slot holds theta itself), log eps, log eps-bar, H-bar, mu, adapting iterations done, then two
 *                      words the chain only reports in: the last iteration's energy error H1 - H0 and the largest finite |H1 - H0| so far
 *   inv_mass           device f64 [C, 5] or NULL (ones): momentum p_j ~ N(0, 1 / inv_mass_j)
 *   n_iter, n_leapfrog, thin > 0, n_adapt >= 0: a chain adapts log eps by dual averaging (target .8) while its state counts fewer than
 *                      n_adapt adapting iterations.  One launch is bounded: n_iter * n_leapfrog * ceil(n_trials / 64) <= 2^19 (about 1.2 s)
 *   free_mask          bit j set: column j is sampled; clear: it keeps its value (no momentum, prior or Jacobian term).  < 32
 *   seed, chain_offset, iter_offset: Philox key and the global indices (both < 2^32) of chain 0 and of this call's first iteration.  A
 *                      chain's output is a pure function of (seed, global chain index, its data set, its incoming state, inv_mass,
 *                      free_mask, n_leapfrog, thin, n_adapt, the iteration range): a run continued from a returned state with iter_offset
 *                      advanced gives the bits of the uncut run, whatever else is in the launch
 *   flags              0 or NDDM_WIENER_CENSORED: a choice-0 trial (the simulator's timeout) is a trial, scored right-censored as
 *                      log P(T > rt - tau) in the posterior and its gradient; tau's upper limit is then min(1.5, the smallest rt of the
 *                      RESPONSES) (1.5 without one).  With no choice-0 trial in the data the flag changes no bit.  Other values: NDDM_ERR_PARAM
 *   outputs, each may be NULL, not all: out_draws f32 [C, K, 5] in theta and out_log_post f32 [C, K] (the log posterior in q, Jacobian
 *                      included, up to an additive constant), K = (iter_offset + n_iter) / thin - iter_offset / thin, global iteration g
 *                      kept when (g + 1) % thin == 0; out_accept f32 [C]: the mean acceptance probability of this call's non-adapting
 *                      iterations (NaN: none); out_divergent i32 [C]: rejections with a non-finite or > 1000 energy error;
 *                      out_flagged i32 [C]
 * Priors: drift N(0, 2^2); boundary N(1, .5^2) on (0, 10); beta Beta(2, 2); tau N(.5, .25^2) on (0, min(1.5, smallest rt)); dc N(1, .5^2)
 * on (0.05, 10) -- the floor is a deviation from JAGS's (0, 10).  A chain whose data set holds a choice-0 trial (without
 * NDDM_WIENER_CENSORED), any other choice than 1 and -1, a non-finite value or an
 * rt <= 0, or whose incoming state (or inverse mass) is not finite, is FLAGGED: no iteration, NaN draws, out_flagged = 1, state unchanged,
 * the other chains unaffected.  Error checks, their order and their status codes are nddm_wiener_log_likelihood's (a chain is a row); C = 0
 * is NDDM_OK.  No scratch memory, no atomics.  The chain: csrc/nddm_wiener_hmc.h, DESIGN.md section 17. */
int nddm_wiener_hmc(int32_t model, const float *data /* [D, n_trials, 2] */, int64_t D, int32_t n_trials, int64_t C,
                    int64_t chains_per_dataset, double *state /* [C, 12] */, const double *inv_mass /* [C, 5] or NULL */, int32_t n_iter,
                    int32_t n_adapt, int32_t n_leapfrog, int32_t thin, uint32_t free_mask, uint64_t seed, uint64_t chain_offset,
                    uint64_t iter_offset, uint32_t flags /* 0, reserved */, float *out_draws, float *out_log_post, float *out_accept,
                    int32_t *out_divergent, int32_t *out_flagged, void *stream);

/* The alpha_not_scaled JAGS fit (alpha_not_scaled.py:138-259): nddm_wiener_hmc's chains coupled by one shared sigma.  Participant p has
 * nddm_wiener_hmc's posterior plus an external measurement extdata[p] ~ N(boundary_p, sigma); sigma ~ N(3, 1) on (0, 10) is shared by all P
 * participants of a joint chain.  Metropolis within Gibbs, n_iter joint iterations per call: per iteration one participant kernel (one
 * iteration of nddm_wiener_hmc's chain for every (p, k), the log posterior gaining -(ext_p - boundary_p)^2 / (2 sigma_k^2)) and then one
 * sigma kernel (an independence Metropolis step on sigma_k's conditional) are enqueued on `stream`, after one pre-pass kernel: 2 n_iter + 1
 * launches, no host synchronisation, no cooperative launch, no atomics.  (ABI 4, additive)
 *   arguments as nddm_wiener_hmc's, D = P participants, chains_per_dataset = S joint chains, C = P * S, participant chain c = p * S + k, and
 *   extdata            device f64 [P]
 *   sigma              device f64 [S], in and out
 *   workspace          device f64 [P * S + S, 4], the caller's: the call's accept and divergence accumulators.  The entry allocates nothing
 *   flags              0 or NDDM_HMC_SIGMA_FIXED: sigma is held and no sigma kernel is launched; either with NDDM_WIENER_CENSORED
 *                      (flags 4, 5), which nddm_wiener_hmc's chains take as that entry does; 2 and 3 are NDDM_ERR_PARAM
 *   n_iter             <= 4096 per call (and nddm_wiener_hmc's n_iter * n_leapfrog * ceil(n_trials / 64) <= 2^19); P >= 2 when sigma is
 *                      sampled (NDDM_ERR_SHAPE); a run cut into calls gives the bits of the uncut run
 *   outputs, each may be NULL, not all: nddm_wiener_hmc's five, out_sigma f32 [S, K] (sigma after both parts of a kept iteration) and
 *                      out_sigma_accept f32 [S] (the share of the call's sigma proposals accepted; NaN with NDDM_HMC_SIGMA_FIXED).
 *                      out_log_post [C, K] is the participant's CONDITIONAL log posterior in q given sigma: it includes the ext term and
 *                      excludes -log sigma and sigma's prior.  The joint log density of joint chain k at a kept draw, up to a constant, is
 *                      sum_p out_log_post[p * S + k] - P log sigma_k - (sigma_k - 3)^2 / 2.
 * A data set that cannot be sampled flags EVERY chain of the call; joint chain k alone is flagged when the incoming state or inverse mass of
 * any (p, k) is not finite, or sigma_k is not finite and > 0 (or not < 10 when sampled).  A flagged joint chain runs no iteration: sigma and
 * states unchanged, draws and out_sigma NaN, out_flagged = 1 for its P chains, the others' bits unaffected.  The order and the status codes of
 * the checks are nddm_wiener_hmc's.  csrc/nddm_wiener_hmc_joint.h, DESIGN.md section 18. */
#define NDDM_HMC_SIGMA_FIXED 1u
int nddm_wiener_hmc_joint(int32_t model, const float *data /* [P, n_trials, 2] */, int64_t P, int32_t n_trials, int64_t C,
                          int64_t chains /* S */, const double *extdata /* [P] */, double *state /* [C, 12] */,
                          const double *inv_mass /* [C, 5] or NULL */, double *sigma /* [S] */, double *workspace /* [C + S, 4] */,
                          int32_t n_iter, int32_t n_adapt, int32_t n_leapfrog, int32_t thin, uint32_t free_mask, uint64_t seed,
                          uint64_t chain_offset, uint64_t iter_offset, uint32_t flags, float *out_draws, float *out_log_post,
                          float *out_accept, int32_t *out_divergent, int32_t *out_flagged, float *out_sigma, float *out_sigma_accept,
                          void *stream);

/* The single-trial model's MARGINAL log-likelihood: the per-trial boundary a ~ N(mu_alpha, std_alpha^2) | a > 0 is latent, z1 ~ N(gamma a,
 * sigma1^2) observes it, and the response is the first passage of the Wiener process with boundary a; the latent is integrated out, one
 * one-dimensional quadrature per (parameter row, trial), one launch.  What importance weights, posterior-predictive log scores and
 * likelihood-based fits of this model need.  (ABI 4, additive)
 *   model              NDDM_SINGLE_TRIAL only: NDDM_ERR_PARAM otherwise.  NDDM_SINGLE_TRIAL_ALT (a latent diffusion coefficient) is OUT OF
 *                      SCOPE: its latent enters the process differently and it has no likelihood here
 *   params             device f32 [R, 8]: drift, mu_alpha, beta, ter, std_alpha, dc, sigma1, gamma
 *   draws_per_dataset, data, n_trials: as nddm_wiener_log_likelihood takes them; data device f32 [D, n_trials, 2] = (choicert, z1), the
 *                      simulator's output format: choicert = +-(ter + decision time), positive the upper boundary, 0 a timeout
 *   t_censor           the decision time a timeout (choicert == 0) is censored at, in seconds: the simulator's max_steps * dt.  A timeout
 *                      carries no time in this model's output
 *   flags              must be 0 (reserved): NDDM_ERR_PARAM otherwise
 *   out_trial          device f32 [R, n_trials] or NULL: the joint log density of (choicert, z1) of trial i under row r
 *   out_sum            device f64 [R] or NULL (not both NULL): its sum over the trials, in a fixed order
 * Special values (none an error): a row with a non-finite parameter, std_alpha <= 0, sigma1 <= 0, dc <= 0, beta outside (0, 1) or ter < 0
 * gives NaN for every trial and its sum, the other rows unaffected; |choicert| <= ter gives -inf; choicert == 0 is scored as
 * log P(no response before t_censor) when t_censor > 0 and gives NaN otherwise; a non-finite z1 gives NaN.  A valid row with a valid
 * trial never gives NaN or +inf.
 * The bits of out_sum are a function of (the row's parameters, its data set, n_trials, t_censor) alone: the same whatever the layout, the
 * draws_per_dataset factorisation, the stream or a capture.  No scratch memory, no atomics: a call made while `stream` is capturing is one
 * kernel node.  Error checks, their order and their status codes are nddm_wiener_log_likelihood's; R = 0 is NDDM_OK.  Its gradient:
 * nddm_wiener_marginal_log_likelihood_grad below.  The math, the quadrature and its accuracy: csrc/nddm_wiener_marginal.h, DESIGN.md section 15. */
int nddm_wiener_marginal_log_likelihood(int32_t model, const float *params, int64_t R, int64_t draws_per_dataset, const float *data,
                                        int32_t n_trials, float t_censor, uint32_t flags /* 0, reserved */,
                                        float *out_trial /* [R, n_trials] or NULL */, double *out_sum /* [R] or NULL */, void *stream);

/* The same marginal log-likelihood for data sets of DIFFERENT trial counts and for rows without the gamma column: what importance weights
 * of the amortizer's draws need (a 7-column flow, a ragged batch of participants).  (ABI 4, additive)
 *   model, draws_per_dataset, t_censor, flags, out_trial, out_sum, stream: as nddm_wiener_marginal_log_likelihood takes them
 *   params, param_cols device f32 [R, param_cols], param_cols 7 or 8 (NDDM_ERR_PARAM otherwise, checked where the flags are).  7: the
 *                      columns drift .. sigma1 and gamma = 1; the bits are those of the 8-column row with gamma = 1.0f
 *   data, n_trials     device f32 [D, n_trials, 2]: n_trials is the PADDED length, the stride of data and of out_trial
 *   set_counts         device i32 [D] or NULL (every set has n_trials trials).  set_counts[d] = n_d: the rows of set d score its trials
 *                      0 .. n_d - 1 only; data at or beyond n_d are never read (NaN there changes nothing); out_trial[r, t >= n_d] is
 *                      written as 0; the row's out_sum is BIT FOR BIT nddm_wiener_marginal_log_likelihood's for that set alone at
 *                      n_trials = n_d.  A count outside [1, n_trials] gives NaN in out_sum and in all n_trials values of out_trial of that
 *                      set's rows, reads none of its data and leaves the other rows unaffected
 * With param_cols 8 and set_counts NULL both outputs have nddm_wiener_marginal_log_likelihood's bits.  Special values, the bit property of
 * out_sum, no scratch memory, no atomics, one capturable kernel node, the error checks, their order and their status codes: that entry
 * point's; R = 0 is NDDM_OK.  The kernels are instantiations of their own: the plain entry point's are unchanged.  DESIGN.md section 26. */
int nddm_wiener_marginal_log_likelihood_ragged(int32_t model, const float *params, int32_t param_cols /* 7 or 8 */, int64_t R,
                                               int64_t draws_per_dataset, const float *data /* [D, n_trials, 2] */,
                                               int32_t n_trials /* the padded length */, const int32_t *set_counts /* device [D] or NULL */,
                                               float t_censor, uint32_t flags /* 0, reserved */, float *out_trial /* [R, n_trials] or NULL */,
                                               double *out_sum /* [R] or NULL */, void *stream);

/* The same marginal log-likelihood AND its gradient in the model's eight parameter columns, one fused launch: what a gradient-based fit of
 * the single-trial model consumes per step (MAP refinement of amortized draws, Laplace / variational fits, HMC / NUTS).  (ABI 4, additive)
 *   model, params, draws_per_dataset, data, n_trials, t_censor: exactly as nddm_wiener_marginal_log_likelihood takes them
 *   flags              must be 0 (reserved): NDDM_ERR_PARAM otherwise
 *   out_loglik         device f64 [R] or NULL: the row's log-likelihood, BIT FOR BIT nddm_wiener_marginal_log_likelihood's out_sum
 *   out_grad           device f64 [R, 8] (NULL: NDDM_ERR_NULL): d out_loglik[r] / d params[r, j], in params' column order (drift, mu_alpha,
 *                      beta, ter, std_alpha, dc, sigma1, gamma): the expectation of the integrand's partials under the normalised integrand
 *                      on the quadrature's last 32 nodes, the chain rule once per row in float64
 * Special values (none an error): an invalid row (nddm_wiener_marginal_log_likelihood's conditions) gives NaN in out_loglik and in every
 * gradient column, the other rows unaffected; |choicert| <= ter (-inf in the value), a timeout with t_censor <= 0, a non-finite z1 or a NaN
 * choicert (NaN in the value) give NaN in every gradient column of their row.  A TIMEOUT WITH t_censor > 0 HAS A GRADIENT: the partials of
 * log P(no response before t_censor) in both of its forms; a valid row of valid trials, timeouts included, gets a finite gradient.
 * The bits of both outputs are a function of (the row's parameters, its data set, n_trials, t_censor) alone: the same whatever the layout,
 * the draws_per_dataset factorisation, the stream or a capture.  No scratch memory, no atomics: a call made while `stream` is capturing is
 * one kernel node.  Error checks, their order and their status codes are nddm_wiener_marginal_log_likelihood's; R = 0 is NDDM_OK.  The
 * math: csrc/nddm_wiener_marginal_grad.h, DESIGN.md section 16. */
int nddm_wiener_marginal_log_likelihood_grad(int32_t model, const float *params, int64_t R, int64_t draws_per_dataset, const float *data,
                                             int32_t n_trials, float t_censor, uint32_t flags /* 0, reserved */,
                                             double *out_loglik /* [R] or NULL */, double *out_grad /* [R, 8] */, void *stream);

/* The distribution function of the same first-passage law (RWiener / HDDM pwiener, the companion of dwiener) and the choice
 * probability: where in its distribution an observed response time falls -- posterior predictive p-values, probability-integral
 * transforms, one-sample KS distances against the exact law, censoring and truncation.  (ABI 4, additive)
 *   model, params, draws_per_dataset, data, flags: exactly as nddm_wiener_log_likelihood takes them; data may be NULL when out_cdf is
 *   out_cdf            device f32 [R, n_trials] or NULL: P(T <= rt - tau, the boundary trial i ended on | row r), the DEFECTIVE distribution
 *                      function (its limit is the boundary's probability); rt <= tau gives 0.  basic_ddm_dc choice 0 (a timeout) gives
 *                      P(T <= rt - tau) over both boundaries, 1 - S of the censored likelihood; alpha_not_scaled y == 0 gives NaN
 *   out_p_upper        device f32 [R] or NULL (not both NULL): P(upper boundary | row r), drift variability integrated out
 * Absolute accuracy 2e-5 (measured: DESIGN.md section 12); relative accuracy in the far lower tail is not promised.  A value depends on
 * (row, trial) alone: the same bits whatever the layout, launch, stream or capture.  Invalid rows give NaN (their trials and their
 * P(upper)) as in nddm_wiener_log_likelihood, whose error checks, their order and their status codes this entry shares.  No scratch
 * memory: a call made while `stream` is capturing is one kernel node.  The math: csrc/nddm_wiener_cdf.h, DESIGN.md section 12. */
int nddm_wiener_cdf(int32_t model, const float *params, int64_t R, int64_t draws_per_dataset, const float *data, int32_t n_trials,
                    uint32_t flags /* 0, reserved */, float *out_cdf /* [R, n_trials] or NULL */,
                    float *out_p_upper /* [R] or NULL; not both NULL */, void *stream);

/* The quantile function of the same first-passage law (RWiener / HDDM qwiener, the inverse of nddm_wiener_cdf): the response time by
 * which a given share of the responses at a boundary has happened -- quantile-probability plots, posterior-predictive quantile checks,
 * chi-square and G^2 quantile fitting.  (ABI 4, additive)
 *   model, params, draws_per_dataset: exactly as nddm_wiener_cdf takes them; row r answers request set r / draws_per_dataset
 *   probs              device f32 [D, n, 2] = (p, boundary code): code > 0 the upper boundary, code < 0 the lower one, code == 0 either
 *                      boundary (G = F_lower + F_upper, limit 1), for both models
 *   flags              0: p is DEFECTIVE, G(t) = p (p beyond the boundary's probability gives NaN, p equal to it +inf);
 *                      NDDM_QUANTILE_CONDITIONAL: p is the share of that boundary's responses, G(t) = p P(boundary) (p > 1 gives NaN,
 *                      p == 1 +inf, P(boundary) == 0 NaN); any other bit: NDDM_ERR_PARAM
 *   out_q              device f32 [R, n]: rt = tau + t with G(t) = target; p == 0 gives tau; p NaN, p < 0 or a NaN code give NaN; a target
 *                      the float32 G does not reach gives +inf
 * nddm_wiener_cdf at the returned time is within 2e-5 of the target (measured: DESIGN.md section 13).  A value depends on (row, p, code)
 * alone: the same bits whatever the layout, launch, stream or capture.  Invalid rows give NaN, their neighbours unaffected.  The solver
 * is bracketed and its trip count is a compile-time constant.  Error checks, their order and their status codes are nddm_wiener_cdf's
 * (NDDM_ERR_NULL for a NULL params / probs / out_q); R = 0 is NDDM_OK.  No scratch memory: a call made while `stream` is capturing is
 * one kernel node.  The solver: csrc/nddm_wiener_quantile.h, DESIGN.md section 13. */
#define NDDM_QUANTILE_CONDITIONAL 1u
int nddm_wiener_quantile(int32_t model, const float *params, int64_t R, int64_t draws_per_dataset,
                         const float *probs /* [D, n, 2] = (p, boundary code) */, int32_t n,
                         uint32_t flags /* 0 or NDDM_QUANTILE_CONDITIONAL */, float *out_q /* [R, n] */, void *stream);

/* replaces the per-trial loop over diffusion_trial(drift, bound_trial, beta, ter, dc),
 * imputation_from_stahl_not_scaled.py:120-148, :207-213.  bounds: device f32 [B, n_trials].
 * out_trials[b, i, :] = (choicert, bound_trial).  A negative (or NaN) boundary is the reference's ValueError
 * (:124-125): such a trial is written as (NaN, bound) -- validate on the host (Python adapter does) to raise. */
int nddm_explicit_boundary_simulate(const float *params, const float *bounds, int64_t B, int32_t n_trials,
                                    float dt, int32_t max_steps, uint64_t seed, uint64_t set_offset,
                                    uint32_t flags, float *out_trials, float *out_summary, void *stream);

/* generic dispatcher over enum nddm_model (the superset of the arguments above; `bounds` is read only by
 * NDDM_EXPLICIT_BOUNDARY, `ext_sigma` / `ext_mode` / `out_extdata` only by NDDM_ALPHA_NOT_SCALED) */
int nddm_simulate(int32_t model, const float *params, const float *bounds, int64_t B, int32_t n_trials, float dt,
                  int32_t max_steps, uint64_t seed, uint64_t set_offset, uint32_t flags, float ext_sigma, int32_t ext_mode,
                  float *out_trials, float *out_summary, float *out_extdata, void *stream);

/* nddm_simulate with a device-resident part of the set offset: the global index of row 0 is
 * set_offset + *set_offset_dev, read by the launch's pre-pass kernel when it RUNS on `stream` (set_offset_dev: device u64,
 * NULL = 0).  For hipGraph capture: the graph bakes kernel arguments in, the word in device memory moves between replays
 * (the training loop of basic_ddm_dc.py:199-202 as one graph per iteration).  The sum must stay below 2^60; it is reduced
 * modulo 2^60 on the device, where it cannot be refused. */
int nddm_simulate_indirect(int32_t model, const float *params, const float *bounds, int64_t B, int32_t n_trials, float dt,
                           int32_t max_steps, uint64_t seed, uint64_t set_offset, const uint64_t *set_offset_dev, uint32_t flags,
                           float ext_sigma, int32_t ext_mode, float *out_trials, float *out_summary, float *out_extdata,
                           void *stream);

/* The trials in a 2-byte WIRE FORMAT, for the exchange step (the all-gather that reassembles a training
 * minibatch on every rank).  out_codes[b, i] = step index | code << 14 (code 1 upper, 2 lower, 0 timeout) -- what the kernels
 * stage in LDS anyway -- for the models whose second column is a function of the code: NDDM_BASIC_DDM_DC (rt, choice) and
 * NDDM_ALPHA_NOT_SCALED without NDDM_BRIDGE (y, acc); max_steps < 2^14.  Gathering the float pairs moves 8 bytes per trial over
 * every xGMI link, which at this simulator's rate IS a link's bandwidth; the codes are a quarter of that, and
 * nddm_decode_codes (2 B read + 8 B written per trial, HBM-bound) gives back exactly the floats the simulator writes:
 * rt = fma(float(k), dt, tau) with tau from the (gathered) parameter rows.  out_trials / out_summary may be given as well
 * (NULL = not written); set_offset_dev as in nddm_simulate_indirect (NULL = 0). */
int nddm_simulate_codes(int32_t model, const float *params, int64_t B, int32_t n_trials, float dt, int32_t max_steps,
                        uint64_t seed, uint64_t set_offset, const uint64_t *set_offset_dev, uint32_t flags, uint16_t *out_codes,
                        float *out_trials, float *out_summary, void *stream);
int nddm_decode_codes(int32_t model, const uint16_t *codes /* device u16 [B, n_trials] */, const float *params /* device f32 [B, P] */,
                      int64_t B, int32_t n_trials, float dt, float *out_trials /* device f32 [B, n_trials, 2] */, void *stream);

/* ---- prior / context samplers (basic_ddm_dc.py:50-80, single_trial_alpha_not_scaled.py:66-102) -------
 * On-device batched draw_prior(): out device f32 [B, P] in the model's parameter order
 * (P = nddm_model_nparams; gamma column of the single-trial family is filled with `gamma`).
 * Stream: Philox key (seed), counter (draw, 0, row_lo, row_hi | 2<<28). */
int nddm_draw_prior(int32_t model, int64_t B, uint64_t seed, uint64_t set_offset, float gamma, float *out_params,
                    void *stream);

/* the same with a device-resident part of the row offset (see nddm_simulate_indirect) */
int nddm_draw_prior_indirect(int32_t model, int64_t B, uint64_t seed, uint64_t set_offset, const uint64_t *set_offset_dev,
                             float gamma, float *out_params, void *stream);

/* sha256 (hex) of the sources the library was built from, as build.py computed it ("unknown" for a hand-made build): the
 * Python binding refuses a library whose sources have changed since */
const char *nddm_source_hash(void);

/* "hipcc=<version>": the compiler that built this library, recorded at build time */
const char *nddm_build_info(void);

/* ---- debugging aid used by the parity tests: the 4 normals of Philox block (c0..c3) under key (k0,k1) ---
 * flags: NDDM_GAUSS_EXACT / NDDM_GAUSS_FAST (bit 0) and the bits below, a namespace of this entry point.  With NDDM_DEBUG_RAW the
 * output is the transform's own factors instead of the normals -- what the simulators' step loop and auxiliary stream consume: per
 * counter r0, cos0, sin0, r1, cos1, sin1 of the block's two Box-Muller pairs, the radius in NOISE UNITS (exact: sqrt(-2 ln u); fast:
 * sqrt(-log2 u), before any multiply by sqrt(2 ln 2)).  A normal of flags 0 / 1 is (r * unit) * cos|sin.  Fed to the CPU oracle in
 * place of its exact transform (oracle/ddm_oracle.c: oracle_philox_simulate_tab) they hold the fast mode to it bit for bit.
 * Any other bit, a form bit without NDDM_DEBUG_RAW, and NDDM_DEBUG_HOT together with NDDM_DEBUG_PACKED are NDDM_ERR_PARAM. */
enum nddm_debug_normals_flags {
    NDDM_DEBUG_RAW = 2,       /* out f32 [n,6]: (r, cos, sin) of the two pairs */
    NDDM_DEBUG_HOT = 4,       /* with NDDM_DEBUG_RAW: the step loop's form of the pair (the angle spliced by v_bitop3_b32 with constants
                                 held in registers) instead of the auxiliary stream's (shift + v_alignbit_b32) */
    NDDM_DEBUG_PACKED = 8     /* with NDDM_DEBUG_RAW: the NDDM_GAUSS_PACKED layout, out f32 [n,12]: (r, cos, sin) of the four pairs */
};
int nddm_debug_normals(const uint32_t *counters /* device u32 [n,4] */, int64_t n, uint32_t k0, uint32_t k1,
                       uint32_t flags, float *out /* device f32 [n,4], [n,6] or [n,12] */, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NDDM_H */
