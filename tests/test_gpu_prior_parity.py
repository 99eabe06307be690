"""The on-device prior sampler (csrc/nddm_prepass.h: prior_kernel) held to its CPU restatement (oracle/ddm_oracle.c section E) bit for
bit: every model and gamma path, rows deep in a rejection chain, the 256-thread block edges with the output confined to its rows, row
indices across the 32-bit carry, in GraphTrainer's part of the index space and at the 2^60 wrap, direct and through the device word,
seeds with a high word, and DevicePrior's calls.  The restatement's statistics are held to the analytic priors on the CPU
(tests/test_prior_host.py), so equality here carries them to the device."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BASIC, SINGLE, ALT = 0, 1, 2
NCOLS = {BASIC: 5, SINGLE: 8, ALT: 8}
MIN_NORMALS = {BASIC: 4, SINGLE: 5, ALT: 5}


def _device_rows(model, B, **kw):
    from bayesflow_nddms_amd import engine
    return engine.draw_prior_device(model, B, **kw).cpu().numpy()


def _assert_same_bits(dev, ref, what):
    assert dev.dtype == np.float32 and dev.shape == ref.shape, (what, dev.dtype, dev.shape, ref.shape)
    d, r = np.ascontiguousarray(dev).view(np.uint32), ref.view(np.uint32)
    if not np.array_equal(d, r):
        bad = np.flatnonzero((d != r).any(axis=1))
        raise AssertionError(f"{what}: {bad.size} of {len(d)} rows differ, first row {bad[0]}: device {dev[bad[0]]} oracle {ref[bad[0]]}")


def test_engine_and_oracle_number_the_models_alike(oracle_mod):
    from bayesflow_nddms_amd import engine
    assert (engine.BASIC_DDM_DC, engine.SINGLE_TRIAL, engine.SINGLE_TRIAL_ALT) == (oracle_mod.M_BASIC, oracle_mod.M_SINGLE, oracle_mod.M_ALT) \
        == (BASIC, SINGLE, ALT)


@pytest.mark.parametrize("model, gamma", [(BASIC, 1.0), (SINGLE, 1.0), (SINGLE, 0.0), (SINGLE, -1.0), (ALT, 0.37)])
def test_every_path(oracle_mod, model, gamma):
    B, seed = 4096, 2023
    ref, nn, nu = oracle_mod.prior_rows(model, B, seed=seed, gamma=gamma, want_counts=True)
    spare = nn - MIN_NORMALS[model]
    assert (spare == 1).sum() >= 100 and (spare >= 2).sum() >= 5, ((spare == 1).sum(), (spare >= 2).sum())     # else vacuous
    assert np.all(nu == (3 if model == BASIC else (5 if gamma < 0 else 4)))
    dev = _device_rows(model, B, seed=seed, gamma=gamma)
    _assert_same_bits(dev, ref, (model, gamma))
    if model == ALT:
        _assert_same_bits(dev, oracle_mod.prior_rows(SINGLE, B, seed=seed, gamma=gamma), "alt against the oracle's single")
        _assert_same_bits(dev, _device_rows(SINGLE, B, seed=seed, gamma=gamma), "alt against the device's single")


def test_deep_rejection_chains(oracle_mod):
    """The 8 rows of a million that consumed the most normals (9 and more: a third normals block), each launched alone."""
    seed = 7
    ref, nn, _ = oracle_mod.prior_rows(SINGLE, 1_000_000, seed=seed, gamma=-1.0, want_counts=True)
    deepest = np.argsort(nn, kind="stable")[-8:]
    assert nn[deepest].max() >= 9 and nn[deepest].min() >= 8, nn[deepest]
    for i in deepest:
        _assert_same_bits(_device_rows(SINGLE, 1, seed=seed, set_offset=int(i), gamma=-1.0), ref[i:i + 1], (int(i), int(nn[i])))


@pytest.mark.parametrize("model", [BASIC, SINGLE])
def test_block_edges_and_confinement(oracle_mod, model):
    import torch
    from bayesflow_nddms_amd import _lib, engine
    P, seed, sentinel = NCOLS[model], 31, -12345.0
    for B in (1, 255, 256, 257, 513):
        buf = torch.full((64 + B * P + 64,), sentinel, dtype=torch.float32, device="cuda")
        out = buf[64:64 + B * P].view(B, P)
        got = engine.draw_prior_device(model, B, seed=seed, set_offset=5, gamma=-1.0, out=out)
        assert got.data_ptr() == out.data_ptr()
        host = buf.cpu().numpy()
        assert np.all(host[:64] == np.float32(sentinel)) and np.all(host[-64:] == np.float32(sentinel)), B
        _assert_same_bits(host[64:-64].reshape(B, P), oracle_mod.prior_rows(model, B, seed=seed, set_offset=5, gamma=-1.0), (model, B))
    # B = 0: success, nothing launched, nothing written
    buf = torch.full((128 + P,), sentinel, dtype=torch.float32, device="cuda")
    with torch.cuda.device(buf.device):
        rc = _lib.lib().nddm_draw_prior(model, 0, seed, 5, -1.0, buf[64:].data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert engine.draw_prior_device(model, 0, seed=seed, out=buf[64:64].view(0, P)).shape == (0, P)
    assert engine.draw_prior_device(model, 0, seed=seed).shape == (0, P)
    assert bool((buf == sentinel).all())


@pytest.mark.parametrize("model", [BASIC, SINGLE])
@pytest.mark.parametrize("offset", [2**32 - 100, 2**32, 2**59, 2**59 + 2**32 - 3, 2**60 - 130])
def test_row_index(oracle_mod, model, offset):
    B, seed = 257, 2023
    dev = _device_rows(model, B, seed=seed, set_offset=offset, gamma=-1.0)
    _assert_same_bits(dev, oracle_mod.prior_rows(model, B, seed=seed, set_offset=offset, gamma=-1.0), (model, offset))
    if offset + B > 2**60:           # rows 2^60 apart share a stream: the last 127 rows are rows 0..126
        lo = oracle_mod.prior_rows(model, 2**60 - offset, seed=seed, set_offset=offset, gamma=-1.0)
        hi = oracle_mod.prior_rows(model, offset + B - 2**60, seed=seed, set_offset=0, gamma=-1.0)
        _assert_same_bits(dev, np.concatenate([lo, hi]), (model, offset, "mod 2^60"))


@pytest.mark.parametrize("model", [BASIC, SINGLE])
def test_row_index_through_the_device_word(oracle_mod, model):
    import torch
    from bayesflow_nddms_amd import engine
    B, seed, P = 257, 2023, NCOLS[model]
    for offset, word in ((2**32 - 7, 2**33 + 11), (0, 2**59)):
        w = torch.tensor([word], dtype=torch.int64, device="cuda")
        dev = _device_rows(model, B, seed=seed, set_offset=offset, gamma=-1.0, set_offset_dev=w)
        _assert_same_bits(dev, oracle_mod.prior_rows(model, B, seed=seed, set_offset=offset + word, gamma=-1.0), (model, offset, word))
    # the word is read when the launch runs: rewritten between two launches into the same rows
    w = torch.tensor([2**59 + 2**32 - 100], dtype=torch.int64, device="cuda")
    out = torch.empty((B, P), dtype=torch.float32, device="cuda")
    for word in (2**59 + 2**32 - 100, 2**59 + 2**32 - 100 + B):
        w.fill_(word)
        engine.draw_prior_device(model, B, seed=seed, set_offset=3, gamma=-1.0, set_offset_dev=w, out=out)
        _assert_same_bits(out.cpu().numpy(), oracle_mod.prior_rows(model, B, seed=seed, set_offset=3 + word, gamma=-1.0), (model, word))


@pytest.mark.parametrize("model", [BASIC, SINGLE])
def test_seeds(oracle_mod, model):
    B = 64
    for seed in (0, 2**32, 2**64 - 1, 0xdeadbeef00000007):
        _assert_same_bits(_device_rows(model, B, seed=seed, set_offset=9, gamma=-1.0),
                          oracle_mod.prior_rows(model, B, seed=seed, set_offset=9, gamma=-1.0), (model, hex(seed)))
    a, b = _device_rows(model, B, seed=5, gamma=-1.0), _device_rows(model, B, seed=5 + 2**32, gamma=-1.0)
    assert not np.any(np.all(a == b, axis=1))                   # the key's high word is in the stream


@pytest.mark.parametrize("name", ["basic", "single", "scale"])
def test_device_prior_calls(oracle_mod, name):
    from bayesflow_nddms_amd.priors import DevicePrior
    model, gamma, cols = {"basic": (BASIC, 1.0, 5), "single": (SINGLE, 1.0, 7), "scale": (SINGLE, -1.0, 8)}[name]
    prior = DevicePrior(name, seed=11)
    for B, offset in ((300, 0), (212, 300)):
        dev = prior(B).cpu().numpy()
        _assert_same_bits(dev, np.ascontiguousarray(oracle_mod.prior_rows(model, B, seed=11, set_offset=offset, gamma=gamma)[:, :cols]),
                          (name, B, offset))
