"""CPU checks of which all-pairs screen a prune runs (plan_screen in fc_kabsch.hip, through fc_debug_screen_plan): one case
per row of the rule and per error, and the shapes whose screen the GPU tests assert.  No device is needed."""

import ctypes as C

import numpy as np
import pytest

from firecode_amd import _lib
from firecode_amd import synthetic as syn

NAN = float("nan")


def plan(n, a, row_block, lean, g_max, h2_model=1, max_rmsd=0.5):
    out = np.zeros(5, dtype=np.int64)
    rc = _lib.load().fc_debug_screen_plan(n, a, row_block, lean, g_max, max_rmsd, h2_model, _lib.pi(out))
    return rc, out.tolist()


@pytest.fixture
def knobs(monkeypatch):
    """FC_SCREEN_F32 / FC_SCREEN_CFG (read on every call) and fc_screen_select, restored afterwards"""
    def set_(f32, cfg, forced):
        for name, value in (("FC_SCREEN_F32", f32), ("FC_SCREEN_CFG", cfg)):
            if value is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, value)
        _lib.screen_select(forced)

    yield set_
    _lib.screen_select(0)


# threshold 0.5 A (thr^2 + margin = 0.250001): the split-half band 2 p0 g_max / A is 0.1 thr^2 at g_max ~ 800-1100 and
# the limit 4 thr^2 at ~31 000-42 000; the fp32 band is 2-2.5 x narrower.  g_max 500: below 0.1 thr^2 for both, 10 000:
# between, 60 000: split-half above the limit and fp32 below it, 200 000: both above.
# (label, N, atoms, row block, lean, g_max, model check, FC_SCREEN_F32, FC_SCREEN_CFG, fc_screen_select,
#  return code, [kind, column tile, stages, speculative, fp64 waves])
CASES = [
    ('row 0: no conformers', 0, 50, 128, 1, 500.0, 1, None, None, 0, 0, [0, 0, 0, 0, 0]),
    ('row 1: FC_SCREEN_CFG=valu8x4', 10000, 50, 128, 1, 500.0, 1, None, 'valu8x4', 0, 0, [1, 64, 1, 0, 0]),
    ('row 2: 193 atoms, narrow band', 4000, 193, 128, 1, 500.0, 1, None, None, 0, 0, [16, 32, 1, 0, 0]),
    ('row 2: 260 atoms, band below the limit', 4000, 260, 128, 1, 10000.0, 1, None, None, 0, 0, [16, 32, 1, 0, 0]),
    ('row 2: 384 atoms', 4000, 384, 128, 1, 10000.0, 1, None, None, 0, 0, [16, 32, 1, 0, 0]),
    ('row 2: 416 atoms, row block 32 (the tile fits)', 4000, 416, 32, 1, 10000.0, 1, None, None, 0, 0, [16, 32, 1, 0, 0]),
    ('row 2: forced 16, band above the limit', 4000, 260, 128, 1, 60000.0, 1, None, None, 16, 0, [16, 32, 1, 0, 0]),
    ('row 2: FC_SCREEN_F32=2, band above the limit', 4000, 260, 128, 1, 60000.0, 1, '2', None, 0, 0, [16, 32, 1, 0, 0]),
    ('row 3: 260 atoms, split-half band too wide', 4000, 260, 128, 1, 60000.0, 1, None, None, 0, 0, [32, 32, 1, 0, 0]),
    ('row 3: 360 atoms', 4000, 360, 128, 1, 60000.0, 1, None, None, 0, 0, [32, 32, 1, 0, 0]),
    ('row 3: no model check', 4000, 260, 128, 1, 10000.0, 0, None, None, 0, 0, [32, 32, 1, 0, 0]),
    ('row 3: forced 32, band above the limit', 4000, 260, 128, 1, 200000.0, 1, None, None, 32, 0, [32, 32, 1, 0, 0]),
    ('row 4: 50 atoms, narrow band', 10000, 50, 128, 1, 500.0, 1, None, None, 0, 0, [16, 64, 1, 0, 0]),
    ('row 4: 50 atoms, band between 0.1 thr^2 and the limit: speculative', 10000, 50, 128, 1, 10000.0, 1, None, None, 0, 0, [16, 64, 1, 1, 4]),
    ('row 4: N <= 512 is never speculative', 512, 50, 128, 1, 10000.0, 1, None, None, 0, 0, [16, 64, 1, 0, 0]),
    ('row 4: split-half band too wide, fp32 band not: fp32, speculative', 10000, 50, 128, 1, 60000.0, 1, None, None, 0, 0, [32, 64, 2, 1, 4]),
    ('row 4: both bands too wide: fp64', 10000, 50, 128, 1, 200000.0, 1, None, None, 0, 0, [64, 64, 1, 0, 4]),
    ('row 4: not lean: split-half with bits', 10000, 50, 128, 0, 500.0, 1, None, None, 0, 0, [16, 64, 1, 0, 0]),
    ('row 4: no model check: fp32, two stages', 10000, 50, 128, 1, 500.0, 0, None, None, 0, 0, [32, 64, 2, 0, 0]),
    ('row 4: FC_SCREEN_F32=0', 10000, 50, 128, 1, 500.0, 1, '0', None, 0, 0, [64, 64, 1, 0, 4]),
    ('row 4: FC_SCREEN_F32=2, band too wide for both', 10000, 50, 128, 1, 200000.0, 1, '2', None, 0, 0, [16, 64, 1, 0, 0]),
    ('row 4: FC_SCREEN_F32=3, narrow band', 10000, 50, 128, 1, 500.0, 1, '3', None, 0, 0, [16, 64, 1, 1, 4]),
    ('row 4: forced 64', 10000, 50, 128, 1, 500.0, 1, None, None, 64, 0, [64, 64, 1, 0, 4]),
    ('row 4: forced 32, not lean: one stage', 10000, 50, 128, 0, 500.0, 1, None, None, 32, 0, [32, 64, 1, 0, 0]),
    ('row 4: forced 16, band too wide', 10000, 50, 128, 1, 200000.0, 1, None, None, 16, 0, [16, 64, 1, 0, 0]),
    ('row 4: NaN g_max: fp64', 10000, 50, 128, 1, NAN, 1, None, None, 0, 0, [64, 64, 1, 0, 4]),
    ('row 4: 80 atoms: 8-wave fp64 workgroups', 10000, 80, 128, 1, 200000.0, 1, None, None, 0, 0, [64, 64, 1, 0, 8]),
    ('row 4: 80 atoms, speculative split-half', 10000, 80, 128, 1, 10000.0, 1, None, None, 0, 0, [16, 64, 1, 1, 8]),
    ('row 4: 128 atoms, no fp64 tile: never speculative', 10000, 128, 128, 1, 10000.0, 1, None, None, 0, 0, [16, 64, 1, 0, 0]),
    ('row 4: 160 atoms', 10000, 160, 128, 1, 10000.0, 1, None, None, 0, 0, [16, 64, 1, 0, 0]),
    ('row 4: 160 atoms, split-half band too wide: fp32', 10000, 160, 128, 1, 60000.0, 1, None, None, 0, 0, [32, 64, 2, 0, 0]),
    ('row 4: 196 atoms, split-half band too wide: fp32 64-column tile', 4000, 196, 128, 1, 60000.0, 1, None, None, 0, 0, [32, 64, 2, 0, 0]),
    ('row 4: 160 atoms, both bands too wide: VALU', 10000, 160, 128, 1, 200000.0, 1, None, None, 0, 0, [1, 64, 1, 0, 0]),
    ('row 5: 260 atoms, not lean', 4000, 260, 128, 0, 10000.0, 1, None, None, 0, 0, [1, 64, 1, 0, 0]),
    ('row 5: 260 atoms, both bands too wide', 4000, 260, 128, 1, 200000.0, 1, None, None, 0, 0, [1, 64, 1, 0, 0]),
    ('row 5: 416 atoms, row block 128 (the tile does not fit)', 4000, 416, 128, 1, 10000.0, 1, None, None, 0, 0, [1, 64, 1, 0, 0]),
    ('row 5: 420 atoms', 4000, 420, 128, 1, 10000.0, 1, None, None, 0, 0, [1, 64, 1, 0, 0]),
    ('row 5: FC_SCREEN_F32=0 at 260 atoms', 4000, 260, 128, 1, 10000.0, 1, '0', None, 0, 0, [1, 64, 1, 0, 0]),
    ('quirk: forced 16 at 420 atoms falls through to VALU', 4000, 420, 128, 1, 10000.0, 1, None, None, 16, 0, [1, 64, 1, 0, 0]),
    ('quirk: forced 16 with a NaN g_max at 260 atoms falls through to VALU', 4000, 260, 128, 1, NAN, 1, None, None, 16, 0, [1, 64, 1, 0, 0]),
    ('FC_E_INVALID: forced 16 with a NaN g_max at 50 atoms', 10000, 50, 128, 1, NAN, 1, None, None, 16, -1, [0, 0, 0, 0, 0]),
    ('FC_E_INVALID: forced 16 without the model check', 10000, 50, 128, 1, 500.0, 0, None, None, 16, -1, [0, 0, 0, 0, 0]),
    ('FC_E_LIMIT: split-half row block does not fit the LDS', 1000, 100, 16384, 1, 100.0, 1, None, None, 0, -5, [0, 0, 0, 0, 0]),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_screen_plan_rule(knobs, case):
    label, n, a, rb, lean, g_max, model, f32, cfg, forced, rc, want = case
    knobs(f32, cfg, forced)
    assert plan(n, a, rb, lean, g_max, model) == (rc, want)


def _g_max(X):
    return float(((X - X.mean(axis=1, keepdims=True)) ** 2).sum(axis=(1, 2)).max())


# ensembles of the GPU tests that assert fc_screen_last_kind after a lean prune (default row block 128, threshold 0.5; the
# ones whose generation takes the CPU more than a few seconds are left out)
GPU_SHAPES = [
    # tests/test_gpu_parity.py::test_prune_large_compact_structures
    *[(n, a, dict(seed=700 + a, cluster_size=3, compact=True), 0, 16 if a <= 384 else 1)
      for n, a in [(150, 193), (140, 224), (130, 260), (120, 320), (100, 384), (100, 416)]],
    # tests/test_gpu_parity.py::test_prune_large_extended_structures_on_the_fp32_pipe (fc_screen_select(32))
    *[(n, a, dict(seed=s, cluster_size=3), 32, 32)
      for n, a, s in [(140, 214, 2), (130, 224, 2)]],
    # tests/test_gpu_parity.py::test_wide_band_takes_the_speculative_screen
    (600, 80, dict(seed=4), 0, 16),
    # tests/test_gpu_fullsize.py: compact and extended structures, and the sharded prune of 260 atoms
    *[(n, a, dict(seed=800 + a, cluster_size=5, compact=True), 0, 16) for n, a in [(7010, 224), (6000, 260), (4500, 320), (3000, 384)]],
    *[(n, a, dict(seed=2, cluster_size=50), 0, 32) for n, a in [(6010, 224), (5000, 260)]],
    (4200, 260, dict(seed=31, cluster_size=5, compact=True), 0, 16),
]


@pytest.mark.parametrize("n,a,gen,forced,kind", GPU_SHAPES)
def test_screen_plan_agrees_with_the_gpu_tests(knobs, n, a, gen, forced, kind):
    X, _, _ = syn.synthetic_ensemble(n, a, **gen)
    knobs(None, None, forced)
    rc, got = plan(n, a, 128, 1, _g_max(X))
    assert rc == 0 and got[0] == kind


def test_screen_plan_refuses_bad_arguments():
    out = np.zeros(5, dtype=np.int64)
    L = _lib.load()
    assert L.fc_debug_screen_plan(100, 0, 128, 1, 1.0, 0.5, 1, _lib.pi(out)) == _lib.FC_E_INVALID
    assert L.fc_debug_screen_plan(100, 50, 128, 1, 1.0, 0.5, -1, _lib.pi(out)) == _lib.FC_E_INVALID
    assert L.fc_debug_screen_plan(100, 50, 128, 1, 1.0, 0.5, 1, C.POINTER(C.c_int64)()) == _lib.FC_E_INVALID
