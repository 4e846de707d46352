"""The complete all-pairs alignments with items that keep their column tile for several row blocks
(k_simbits_screen_mfma mode 2, csrc/fc_items.h).  The shape of an item changes which workgroup
computes a pair, never the pair's arithmetic: the two (N, N) outputs are BIT-IDENTICAL between FC_COMPLETE_ROW_CHUNK=1
(single row blocks, the form before) and

  * the default (chunks of two in front of about three rounds of single items; at these sizes the whole launch is
    shorter than that, so the default alone would be single items again), and
  * chunks forced onto small ensembles by a short tail (FC_SCREEN_TAIL_SLOTS): chunks + single items + halves,
    everything in chunks (also a last chunk shorter than the others), chunks of 2, 3, 4 and 8.

The library allocates the two device matrices itself, so they cannot be prefilled with NaN from here; instead a pass
over ANOTHER ensemble of the same size runs in front of every compared pass: an element a pass failed to write then
holds a value of that other ensemble (or whatever the allocation held), not the right one of the pass before.
Every case also checks 256 seeded pairs -- a share of them in the last column tile and in the last row block --
against the oracle at 1e-10."""
import numpy as np
import pytest

from firecode_amd import synthetic as syn
from oracle import cpu_ref as o

pytestmark = pytest.mark.gpu

TOL = 1e-10
# (FC_COMPLETE_ROW_CHUNK, FC_SCREEN_TAIL_SLOTS); None = unset
ARMS = [(None, None), ("4", "2"), ("4", "0"), ("3", "1"), ("2", "3"), ("8", "0")]


def _ensemble(n, a, seed):
    X, _, _ = syn.synthetic_ensemble(n, a, seed=seed, cluster_size=5 if a <= 100 else 50)
    return X


def _setenv(monkeypatch, chunk, tail):
    for name, v in (("FC_COMPLETE_ROW_CHUNK", chunk), ("FC_SCREEN_TAIL_SLOTS", tail)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)


def _sample_pairs(n, rng, count=256):
    """count pairs i < j: a quarter with j in the last column tile, a quarter with i in the last row block (where it has
    more than one row), the rest anywhere"""
    i = rng.integers(0, n - 1, size=count)
    j = i + 1 + rng.integers(0, n, size=count) % (n - 1 - i)
    q = count // 4
    j0 = (n - 1) // 64 * 64
    j[:q] = rng.integers(max(j0, 1), n, size=q)
    i[:q] = rng.integers(0, j[:q])
    i0 = (n - 1) // 128 * 128
    if n - i0 >= 2:
        i[q:2 * q] = rng.integers(i0, n - 1, size=q)
        j[q:2 * q] = i[q:2 * q] + 1 + rng.integers(0, n, size=q) % (n - 1 - i[q:2 * q])
    assert np.all(i < j) and np.all(j < n) and np.all(i >= 0)
    return i, j


def _check_oracle(X, R, D, rng):
    i, j = _sample_pairs(len(X), rng)
    r0, d0 = o.rmsd_and_max_batch(X[i], X[j], center=True)
    er, ed = np.abs(R[i, j] - r0).max(), np.abs(D[i, j] - d0).max()
    print(f"n={len(X)} a={X.shape[1]}: max |rmsd - oracle| {er:.3e}, max |maxdev - oracle| {ed:.3e}")
    assert er < TOL and ed < TOL


def _compare_arms(fc, monkeypatch, n, a, seed):
    X, Y = _ensemble(n, a, seed), _ensemble(n, a, seed + 1000)
    rng = np.random.default_rng(seed)
    with fc.DeviceEnsemble(X, center=True) as ens, fc.DeviceEnsemble(Y, center=True) as other:
        _setenv(monkeypatch, "1", None)
        R1, D1, _ = ens.rmsd_and_max_all()
        assert not np.isnan(R1).any() and not np.isnan(D1).any() and np.all(np.diag(R1) == 0) and np.all(np.diag(D1) == 0)
        _check_oracle(X, R1, D1, rng)
        for chunk, tail in ARMS:
            _setenv(monkeypatch, chunk, tail)
            other.rmsd_and_max_all()
            R, D, _ = ens.rmsd_and_max_all()
            assert np.array_equal(R, R1) and np.array_equal(D, D1), (chunk, tail)
    _setenv(monkeypatch, None, None)


@pytest.mark.parametrize("n", [17, 64, 65, 129, 200, 513, 640, 1041])
def test_chunked_items_equal_single_row_blocks_bit_for_bit(fc, monkeypatch, n):
    """50 atoms (two workgroups per CU, the benchmark's kernel): a single partial row block, N % 64 in {1, 8, 17, 0},
    2 ... 9 row blocks -- counts the chunk lengths do not divide"""
    _compare_arms(fc, monkeypatch, n, 50, seed=300 + n)


@pytest.mark.parametrize("a", [80, 105, 209])
def test_chunked_items_of_the_one_workgroup_kernels(fc, monkeypatch, a):
    """the three other instantiations (64-, 32- and 16-column tiles, eight waves): they stay on single row blocks by
    default and take chunks when asked"""
    _compare_arms(fc, monkeypatch, 300, a, seed=a)


@pytest.mark.parametrize("world", [2, 3])
def test_chunked_items_of_logical_ranks(fc, monkeypatch, world):
    """rank r of `world` takes the row blocks dealt to it in snake order: the blocks of a chunk are not neighbours.  Each
    rank's rows, from either form of items, equal the single-rank pass with single row blocks."""
    from firecode_amd import _lib
    from firecode_amd import dist as fdist

    n, a = 1041, 50
    X, Y = _ensemble(n, a, 77), _ensemble(n, a, 1077)
    iu, ju = np.triu_indices(n, 0)  # the diagonal too
    owner = fdist.owner_of_rows(n, world, 128)
    try:
        with fc.DeviceEnsemble(X, center=True) as ens, fc.DeviceEnsemble(Y, center=True) as other:
            _setenv(monkeypatch, "1", None)
            R1, D1, _ = ens.rmsd_and_max_all()
            _check_oracle(X, R1, D1, np.random.default_rng(world))
            for chunk, tail in [(None, None), ("4", "2"), ("4", "0"), ("3", "1")]:
                _setenv(monkeypatch, chunk, tail)
                for rk in range(world):
                    _lib.call("fc_debug_comm_loopback", rk, world)
                    mine = owner[iu] == rk
                    other.bench_rmsd_and_max_all_sampled(iu[:1], ju[:1], reps=1)
                    _, _, st, r, d = ens.bench_rmsd_and_max_all_sampled(iu[mine], ju[mine], reps=1)
                    assert int(st[2]) == 1
                    assert np.array_equal(r, R1[iu[mine], ju[mine]]) and np.array_equal(d, D1[iu[mine], ju[mine]]), (chunk, tail, rk)
    finally:
        _lib.call("fc_debug_comm_loopback", -1, 0)
        _setenv(monkeypatch, None, None)
