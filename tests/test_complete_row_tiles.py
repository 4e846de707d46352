"""The complete all-pairs alignments with the row conformer of the atom pass read from Xt, the row-tile-major copy of the
ensemble (k_simbits_screen_mfma mode 2 with ROWT, csrc/fc_items.h).  Where an operand comes from
changes no pair's arithmetic: the two (N, N) outputs of FC_COMPLETE_ROW_TILES=1 (the default) equal those of
FC_COMPLETE_ROW_TILES=0 (the row conformer from three rows of Xs per atom, the form before) as raw 64-bit patterns --
over partial row tiles and row blocks, odd and tiny atom counts, all four instantiations of the kernel, logical ranks, both
item shapes, the running-sum form, an atom selection, and an ensemble made after another one was destroyed.

The library allocates the two device matrices itself, so they cannot be prefilled with NaN from here; instead a pass over
ANOTHER ensemble of the same size runs in front of every compared pass: an element a pass failed to write then holds a
value of that other ensemble (or whatever the allocation held), not the right one of the pass before.  One case of each
tile width is also compared with the oracle: rmsd within 1e-10, max deviation within 1e-10 + the pair's conditioning
bound."""
import numpy as np
import pytest

from firecode_amd import synthetic as syn
from oracle import cpu_ref as o

pytestmark = pytest.mark.gpu

TOL = 1e-10
SWITCHES = ("FC_COMPLETE_ROW_TILES", "FC_COMPLETE_ROW_CHUNK", "FC_SCREEN_TAIL_SLOTS", "FC_COMPLETE_EIG")


def _ensemble(n, a, seed):
    X, _, _ = syn.synthetic_ensemble(n, a, seed=seed, cluster_size=5 if a <= 100 else 50)
    return X


def _setenv(monkeypatch, **env):
    for name in SWITCHES:
        if env.get(name) is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, env[name])


def _bits(M):
    return np.ascontiguousarray(M).view(np.uint64)


def _check_oracle(X, R, D, seed, count=256):
    rng = np.random.default_rng(seed)
    n = len(X)
    i = rng.integers(0, n - 1, size=count)
    j = i + 1 + rng.integers(0, n, size=count) % (n - 1 - i)
    q = count // 4
    i[:q] = rng.integers((n - 1) // 16 * 16, n, size=q)  # a quarter in the last (partial) row tile, as row or as column
    j[:q] = rng.integers(0, n, size=q)
    keep = i != j
    i, j = i[keep], j[keep]
    r0, d0 = o.rmsd_and_max_batch(X[i], X[j], center=True)
    bound = o.rotation_error_bound_batch(X[i], X[j], center=True)
    er, ed = np.abs(R[i, j] - r0), np.abs(D[i, j] - d0)
    print(f"n={n} a={X.shape[1]}: max |rmsd - oracle| {er.max():.3e}, max |maxdev - oracle| {ed.max():.3e}, "
          f"largest conditioning allowance {bound.max():.3e}")
    assert er.max() < TOL and np.all(ed <= TOL + bound)


def _compare(fc, monkeypatch, X, Y, atom_mask=None, oracle_seed=None, **env):
    """both outputs with the row conformer from Xt and from Xs, under the switches of `env`: identical bit patterns"""
    try:
        with fc.DeviceEnsemble(X, atom_mask, center=True) as ens, fc.DeviceEnsemble(Y, atom_mask, center=True) as other:
            _setenv(monkeypatch, FC_COMPLETE_ROW_TILES="0", **env)
            R0, D0, _ = ens.rmsd_and_max_all()
            assert not np.isnan(R0).any() and not np.isnan(D0).any() and np.all(np.diag(R0) == 0) and np.all(np.diag(D0) == 0)
            for tiles in (None, "1"):  # the default is the new path
                _setenv(monkeypatch, FC_COMPLETE_ROW_TILES=tiles, **env)
                other.rmsd_and_max_all()
                R, D, _ = ens.rmsd_and_max_all()
                assert np.array_equal(_bits(R), _bits(R0)) and np.array_equal(_bits(D), _bits(D0)), (tiles, env)
            if oracle_seed is not None:
                Xsel = X if atom_mask is None else X[:, np.asarray(atom_mask, dtype=bool)]
                _check_oracle(Xsel, R, D, oracle_seed)
    finally:
        _setenv(monkeypatch)


@pytest.mark.parametrize("n", [17, 65, 129, 200, 513])
def test_sizes(fc, monkeypatch, n):
    """50 atoms (two workgroups per CU, the benchmark's kernel): a partial last row tile, a partial last row block,
    several row blocks (at 513 with half items when the tail is short)"""
    _compare(fc, monkeypatch, _ensemble(n, 50, 400 + n), _ensemble(n, 50, 1400 + n), oracle_seed=n if n == 200 else None)


@pytest.mark.parametrize("a", [3, 4, 5, 49, 50, 52])
def test_atom_counts(fc, monkeypatch, a):
    """an odd atom count (the second atom of the last pair is a zero of Xt), an odd and an even number of rounds, tiny
    structures (fewer rounds than a k-group holds)"""
    _compare(fc, monkeypatch, _ensemble(129, a, 500 + a), _ensemble(129, a, 1500 + a))


@pytest.mark.parametrize("a", [53, 80, 105, 171, 209])
def test_the_one_workgroup_kernels(fc, monkeypatch, a):
    """the other instantiations: eight waves with 64 columns (53, 80), 32 columns (105, 171), 16 columns (209); from 171
    atoms a conformer's rounds span more than the load's immediate reaches (171 and 209: 86 and 105 rounds of 768 bytes)"""
    _compare(fc, monkeypatch, _ensemble(200, a, 600 + a), _ensemble(200, a, 1600 + a), oracle_seed=a if a in (105, 209) else None)


@pytest.mark.parametrize("chunk,tail", [("1", None), ("4", "2"), ("4", "0")])
def test_item_shapes(fc, monkeypatch, chunk, tail):
    """single row blocks, and chunks of four forced onto a small ensemble by a short tail (with and without half items):
    the row tiles a wave walks then lie in several row blocks"""
    _compare(fc, monkeypatch, _ensemble(513, 50, 71), _ensemble(513, 50, 1071), FC_COMPLETE_ROW_CHUNK=chunk,
             FC_SCREEN_TAIL_SLOTS=tail)


@pytest.mark.parametrize("n,a", [(200, 50), (129, 49), (200, 105)])
def test_running_sum_form(fc, monkeypatch, n, a):
    """FC_COMPLETE_EIG=0: the rmsd from the sum of the atom pass (one more chain per atom and pair in the loop)"""
    _compare(fc, monkeypatch, _ensemble(n, a, 81 + a), _ensemble(n, a, 1081 + a), FC_COMPLETE_EIG="0")


def test_atom_selection_and_centring(fc, monkeypatch):
    """37 of 60 atoms selected, every conformer shifted by its own vector: Xt carries the centred, selected atoms"""
    n, a_all = 200, 60
    rng = np.random.default_rng(91)
    mask = np.zeros(a_all, dtype=bool)
    mask[rng.permutation(a_all)[:37]] = True
    X = _ensemble(n, a_all, 91) + rng.normal(scale=25.0, size=(n, 1, 3))
    Y = _ensemble(n, a_all, 1091) + rng.normal(scale=25.0, size=(n, 1, 3))
    _compare(fc, monkeypatch, X, Y, atom_mask=mask, oracle_seed=91)


def test_a_second_ensemble_after_the_first_is_destroyed(fc, monkeypatch):
    """Xt is made on an ensemble's first complete-alignment call and freed with it: an ensemble of another shape, then one
    of the same shape with other coordinates, created behind a destroyed one, must not see anything of it"""
    try:
        _setenv(monkeypatch)
        first = fc.DeviceEnsemble(_ensemble(200, 50, 101), center=True)
        first.rmsd_and_max_all()
        first.close()
        for n, a, seed in ((129, 49, 102), (200, 50, 103)):
            _compare(fc, monkeypatch, _ensemble(n, a, seed), _ensemble(n, a, 1000 + seed), oracle_seed=seed)
    finally:
        _setenv(monkeypatch)


@pytest.mark.parametrize("world", [2, 3])
def test_logical_ranks(fc, monkeypatch, world):
    """rank r of `world` takes the row blocks dealt to it in snake order: the row tiles of an item are not neighbours.
    Each rank's rows with the row conformer from Xt equal the single-rank pass with the row conformer from Xs."""
    from firecode_amd import _lib
    from firecode_amd import dist as fdist

    n, a = 1041, 50
    X, Y = _ensemble(n, a, 77), _ensemble(n, a, 1077)
    iu, ju = np.triu_indices(n, 0)  # the diagonal too
    owner = fdist.owner_of_rows(n, world, 128)
    try:
        with fc.DeviceEnsemble(X, center=True) as ens, fc.DeviceEnsemble(Y, center=True) as other:
            _setenv(monkeypatch, FC_COMPLETE_ROW_TILES="0")
            R0, D0, _ = ens.rmsd_and_max_all()
            for chunk, tail in [(None, None), ("4", "2")]:
                _setenv(monkeypatch, FC_COMPLETE_ROW_TILES="1", FC_COMPLETE_ROW_CHUNK=chunk, FC_SCREEN_TAIL_SLOTS=tail)
                for rk in range(world):
                    _lib.call("fc_debug_comm_loopback", rk, world)
                    mine = owner[iu] == rk
                    other.bench_rmsd_and_max_all_sampled(iu[:1], ju[:1], reps=1)
                    _, _, st, r, d = ens.bench_rmsd_and_max_all_sampled(iu[mine], ju[mine], reps=1)
                    assert int(st[2]) == 1
                    assert np.array_equal(_bits(r), _bits(R0[iu[mine], ju[mine]])), (chunk, tail, rk)
                    assert np.array_equal(_bits(d), _bits(D0[iu[mine], ju[mine]])), (chunk, tail, rk)
    finally:
        _lib.call("fc_debug_comm_loopback", -1, 0)
        _setenv(monkeypatch)
