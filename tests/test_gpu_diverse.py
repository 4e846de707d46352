"""RMSD-diverse selection on the GPU (fc_ensemble_select_diverse and the Python layers above it) against the NumPy
restatement of its contract (tests/diverse_ref.py) on the oracle's Kabsch RMSD.

Bars: indices and labels identical, distances and radii within 1e-10 -- on ensembles whose every decision (argmax,
``t < D[j]``, radius stop) the restatement recorded with a gap above 1e-9, so that rounding cannot flip one."""

import numpy as np
import pytest

from diverse_ref import prepared, replay, select_diverse
from firecode_amd import synthetic as syn
from oracle import cpu_ref as o

pytestmark = pytest.mark.gpu

TOL = 1e-10
GAP = 1e-9
FOLDS = {2: (0, 180), 3: (0, 120, 240), 4: (0, 90, 180, 270), 6: (0, 60, 120, 180, 240, 300)}


def _compare(fc, X, atoms, n, start=0, stop_rmsd=None, heavy_atoms_only=True, monkeypatch=None, lanes=(None,)):
    """the selection against the restatement (computed once), for each forced lane form in ``lanes``"""
    Xsel = prepared(X, atoms, heavy_atoms_only)
    ref = select_diverse(Xsel, n, start=start, stop_rmsd=stop_rmsd)
    assert ref[4].min_gap > GAP, f"the ensemble has a near-tie ({ref[4].min_gap:.3g}): choose another"
    for form in lanes:
        if form is not None:
            monkeypatch.setenv("FC_DIVERSE_LANES", form)
        got = fc.pruner.select_diverse(X, atoms, n=n, stop_rmsd=stop_rmsd, start=start,
                                       heavy_atoms_only=heavy_atoms_only)
        assert np.array_equal(got.indices, ref[0]), form
        assert got.labels.dtype == np.int32 and np.array_equal(got.labels, ref[1]), form
        assert np.abs(got.distances - ref[2]).max() < TOL, form
        assert np.isinf(got.radii[0]) and np.abs(got.radii[1:] - ref[3][1:]).max(initial=0.0) < TOL, form
        assert len(got.labels) == 0 or got.labels.max() < len(got.indices), form  # every label names a pick
    return got


def _ensemble(kind, N, A, seed):
    if kind == "clusters":
        X, atoms, _ = syn.synthetic_ensemble(N, A, seed=seed)
        return X, atoms
    return syn.continuous_ensemble(N, A, seed=seed), np.array(["C"] * A)


BOTH = ("1", "8")  # the step kernel's two forms: one lane per conformer, eight


@pytest.mark.parametrize("kind", ["clusters", "continuous"])
@pytest.mark.parametrize("N,A", [(1, 5), (2, 5), (64, 20), (257, 50), (600, 80), (300, 200)])
def test_diverse_parity(fc, monkeypatch, kind, N, A):
    """both lane forms of the step kernel against the restatement, n = all and n < N from another start"""
    X, atoms = _ensemble(kind, N, A, seed=N + A)
    _compare(fc, X, atoms, N, monkeypatch=monkeypatch, lanes=BOTH)
    if N > 2:
        _compare(fc, X, atoms, min(N - 1, 40), start=N // 3, monkeypatch=monkeypatch, lanes=BOTH)


def test_diverse_parity_beyond_the_lds_stage(fc, monkeypatch):
    """2 100 selected atoms: the representative no longer fits the kernel's LDS stage (2 048) and is read from HBM"""
    rng = np.random.default_rng(7)
    X = rng.normal(scale=4.0, size=(1, 2100, 3)) + rng.normal(scale=0.3, size=(40, 2100, 3))
    _compare(fc, X, np.array(["C"] * 2100), 12, start=5, monkeypatch=monkeypatch, lanes=BOTH)


NESTED = [1, 2, 3, 4, 5, 7, 8]  # the run 3-8-9-10-13-14-15-17-18-19 (tests/test_gpu_molecules.py, "nested")
BRANCH = [0, 9, 10, 11, 12]     # 1-33 and the two disjoint sides of 33 ("branch")


def _catalyst_scan(fc, golden, sel):
    from firecode_amd import torsion_perception as tp
    from firecode_amd.pruner import rotation_mask

    atoms = np.array([str(a) for a in golden["fx_catalyst_atoms"]])
    base = np.asarray(golden["fx_catalyst_coords"], dtype=np.float64)[0]
    graph = tp.graphize(atoms, base)
    torsions = tp.get_torsions(graph, double_bonds=tp.get_double_bonds_indices(base, atoms), mode="csearch")
    quads = np.array([torsions[k].torsion for k in sel], dtype=np.int64)
    masks = np.array([rotation_mask(graph, q, len(atoms)) for q in quads])
    grid = o.cartesian_product(*[FOLDS[int(torsions[k].n_fold)] for k in sel])
    return atoms, base, graph, [torsions[k] for k in sel], quads, masks, grid


def test_diverse_real_molecule(fc, golden):
    """the catalyst (85 atoms, 46 heavy, hydrogens between them) scanned over a torsion group of seven 3-fold bonds
    (2 187 conformers): heavy-atom selection.  (Symmetric rotamers of this molecule put some conformers at equal
    distances to a representative, within 1e-15; the first 40 picks from conformer 0 meet none of them -- the
    restatement's record shows it -- while longer selections do, where rounding may order them either way.)"""
    atoms, base, _, _, quads, masks, grid = _catalyst_scan(fc, golden, NESTED)
    X, _ = fc.torsion_module.torsion_scan(base, quads, masks, grid)
    ref_X, _ = o.torsion_scan(base, quads, masks, grid)
    assert len(X) == 2187 and np.abs(X - ref_X).max() < TOL
    got = _compare(fc, X, atoms, 40)
    assert len(got.indices) == 40


def test_diverse_clusters(fc):
    """K well-separated clusters and n = K: one representative per cluster, every label in the conformer's own"""
    for K, A, seed in ((12, 30, 1), (40, 50, 2)):
        X, atoms, cid = syn.synthetic_ensemble(5 * K, A, seed=seed)
        got = fc.pruner.select_diverse(X, atoms, n=K)
        assert sorted(cid[got.indices].tolist()) == list(range(K))
        assert np.array_equal(cid[got.indices][got.labels], cid)
        assert got.distances.max() < 0.3 < got.radii[-1]


def test_diverse_edges(fc):
    X, atoms, _ = syn.synthetic_ensemble(50, 20, seed=4)
    N = len(X)
    # n >= N selects everything: each label is the conformer's own position, each distance 0
    for n in (N, N + 7):
        got = fc.pruner.select_diverse(X, atoms, n=n, start=3)
        assert sorted(got.indices.tolist()) == list(range(N)) and got.indices[0] == 3
        assert np.array_equal(got.indices[got.labels], np.arange(N)) and np.all(got.distances == 0.0)
        assert np.all(np.diff(got.radii) <= 0.0)
    # exact duplicates: ties by lowest index; no copy is picked while a conformer at >= 1e-9 is uncovered
    rng = np.random.default_rng(8)
    D = syn.continuous_ensemble(30, 20, seed=9)
    src = rng.integers(0, 30, size=20)
    Y = np.concatenate([D, D[src]])
    perm = rng.permutation(len(Y))
    Y = Y[perm]
    group = np.concatenate([np.arange(30), src])[perm]  # the distinct conformer each row is a copy of
    lowest = {g: int(np.flatnonzero(group == g)[0]) for g in range(30)}
    got = fc.pruner.select_diverse(Y, np.array(["C"] * 20), n=len(Y))
    big = got.radii >= 1e-9
    assert big.sum() == 30 and np.all(big[:30])  # the 30 distinct ones first
    assert sorted(got.indices[:30].tolist()) == sorted(lowest.values())
    assert np.all(got.radii[30:] < 1e-9)
    # radius stop: at the first m <= stop_rmsd, and afterwards max D <= stop_rmsd
    full = fc.pruner.select_diverse(X, atoms, n=N)
    stop = 0.5 * (full.radii[9] + full.radii[10])
    got = _compare(fc, X, atoms, N, stop_rmsd=stop)
    assert np.array_equal(got.indices, full.indices[:10]) and got.distances.max() <= stop < got.radii[-1]
    only = fc.pruner.select_diverse(X, atoms, stop_rmsd=stop)
    assert np.array_equal(only.indices, got.indices)
    # a radius stop far beyond the first batch of 64 steps (277 picks)
    C = syn.continuous_ensemble(1000, 30, seed=3)
    got = _compare(fc, C, np.array(["C"] * 30), 1000, stop_rmsd=0.5)
    assert 64 < len(got.indices) < 1000 and got.distances.max() <= 0.5
    # energies: the first representative is the lowest energy (lowest index on ties)
    E = rng.normal(size=N)
    E[[17, 33]] = E.min() - 1.0
    got = fc.pruner.select_diverse(X, atoms, n=5, energies=E)
    assert got.indices[0] == 17
    assert np.array_equal(got.indices, fc.pruner.select_diverse(X, atoms, n=5, start=17).indices)
    # N = 0
    got = fc.pruner.select_diverse(np.zeros((0, 20, 3)), atoms, n=3)
    assert len(got.indices) == 0 and len(got.labels) == 0


def test_diverse_full_size(fc):
    """10^5 x 50, n = 200: the rows d(s_k, .) of the picks from fc_ensemble_rmsd_pairs, the greedy loop replayed on
    them in NumPy, and 2 048 sampled pairs against the oracle"""
    N, A, K = 100_000, 50, 200
    X = syn.continuous_ensemble(N, A, seed=21)
    atoms = np.array(["C"] * A)
    got = fc.pruner.select_diverse(X, atoms, n=K)
    assert len(got.indices) == K and len(set(got.indices.tolist())) == K
    ens = fc.DeviceEnsemble(X, atom_mask=np.ones(A, bool), center=True)
    try:
        j = np.arange(N, dtype=np.int64)
        rows = [ens.rmsd_pairs(np.full(N, s, dtype=np.int64), j)[0] for s in got.indices]
    finally:
        ens.close()
    idx, lab, dist = replay(rows, int(got.indices[0]), N, K)
    assert np.array_equal(idx, got.indices) and np.array_equal(lab, got.labels)
    assert np.abs(dist - got.distances).max() < TOL
    for k in range(1, K):  # the radius of pick k is its distance to the picks before it
        assert abs(got.radii[k] - min(rows[q][got.indices[k]] for q in range(k))) < TOL
    rng = np.random.default_rng(3)
    ks, js = rng.integers(0, K, 2048), rng.integers(0, N, 2048)
    ref = o.rmsd_and_max_batch(X[got.indices[ks]], X[js], center=True)[0]
    dev = np.array([rows[k][jj] for k, jj in zip(ks, js)])
    assert np.abs(dev - ref).max() < TOL


def test_diverse_csearch(fc, golden):
    """csearch mode 1: clustered_csearch_core(diversity="rmsd") keeps the starting structure first and then the
    greedy max-min selection of the TFD-pruned set; most_diverse_conformers(method="rmsd") and
    Ensemble.diversity_selection agree with select_diverse"""
    atoms, base, graph, torsions, quads, masks, _ = _catalyst_scan(fc, golden, BRANCH)
    rows = [tuple(int(v) for v in t.torsion) + (int(t.n_fold),) for t in torsions]
    pruned = fc.torsion_module.clustered_csearch_core(base, rows, masks, n_out=10 ** 6)
    n_out = 25
    assert len(pruned) > n_out
    out = fc.torsion_module.clustered_csearch_core(base, rows, masks, n_out=n_out, diversity="rmsd")
    sel = fc.pruner.select_diverse(pruned, atoms, n=n_out, start=0, heavy_atoms_only=False)
    assert out.shape == (n_out,) + base.shape
    assert np.array_equal(out[0], base) and np.array_equal(out, pruned[sel.indices])
    # clustered_csearch has the atoms: the heavy-atom RMSD, like every other RMSD stage
    out2 = fc.torsion_module.clustered_csearch(atoms, base, torsions, graph, n_out=n_out, logfunction=None,
                                               diversity="rmsd")
    sel_heavy = fc.pruner.select_diverse(pruned, atoms, n=n_out, start=0)
    assert np.array_equal(out2[0], base) and np.array_equal(out2, pruned[sel_heavy.indices])
    assert np.array_equal(out2, fc.torsion_module.clustered_csearch_core(base, rows, masks, n_out=n_out,
                                                                          diversity="rmsd", atoms=atoms))
    assert not np.array_equal(sel_heavy.indices, sel.indices)  # (the hydrogens do change the choice here)
    # the default keeps the reference's random draw
    rnd = fc.torsion_module.clustered_csearch_core(base, rows, masks, n_out=n_out, seed=4)
    assert np.array_equal(rnd, np.array(fc.torsion_module.most_diverse_conformers(n_out, list(pruned), seed=4)))
    # most_diverse_conformers(method="rmsd"): all atoms by default, heavy atoms with atoms=
    md = fc.torsion_module.most_diverse_conformers(10, list(pruned), method="rmsd")
    assert np.array_equal(np.array(md), pruned[sel.indices[:10]])
    md_h = fc.torsion_module.most_diverse_conformers(10, list(pruned), method="rmsd", atoms=atoms)
    sel_h = fc.pruner.select_diverse(pruned, atoms, n=10, start=0)
    assert np.array_equal(np.array(md_h), pruned[sel_h.indices])
    # at most n structures: all of them, in selection order
    few = pruned[:9]
    md_all = fc.torsion_module.most_diverse_conformers(20, list(few), method="rmsd", atoms=atoms)
    sel_all = fc.pruner.select_diverse(few, atoms, n=20, start=0)
    assert len(sel_all.indices) == 9 and np.array_equal(np.array(md_all), few[sel_all.indices])
    assert fc.torsion_module.most_diverse_conformers(3, [], method="rmsd") == []
    # Ensemble.diversity_selection: energies follow the kept structures, the lowest energy first
    from firecode_amd.ensemble import Ensemble

    E = np.random.default_rng(6).normal(size=len(pruned))
    lines = []
    ens = Ensemble(atoms=atoms, coords=pruned.copy(), energies=E.copy(), logfunction=lines.append)
    got = ens.diversity_selection(n=12)
    ref = fc.pruner.select_diverse(pruned, atoms, n=12, energies=E)
    assert np.array_equal(got.indices, ref.indices) and ref.indices[0] == int(np.argmin(E))
    assert np.array_equal(ens.coords, pruned[ref.indices]) and np.array_equal(ens.energies, E[ref.indices])
    assert len(lines) == 1 and lines[0].startswith(f"Kept 12 of {len(pruned)} candidates for RMSD diversity")
    ens2 = Ensemble(atoms=atoms, coords=pruned.copy(), energies=E.copy(), logfunction=None)
    cover = ens2.diversity_selection(stop_rmsd=0.5 * ref.radii[-1], verbose=False)
    assert len(ens2.coords) == len(ens2.energies) == len(cover.indices) > 12
