"""Symmetry- and mirror-aware RMSD-diverse selection on the GPU (fc_ensemble_select_diverse_perm and the Python layers
above it) against the NumPy restatement of its contract: ``diverse_ref.select_diverse`` with the d_sym row of
tests/diverse_sym_ref.py.

Bars, as in test_gpu_diverse.py: indices and labels identical, distances and radii within 1e-10 -- on ensembles whose
every decision (argmax, ``t < D[j]``, radius stop) the restatement recorded with a gap above 1e-9.  After every
symmetry-aware call the default selection and the default prune run on the same handle against their references."""

import functools
import os

import numpy as np
import pytest

import diverse_ref as dr
import diverse_sym_ref as ds
import enant_ref as er
import symm_ref as sr
from firecode_amd import symmetry as S
from firecode_amd import synthetic as syn
from oracle import cpu_ref as o

pytestmark = pytest.mark.gpu

TOL = 1e-10
GAP = 1e-9
BOTH = ("1", "8")  # the step kernel's two forms: one lane per conformer, eight

# kind, N, A, table, mirror, runs (seed 3 throughout: tests/diverse_sym_ref.ensemble).  runs: "a" n = all, "p" n < N from
# another start, "c" the cover at 0.5 A -- all three where the restatement's rows (N x A x K x handednesses each) take a few
# seconds together; the cover of the largest case and the default prune of its coordinates are recorded
# (tests/golden/make_golden_diverse_sym.py writes them with the same functions)
CASES = {
    "1x5-path-mirror": ("clusters", 1, 5, "path", True, "ac"),
    "2x5-path-mirror": ("clusters", 2, 5, "path", True, "ac"),
    "33x9-path": ("clusters", 33, 9, "path", False, "apc"),
    "257x20-path-mirror": ("clusters", 257, 20, "path", True, "apc"),
    "150x13-blocks-mirror": ("clusters", 150, 13, "blocks", True, "apc"),
    "300x50-blocks": ("clusters", 300, 50, "blocks", False, "pc"),
    "100x20-swaps64-mirror": ("clusters", 100, 20, "swaps64", True, "pc"),
    "257x50-identity-mirror": ("clusters", 257, 50, "identity", True, "apc"),
    "600x80-path-mirror": ("clusters", 600, 80, "path", True, "pc"),
    "continuous-257x50-path-mirror": ("continuous", 257, 50, "path", True, "apc"),
    "continuous-300x13-blocks-mirror": ("continuous", 300, 13, "blocks", True, "pc"),
    "64x3-planar-blocks-mirror": ("clusters", 64, 3, "blocks", True, "apc"),  # three atoms: every conformer its own mirror image
}
RECORDED = "600x80-path-mirror"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diverse_sym_v1.npz")


class Case:
    def __init__(self, name):
        kind, N, A, table, self.mirror, self.runs = CASES[name]
        self.X, self.atoms, self.table, self.cid = ds.ensemble(kind, N, A, table, self.mirror)
        self.N = N
        self.n_part = min(N - 1, 40 if N * len(self.table) < 6000 else 20)
        row, self._rows = ds.sym_row(self.table, self.mirror), {}
        self.row = lambda Xsel, s: self._rows[s] if s in self._rows else self._rows.setdefault(s, row(Xsel, s))
        self._refs = {}
        self.recorded = np.load(GOLDEN, allow_pickle=False) if name == RECORDED else None

    def ref(self, n, start=0, stop_rmsd=None):
        """the restatement's (indices, labels, distances, radii, smallest gap of any decision)"""
        key = (n, start, stop_rmsd)
        if key not in self._refs:
            if self.recorded is not None and key == (self.N, 0, 0.5):
                g = self.recorded
                self._refs[key] = (g["cover_indices"], g["cover_labels"], g["cover_distances"], g["cover_radii"],
                                   float(g["cover_min_gap"]))
            else:
                out = dr.select_diverse(self.X, n, start=start, stop_rmsd=stop_rmsd, row=self.row)
                self._refs[key] = out[:4] + (out[4].min_gap,)
        return self._refs[key]

    @functools.cached_property
    def default_refs(self):
        """what the default entry points give on these coordinates: a short selection and the prune's mask"""
        sel = dr.select_diverse(self.X, min(self.N, 6), start=0)
        if self.recorded is not None:
            return sel, self.recorded["prune_mask"]
        return sel, o.prune_by_rmsd(self.X, self.atoms, 0.5)[1]


@functools.lru_cache(maxsize=None)
def _case(name):
    return Case(name)


def _defaults_unchanged(ens, case):
    sel, mask = case.default_refs
    got = ens.select_diverse(min(case.N, 6))
    assert np.array_equal(got[0], sel[0]) and np.array_equal(got[1], sel[1])
    assert np.abs(got[2] - sel[2]).max() < TOL and np.abs(got[3][1:] - sel[3][1:]).max(initial=0.0) < TOL
    if case.N >= 2:
        assert np.array_equal(ens.prune(0.5, 1.0)[0], mask)


def _compare(ens, case, n, start=0, stop_rmsd=None, monkeypatch=None, lanes=(None,)):
    ref = case.ref(n, start, stop_rmsd)
    assert ref[4] > GAP, f"the ensemble has a near-tie ({ref[4]:.3g}): choose another"
    for form in lanes:
        if form is not None:
            monkeypatch.setenv("FC_DIVERSE_LANES", form)
        idx, lab, dist, rad = ens.select_diverse(n, start=start, stop_rmsd=stop_rmsd, symmetry=case.table,
                                                 prune_enantiomers=case.mirror)
        print(f"lanes={form} n={n} start={start} stop={stop_rmsd}: {len(idx)} picks, |d - ref| "
              f"{np.abs(dist - ref[2]).max():.2e}, gap {ref[4]:.2e}")
        assert np.array_equal(idx, ref[0]), form
        assert lab.dtype == np.int32 and np.array_equal(lab, ref[1]), form
        assert np.abs(dist - ref[2]).max() < TOL, form
        assert np.isinf(rad[0]) and np.abs(rad[1:] - ref[3][1:]).max(initial=0.0) < TOL, form
        assert lab.max() < len(idx), form
        _defaults_unchanged(ens, case)
    return idx, lab, dist, rad


@pytest.mark.parametrize("name", sorted(CASES))
def test_diverse_sym_parity(fc, monkeypatch, name):
    """both lane forms against the restatement: n = all, n < N from another start, and the cover at 0.5 A -- which on
    the clustered ensembles is exactly one representative per cluster, where the default call picks duplicates"""
    case = _case(name)
    N = case.N
    with fc.DeviceEnsemble(case.X, atom_mask=np.ones(len(case.atoms), bool), center=True) as ens:
        if "a" in case.runs:
            _compare(ens, case, N, monkeypatch=monkeypatch, lanes=BOTH)
        if "p" in case.runs:
            _compare(ens, case, case.n_part, start=N // 3, monkeypatch=monkeypatch, lanes=BOTH)
        idx, lab, dist, _ = _compare(ens, case, N, stop_rmsd=0.5, monkeypatch=monkeypatch, lanes=BOTH)
        assert dist.max() <= 0.5
        if case.cid is not None and N >= 33 and len(case.atoms) > 3:  # (three atoms: triangles, whose clusters overlap)
            K = len(np.unique(case.cid))
            assert sorted(case.cid[idx].tolist()) == list(range(K)) and np.array_equal(case.cid[idx][lab], case.cid)
            assert len(ens.select_diverse(N, stop_rmsd=0.5)[0]) > K


def test_first_row_is_d_sym(fc, monkeypatch):
    """n_max = 1: distances = d_sym(start, .) -- on an ensemble, on exact relabelled / reflected copies (0 within 1e-10)
    and on collinear structures (a covariance of rank one: the eigenvalue is double, the Jacobi sweeps take over)"""
    case = _case("150x13-blocks-mirror")
    ones = np.ones(13, bool)
    with fc.DeviceEnsemble(case.X, atom_mask=ones, center=True) as ens:
        for start in (0, 77):
            for form in BOTH:
                monkeypatch.setenv("FC_DIVERSE_LANES", form)
                idx, lab, dist, rad = ens.select_diverse(1, start=start, symmetry=case.table, prune_enantiomers=True)
                want = case.row(case.X, start).copy()
                want[start] = 0.0
                assert idx.tolist() == [start] and not lab.any() and np.abs(dist - want).max() < TOL
                _defaults_unchanged(ens, case)
    rng = np.random.default_rng(5)
    x = syn.continuous_ensemble(1, 13, seed=8)[0]
    copies = [x] + [x[row] @ syn.random_rotation(rng).T + rng.normal(size=3) for row in case.table[1:]]
    copies += [er.reflect(c[None], [0], axis=k % 3)[0] for k, c in enumerate(copies)]
    Y = np.ascontiguousarray(np.stack(copies + [syn.continuous_ensemble(2, 13, seed=9)[1]]))
    line = np.linspace(-3.0, 3.0, 13)[:, None] * np.array([[0.6, -0.3, 0.74]])
    Z = np.stack([(line * s)[::d] @ syn.random_rotation(rng).T for s in (1.0, 1.0, 1.1, 0.8) for d in (1, -1)])
    for W, table, zero in ((Y, case.table, np.arange(len(Y) - 1)), (Z, sr.path_table(13), np.arange(4))):
        want = ds.sym_row(table, True)(W, 0)
        assert np.abs(want[zero]).max() < 1e-12 and want[-1] > 0.05
        with fc.DeviceEnsemble(W, atom_mask=ones, center=True) as ens:
            for form in BOTH:
                monkeypatch.setenv("FC_DIVERSE_LANES", form)
                dist = ens.select_diverse(1, symmetry=table, prune_enantiomers=True)[2]
                assert np.abs(dist[zero]).max() < TOL and np.abs(dist - want).max() < TOL, form


def test_identity_table_is_the_default_bit_for_bit(fc, monkeypatch):
    X = syn.continuous_ensemble(300, 20, seed=6)
    ident = np.arange(20)[None]
    with fc.DeviceEnsemble(X, atom_mask=np.ones(20, bool), center=True) as ens:
        for form in BOTH:
            monkeypatch.setenv("FC_DIVERSE_LANES", form)
            for kw in ({"n_max": 300}, {"n_max": 50, "start": 9}, {"n_max": 300, "stop_rmsd": 0.5}):
                a, b = ens.select_diverse(**kw), ens.select_diverse(symmetry=ident, **kw)
                assert all(np.array_equal(u, v) for u, v in zip(a, b))


def test_largest_structure_the_lds_takes(fc):
    """K = 64 and the 1 077 selected atoms that just fit (the refusal of 1 078: tests/test_diverse_sym_cpu.py); N = 40,
    5 picks (the restatement's five rows are 64 alignments of 40 x 1 077 atoms each: no mirror images here)"""
    A = S.diverse_max_selected(64)
    assert A == 1077
    rng = np.random.default_rng(4)
    table = sr.transposition_table(A, 6)
    X = rng.normal(scale=4.0, size=(1, A, 3)) + rng.normal(scale=0.3, size=(40, A, 3))
    X, _ = sr.relabel_half(X, table, 4)
    ref = dr.select_diverse(X, 5, start=3, row=ds.sym_row(table, False))
    assert ref[4].min_gap > GAP
    with fc.DeviceEnsemble(X, atom_mask=np.ones(A, bool), center=True) as ens:
        idx, lab, dist, rad = ens.select_diverse(5, start=3, symmetry=table)
    assert np.array_equal(idx, ref[0]) and np.array_equal(lab, ref[1])
    assert np.abs(dist - ref[2]).max() < TOL and np.abs(rad[1:] - ref[3][1:]).max() < TOL


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


def test_drivers_pass_both_keywords_through(fc):
    """Ensemble.diversity_selection, most_diverse_conformers(method="rmsd") and a clustered search with diversity="rmsd"
    against pruner.select_diverse on the same input; a graph is perceived where the element symbols are known"""
    import networkx as nx

    from firecode_amd.ensemble import Ensemble
    from firecode_amd.pruner import rotation_mask

    case = _case("150x13-blocks-mirror")
    X, atoms, table = case.X, case.atoms, case.table
    kw = {"symmetry": table, "prune_enantiomers": True}
    ref = fc.pruner.select_diverse(X, atoms, n=30, start=0, **kw)
    want = case.ref(30)
    assert np.array_equal(ref.indices, want[0]) and np.array_equal(ref.labels, want[1])
    assert sorted(case.cid[ref.indices].tolist()) == list(range(30))  # one per cluster ...
    plain = fc.pruner.select_diverse(X, atoms, n=30, start=0)
    assert len(set(case.cid[plain.indices].tolist())) < 30            # ... which the default call does not give
    md = fc.torsion_module.most_diverse_conformers(30, list(X), method="rmsd", atoms=atoms, **kw)
    assert np.array_equal(np.array(md), X[ref.indices])
    md_all = fc.torsion_module.most_diverse_conformers(30, list(X), method="rmsd", **kw)  # all atoms: the same here
    assert np.array_equal(np.array(md_all), X[ref.indices])
    E = np.random.default_rng(6).normal(size=len(X))
    lines = []
    ens = Ensemble(atoms=atoms, coords=X.copy(), energies=E.copy(), logfunction=lines.append)
    got = ens.diversity_selection(n=30, **kw)
    by_energy = fc.pruner.select_diverse(X, atoms, n=30, energies=E, **kw)
    assert _same(got, by_energy) and got.indices[0] == int(np.argmin(E))
    assert np.array_equal(ens.coords, X[got.indices]) and np.array_equal(ens.energies, E[got.indices])
    assert len(lines) == 1 and lines[0].startswith(
        f"Kept 30 of {len(X)} candidates for RMSD diversity, 6 atom permutations, mirror images included (covering")
    # the star's graph (a centre and three arms of four) gives the table the case was built with
    star = nx.Graph([(0, 1 + 4 * m) for m in range(3)] + [(a, a + 1) for m in range(3) for a in range(1 + 4 * m, 4 + 4 * m)])
    assert _same(fc.pruner.select_diverse(X, atoms, n=30, start=0, symmetry=star, prune_enantiomers=True), ref)
    only_mirror = fc.pruner.select_diverse(X, atoms, n=30, start=0, prune_enantiomers=True)
    assert _same(only_mirror, fc.pruner.select_diverse(X, atoms, n=30, start=0, symmetry=np.arange(13)[None], prune_enantiomers=True))
    # csearch mode 1 on a symmetric chain of eight carbons: five 3-fold bonds, the path's reversal as its symmetry
    A = 8
    base = np.array([[1.25 * a, 0.9 * (a % 2), 0.0] for a in range(A)])
    catoms, chain = np.array(["C"] * A), nx.path_graph(A)
    rows = [(a, a + 1, a + 2, a + 3, 3) for a in range(A - 3)]
    masks = np.array([rotation_mask(chain, r[:4], A) for r in rows])
    ckw = {"symmetry": sr.path_table(A), "prune_enantiomers": True}
    pruned = fc.torsion_module.clustered_csearch_core(base, rows, masks, n_out=10 ** 6)
    n_out = 12
    assert len(pruned) > n_out
    out = fc.torsion_module.clustered_csearch_core(base, rows, masks, n_out=n_out, diversity="rmsd", atoms=catoms, **ckw)
    sel = fc.pruner.select_diverse(pruned, catoms, n=n_out, start=0, **ckw)
    assert out.shape == (n_out, A, 3) and np.array_equal(out, pruned[sel.indices])
    sel_plain = fc.pruner.select_diverse(pruned, catoms, n=n_out, start=0)
    assert not np.array_equal(sel.indices, sel_plain.indices)  # (the chain's mirror images and reversals do matter)


def test_bench_hook_under_d_sym(fc):
    """fc_bench_select_diverse_perm: the picks of the product call with the same arguments, and the two counters of a
    selection of its own -- every (conformer, permutation, handedness) of a step forms at most one eigenvalue, and only
    some of those go on to the explicit pass; with K = 1 and no mirror images it is the plain hook, and counts nothing"""
    N, A, n_max = 64, 12, 8
    X = syn.continuous_ensemble(N, A, seed=12)
    swap = np.arange(A)
    swap[[0, 1]] = 1, 0
    table = np.stack([np.arange(A), swap])
    with fc.DeviceEnsemble(X, atom_mask=np.ones(A, bool), center=True) as ens:
        want = ens.select_diverse(n_max, symmetry=table, prune_enantiomers=True)[0]
        dev, host, idx, (formed, explicit) = ens.bench_select_diverse(n_max, reps=2, symmetry=table, prune_enantiomers=True)
        print(f"device {dev:.3f} ms, host {host:.3f} ms, formed {formed}, explicit {explicit}")
        assert len(want) == n_max and np.array_equal(idx, want)
        assert 0 < explicit <= formed <= n_max * N * 2 * 2
        assert dev > 0.0 and host > 0.0
        plain = ens.bench_select_diverse(n_max, reps=2)
        ident = ens.bench_select_diverse(n_max, reps=2, symmetry=np.arange(A)[None])
        assert np.array_equal(ident[2], plain[2]) and np.array_equal(plain[2], ens.select_diverse(n_max)[0])
        assert ident[3] == (0, 0)
