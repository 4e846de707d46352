"""tests/degenerate_ref.py against the oracle (no GPU): the closed-form distances of the one-atom, two-atom and collinear
kinds and of the scaled family equal the oracle's Kabsch rows to 1e-12, the planar and mirrored kinds have the geometry
they promise, and every generator is seeded."""

import numpy as np
import pytest

import degenerate_ref as dg
import diverse_ref as dr
import diverse_sym_ref as ds
import enant_ref as er
import knn_cross_ref as xr
import knn_ref
import knn_sym_ref as ks
import symm_ref as sr
from oracle import cpu_ref as o

CLOSED = 1e-12
CHAIN = {"spacing": 1.4, "jitter": 0.02, "stretch": 0.05}


def _centred(X):
    return X - X.mean(axis=1, keepdims=True)


def test_one_atom_is_at_distance_zero():
    X = dg.one_atom(7)
    assert X.shape == (7, 1, 3) and np.abs(X).max() > 1.0
    D = knn_ref.distance_rows(X)
    assert np.all(D == 0.0)


def test_two_atoms_closed_form():
    r = dg.two_atoms_lengths(33)
    X = dg.two_atoms(33, r)
    assert np.abs(np.linalg.norm(X[:, 0] - X[:, 1], axis=1) - 2.0 * r).max() < 1e-14
    assert np.abs(knn_ref.distance_rows(X) - dg.two_atoms_distances(r)).max() < CLOSED
    rq = dg.two_atoms_lengths(9, seed=8)
    Q = dg.two_atoms(9, rq, seed=8)
    assert np.abs(xr.distance_rows(Q, X) - dg.two_atoms_distances(rq, r)).max() < CLOSED


@pytest.mark.parametrize("A", [3, 13, 40])
def test_collinear_closed_form(A):
    """also under the path's reversal table and with the mirror flag (a line is its own mirror image)"""
    X, t = dg.collinear(40, A, CHAIN, seed=A)
    Xc = _centred(X)
    # rank one: the second singular value of every centred conformer vanishes
    assert max(np.linalg.svd(c, compute_uv=False)[1] for c in Xc) < 1e-13
    assert np.abs(np.linalg.norm(Xc, axis=2) - np.abs(t)).max() < 1e-13
    rev = np.sign(np.diff(t, axis=1)[:, 0] * (t[:, -1] - t[:, 0]))  # (laid out monotonically, in either direction)
    assert np.all(rev == 1.0)
    D = dg.collinear_distances(t)
    assert np.abs(knn_ref.distance_rows(X) - D).max() < CLOSED
    table = sr.path_table(A)
    Dsym = dg.collinear_distances(t, reversal=True)
    for mirror in (False, True):
        assert np.abs(ds.matrix(X, table, mirror) - Dsym).max() < CLOSED
    assert np.abs(ds.matrix(X, np.arange(A)[None], True) - D).max() < CLOSED
    Q, tq = dg.collinear(6, A, CHAIN, seed=A + 100)
    assert np.abs(xr.distance_rows(Q, X) - dg.collinear_distances(tq, t)).max() < CLOSED


def test_half_of_the_chains_are_reversed():
    _, t = dg.collinear(200, 13, CHAIN)
    up = (t[:, -1] > t[:, 0]).mean()
    assert 0.35 < up < 0.65


def test_planar_structures_are_their_own_mirror_images():
    X = dg.planar(30, 12)
    Xc = _centred(X)
    assert max(np.linalg.svd(c, compute_uv=False)[2] for c in Xc) < 1e-13  # rank two
    B = np.einsum("ai,aj->ij", Xc[0], Xc[1])
    assert abs(np.linalg.det(B)) < 1e-10 * np.linalg.norm(B) ** 3
    D = knn_ref.distance_rows(X)
    assert np.abs(ds.matrix(X, np.arange(12)[None], True) - D).max() < CLOSED
    off = D[~np.eye(30, dtype=bool)]
    assert off.min() > 0.05


def test_mirrored_tops_have_a_double_root_against_their_image():
    N, A = 21, 12
    X, image_of = dg.mirrored_tops(N, A)
    n0 = (N + 1) // 2
    assert np.array_equal(image_of[:N - n0], np.arange(n0, N)) and image_of[N - n0:n0].tolist() == [-1] * (2 * n0 - N)
    Xc = _centred(X)
    for i in range(N):
        m = np.sort(np.linalg.eigvalsh(Xc[i].T @ Xc[i]))
        assert abs(m[0] - m[1]) < 1e-12 * m[2] and m[2] > 2.0 * m[1]  # the two smallest second moments are equal
    plain = knn_ref.distance_rows(X)
    aware = ds.matrix(X, np.arange(A)[None], True)
    for i in np.flatnonzero(image_of >= 0):
        j = image_of[i]
        s = np.linalg.svd(np.einsum("ai,aj->ij", Xc[i], Xc[j]), compute_uv=False)
        assert abs(s[1] - s[2]) < 1e-12 * s[0] and np.linalg.det(np.einsum("ai,aj->ij", Xc[i], Xc[j])) < 0.0
        assert aware[i, j] < CLOSED and plain[i, j] > 0.1
        others = np.delete(plain[i], [i, j])
        assert others.min() < plain[i, j]  # without the flag the image is not the nearest neighbour


GAP = 1e-9


@pytest.mark.parametrize("cap", [0.05, 0.25])
@pytest.mark.parametrize("name", dg.SCALED_BASES)
def test_scaled_family_closed_forms(name, cap):
    """128 conformers a hair inside and outside ``cap`` of the reference: the closed-form RMSD and max-deviation matrices
    against the oracle's; every pair more than GAP from both thresholds under both threshold settings, and the oracle's
    own bits -- plain, with the mirror flag, under the reversal table -- are the closed form's; under the reversal table
    with the mirror flag the distance is the plain one"""
    b = dg.scaled_base(name)
    A = len(b)
    assert np.abs(b.mean(axis=0)).max() < 1e-13 and A == {"full": 23, "planar": 12, "line": 40, "full224": 224}[name]
    assert np.linalg.matrix_rank(b, tol=1e-9) == {"full": 3, "planar": 2, "line": 1, "full224": 3}[name]
    assert 1.0 < dg.base_reach(b) / dg.base_rms(b) < 4.0  # (max_dev = 4 cap is clear at the RMSD edge)
    X, a = dg.scaled_family(b, dg.knife_offsets(cap, 128), seed=A)
    assert X.shape == (129, A, 3) and a[-1] == 1.0 and 40 < (a[:-1] > 1.0).sum() < 88
    R, M = dg.scaled_rmsd(b, a), dg.scaled_maxdev(b, a)
    assert np.abs(R[:-1, -1] - dg.knife_offsets(cap, 128)).max() < 1e-14
    atoms = np.array(["C"] * A)
    _, R0, M0 = o.rmsd_similarity_matrix(X, atoms, cap)
    print(f"{name} cap={cap}: max|R - oracle|={np.abs(R - R0).max():.3g} max|M - oracle|={np.abs(M - M0).max():.3g}")
    assert np.abs(R - R0).max() < CLOSED and np.abs(M - M0).max() < CLOSED
    iu = np.triu_indices(129, 1)
    for edge in ("rmsd", "dev"):
        thr, dev = dg.knife_thresholds(b, cap, edge)
        gap = min(np.abs(R[iu] - thr).min(), np.abs(M[iu] - dev)[R[iu] < thr].min())
        S = (R < thr) & (M < dev) & ~np.eye(129, dtype=bool)
        edge_pairs = S[:-1, -1]
        print(f"  {edge} edge: thr={thr:.6g} dev={dev:.6g} gap={gap:.3g}, {int(edge_pairs.sum())} of 128 inside")
        assert gap > GAP and np.array_equal(edge_pairs, np.arange(128) < 64)
        assert np.array_equal(o.rmsd_similarity_matrix(X, atoms, thr, dev)[0], S)
        mats = er.similarity(X, atoms, thr, dev)
        assert mats.min_gap > GAP and np.array_equal(mats.S, S)
        if A <= 40:
            sym = sr.similarity(X, atoms, sr.path_table(A), thr, dev)
            assert sym.min_gap > GAP and np.array_equal(sym.S, S)
    if A <= 40:
        rows = np.arange(0, 129, 8)
        assert np.abs(ks.distance_rows(X[rows], X, sr.path_table(A), mirror=True) - R[rows]).max() < CLOSED


def test_generators_are_seeded():
    for make in (lambda s: dg.one_atom(5, seed=s), lambda s: dg.two_atoms(5, dg.two_atoms_lengths(5), seed=s),
                 lambda s: dg.collinear(5, 13, CHAIN, seed=s)[0], lambda s: dg.planar(5, 12, seed=s),
                 lambda s: dg.mirrored_tops(5, 12, seed=s)[0],
                 lambda s: dg.scaled_family(dg.scaled_base("full"), dg.knife_offsets(0.25, 5), seed=s)[0]):
        assert np.array_equal(make(3), make(3)) and not np.array_equal(make(3), make(4))


def test_restatements_take_the_degenerate_rows():
    """the lists and the selection of the existing restatements run on these rows, ties at distance 0 included"""
    X = dg.one_atom(6)
    ref = knn_ref.knn(X, 3)
    assert np.array_equal(ref.indices[0], [1, 2, 3]) and np.array_equal(ref.indices[4], [0, 1, 2]) and ref.min_gap == 0.0
    idx, lab, dist, rad, _ = dr.select_diverse(X, 6, start=2)
    assert idx.tolist() == [2, 0, 1, 3, 4, 5] and np.all(dist == 0.0) and np.all(rad[1:] == 0.0)
    assert dr.select_diverse(X, 6, start=2, stop_rmsd=0.0)[0].tolist() == [2]
