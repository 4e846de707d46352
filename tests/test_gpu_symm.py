"""Symmetry-aware RMSD prune on the GPU (fc_prune_rmsd_perm, fc_rmsd_simbits_perm, fc_rmsd_clusters_perm,
fc_ensemble_rmsd_pairs_perm and the Python layers above them) against the NumPy restatement of the contract
(tests/symm_ref.py on oracle.cpu_ref).

Bars: masks, similarity bits, counts and clusters identical; values within 1e-10, the max deviation widened only by the
pair's own conditioning (oracle.rotation_error_bound_batch).  Every ensemble asserts ``min_gap > 1e-9`` from the
restatement first, so no pair is ever exempted."""

import functools

import networkx as nx
import numpy as np
import pytest

import dbscan_ref as dr
import symm_ref as sr
from firecode_amd import synthetic as syn
from oracle import cpu_ref as o

pytestmark = pytest.mark.gpu

TOL = 1e-10
GAP = 1e-9
THR = 0.5
TILE = 16        # conformers per side of a tile of the all-pairs kernel (fc_symm.hip)
SHARE = 8        # workgroups that share the column tiles of one row tile
LDS = 160 * 1024


def lds_bytes(A, K):
    """the tile of the contract (include/fc_hip.h): two coordinate tiles of 16 conformers at an odd stride, the table, and
    the queue of candidate pairs (512 entries of two words, and its fill level)"""
    return 2 * TILE * ((3 * A) | 1) * 8 + (2 * K * A + 7) // 8 * 8 + 2 * 512 * 8 + 8


def largest_A(K):
    A = 1
    while lds_bytes(A + 1, K) <= LDS:
        A += 1
    return A


# ---- tables and ensembles ------------------------------------------------------------------------------------------------
def _table(kind, A):
    if kind == "ident":
        return np.arange(A)[None]
    if kind == "path":
        return sr.path_table(A)
    if kind == "swap01":  # a single transposition
        return sr.transposition_table(A, 1)
    if kind == "blocks":  # S3 on three runs of atoms: the three-arm star at A = 13, all of S3 at A = 3
        return sr.block_table(A, (A - 1) // 3 if A > 3 else 1, first=1 if A > 3 else 0)
    if kind == "swaps64":
        return sr.transposition_table(A, 6)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def _case(kind, N, A, seed):
    """a clustered ensemble with a random half of its conformers relabelled by a random non-identity row of the table"""
    table = _table(kind, A)
    X, atoms, assign = syn.synthetic_ensemble(N, A, seed=seed)
    Y, which = sr.relabel_half(X, table, seed)
    return Y, atoms, table, assign


@functools.lru_cache(maxsize=None)
def _reference(kind, N, A, seed, thr=THR):
    Y, atoms, table, _ = _case(kind, N, A, seed)
    mats = sr.similarity(Y, atoms, table, thr)
    assert mats.min_gap > GAP, f"{(kind, N, A, seed)}: a decisive value within {mats.min_gap:.3g} of its threshold: choose another seed"
    return mats, o.greedy_prune_from_matrix(mats.S), o.greedy_prune_from_matrix(mats.S_default)


def _device_results(fc, X, table, thr=THR):
    """default prune, the symmetry-aware bits, prune, clusters and values, then the default calls again, on ONE handle"""
    from firecode_amd import _lib

    out = {}
    n = len(X)
    iu, ju = np.triu_indices(n, 1)
    pick = np.random.default_rng(0).choice(len(iu), size=min(len(iu), 300), replace=False)
    with fc.DeviceEnsemble(X, center=True) as ens:
        out["mask_default_before"], _ = ens.prune(thr, 2 * thr)
        bits, out["grey"] = ens.simbits(thr, 2 * thr, symmetry=table)
        out["bits"] = _lib.unpack_bits(bits, n)
        out["mask"], out["stats"] = ens.prune(thr, 2 * thr, symmetry=table)
        out["clusters"] = ens.clusters(thr, 2 * thr, symmetry=table)
        if len(pick):
            out["pairs"] = np.stack([iu[pick], ju[pick]])
            out["values"] = ens.rmsd_pairs(iu[pick], ju[pick], symmetry=table)
        # nothing moved: the default calls in the same process, on the same handle, after the symmetry-aware ones
        out["mask_default"], out["stats_default"] = ens.prune(thr, 2 * thr)
        bits0, out["grey_default"] = ens.simbits(thr, 2 * thr)
        out["bits_default"] = _lib.unpack_bits(bits0, n)
        out["clusters_default"] = ens.clusters(thr, 2 * thr)
        if len(pick):
            out["values_default"] = ens.rmsd_pairs(iu[pick], ju[pick])
    return out


def _assert_parity(got, mats, mask_sym, mask_default, X, table, label=""):
    n = len(mask_sym)
    upper = np.triu(mats.S, 1)
    assert np.array_equal(got["bits"], upper), label
    assert np.array_equal(got["mask"], mask_sym), label
    assert int(got["grey"]) == 0 and int(got["stats"][3]) == 0, label
    assert int(got["stats"][0]) == n * (n - 1) // 2 and int(got["stats"][2]) == int(upper.sum()), label
    assert int(got["stats"][1]) >= int(got["stats"][2]) and int(got["stats"][5]) == int(mask_sym.sum()), label
    labels, reps, sizes, cstats = got["clusters"]
    l0, r0, s0 = sr.components(mats.S)
    assert np.array_equal(labels, l0) and np.array_equal(reps, r0) and np.array_equal(sizes, s0), label
    assert int(cstats[2]) == int(upper.sum()) and int(cstats[3]) == 0 and int(cstats[5]) == len(r0), label
    # nothing moved
    for key in ("mask_default_before", "mask_default"):
        assert np.array_equal(got[key], mask_default), (label, key)
    assert np.array_equal(got["bits_default"], np.triu(mats.S_default, 1)) and int(got["grey_default"]) == 0, label
    assert int(got["stats_default"][2]) == int(np.triu(mats.S_default, 1).sum()), label
    ld, rd, sd = sr.components(mats.S_default)
    assert np.array_equal(got["clusters_default"][0], ld) and np.array_equal(got["clusters_default"][2], sd), label
    if "pairs" in got:
        i, j = got["pairs"]
        r, m = got["values"]
        Xp = sr.prepared(X, np.array(["C"] * X.shape[1]))
        assert r.shape == m.shape == (len(i), len(table)), label
        for k, perm in enumerate(table):
            bound = o.rotation_error_bound_batch(Xp[i], Xp[j][:, perm])
            assert np.abs(r[:, k] - mats.R[k, i, j]).max() < TOL, (label, k)
            assert np.all(np.abs(m[:, k] - mats.M[k, i, j]) <= TOL + bound), (label, k)
        assert np.abs(got["values_default"][0] - mats.R[0, i, j]).max() < TOL, label


# ---- 1. values -----------------------------------------------------------------------------------------------------------
def _value_structures(kind, A, rng, n=16):
    if kind == "random":
        P, Q = rng.normal(scale=2.0, size=(n, A, 3)), rng.normal(scale=2.0, size=(n, A, 3))
    elif kind == "clustered":
        P = rng.normal(scale=2.0, size=(n, A, 3))
        Q = np.stack([p @ syn.random_rotation(rng).T for p in P]) + rng.normal(scale=0.05, size=(n, A, 3))
    else:  # degenerate: the first pair planar, the second collinear, the rest random
        P, Q = rng.normal(scale=2.0, size=(n, A, 3)), rng.normal(scale=2.0, size=(n, A, 3))
        P[0, :, 2] = 0.0
        Q[0, :, 2] = 0.0
        P[1] = rng.normal(scale=2.0, size=(A, 1)) * np.array([1.0, 0.0, 0.0])
        Q[1] = rng.normal(scale=2.0, size=(A, 1)) * np.array([0.0, 1.0, 0.0])
    return P + rng.normal(scale=3.0, size=(n, 1, 3)), Q + rng.normal(scale=3.0, size=(n, 1, 3))


VALUE_TABLES = [("ident", 1), ("path", 2), ("swap01", 2), ("blocks", 6)]


@pytest.mark.parametrize("kind", ["random", "clustered", "degenerate"])
@pytest.mark.parametrize("A", [3, 9, 13, 50, 200])
def test_pair_values(fc, kind, A):
    """all K values of each pair against the oracle on (p, q[perm]): K = 1, 2 and 6; a derangement (the reversal at even A,
    the three-cycles of the block table), a single transposition; a planar and a collinear pair"""
    rng = np.random.default_rng(100 + A)
    P, Q = _value_structures(kind, A, rng)
    n = len(P)
    X = np.concatenate([P, Q])
    pi, pj = np.arange(n), np.arange(n) + n
    Pc, Qc = P - P.mean(axis=1, keepdims=True), Q - Q.mean(axis=1, keepdims=True)
    with fc.DeviceEnsemble(X, center=True) as ens:
        for name, K in VALUE_TABLES:
            table = _table(name, A)
            assert len(table) == K
            r, m = ens.rmsd_pairs(pi, pj, symmetry=table)
            assert r.shape == m.shape == (n, K)
            for k, perm in enumerate(table):
                r0, m0 = o.rmsd_and_max_batch(Pc, Qc[:, perm])
                bound = o.rotation_error_bound_batch(Pc, Qc[:, perm])
                assert np.abs(r[:, k] - r0).max() < TOL, (kind, A, name, k)
                fin = np.isfinite(bound)
                assert np.all(np.abs(m[:, k] - m0)[fin] <= TOL + bound[fin]), (kind, A, name, k)
                if kind == "degenerate":
                    assert np.isinf(bound[1]) and np.isfinite(bound[2:]).all()
                else:
                    assert fin.all()
        rd, md = ens.rmsd_pairs(pi, pj)  # the default call on the same handle
    r0, m0 = o.rmsd_and_max_batch(Pc, Qc)
    assert np.abs(rd - r0).max() < TOL
    # the drop-in name: a table over all atoms and an atom mask
    am = np.ones(A, dtype=bool)
    if A > 3:
        am[A - 1] = False  # (the last atom: fixed by the transposition of atoms 0 and 1)
    table = _table("swap01", A)
    r, m = fc.rmsd.rmsd_and_max_batch(X, pi, pj, center=True, atom_mask=am, symmetry=table)
    sel = sr.selected(table, am)
    Ps, Qs = P[:, am] - P[:, am].mean(axis=1, keepdims=True), Q[:, am] - Q[:, am].mean(axis=1, keepdims=True)
    for k, perm in enumerate(sel):
        r0, m0 = o.rmsd_and_max_batch(Ps, Qs[:, perm])
        bound = o.rotation_error_bound_batch(Ps, Qs[:, perm])
        fin = np.isfinite(bound)
        assert np.abs(r[:, k] - r0).max() < TOL and np.all(np.abs(m[:, k] - m0)[fin] <= TOL + bound[fin]), (kind, A, k)


# ---- 2. masks, bits, counts and clusters ---------------------------------------------------------------------------------
PARITY = (
    # N at each side of the tile edges in rows and columns (16), of the column share (8 tiles = 128) and of the bit words (64)
    [("path", n, 9, 1) for n in (1, 2, TILE - 1, TILE, TILE + 1, 63, 64, 65, TILE * SHARE, TILE * SHARE + 1, 150)]
    + [("blocks", 150, 13, 2)]                                         # the three-arm star, K = 6
    + [("path", 64, 3, 5), ("blocks", 64, 3, 6), ("path", 150, 30, 3), ("path", 150, 80, 4)]  # atom counts
    + [("ident", 150, 9, 1), ("swap01", 65, 13, 7), ("swaps64", 65, 13, 8)]                 # K = 1; one transposition; K = 64
)


@pytest.mark.parametrize("kind,N,A,seed", PARITY)
def test_prune_parity_relabelled_half(fc, kind, N, A, seed):
    Y, atoms, table, assign = _case(kind, N, A, seed)
    mats, mask_sym, mask_default = _reference(kind, N, A, seed)
    _assert_parity(_device_results(fc, Y, table), mats, mask_sym, mask_default, Y, table, (kind, N, A, seed))
    if kind == "ident":  # K = 1: the default prune's bits and mask, bit for bit
        assert np.array_equal(mats.S, mats.S_default) and np.array_equal(mask_sym, mask_default)
    if N == 150 and A >= 9 and kind != "ident":  # survivors: one per cluster; the default prune keeps about twice as many
        assert int(mask_sym.sum()) == len(np.unique(assign)) == 30
        assert int(mask_default.sum()) > 1.5 * 30
    if (kind, N, A, seed) == ("path", 150, 9, 1):
        assert np.array_equal(mask_default, o.prune_by_rmsd(Y, atoms, THR)[1])


def test_largest_atom_count_and_the_refusal_one_above_it(fc):
    K = 2
    A = largest_A(K)
    assert lds_bytes(A, K) <= LDS < lds_bytes(A + 1, K) and A > 200
    Y, atoms, table, _ = _case("path", 20, A, 9)
    mats, mask_sym, mask_default = _reference("path", 20, A, 9)
    _assert_parity(_device_results(fc, Y, table), mats, mask_sym, mask_default, Y, table, "largest A")
    from firecode_amd import _lib

    Z = np.concatenate([Y, Y[:, :1] + 1.0], axis=1)
    big = sr.path_table(A + 1)
    with fc.DeviceEnsemble(Z, center=True) as ens:
        for call in (lambda: ens.prune(THR, 2 * THR, symmetry=big), lambda: ens.simbits(THR, 2 * THR, symmetry=big),
                     lambda: ens.clusters(THR, 2 * THR, symmetry=big)):
            with pytest.raises(fc.FirecodeHipInputError, match="LDS") as err:
                call()
            assert err.value.code == _lib.FC_E_LIMIT
        r, _ = ens.rmsd_pairs([0], [1], symmetry=big)  # the value call stages nothing in LDS
        assert r.shape == (1, 2)
        m0, _ = ens.prune(THR, 2 * THR)  # the handle is as good as before
    assert np.array_equal(m0, o.prune_by_rmsd(Z, np.array(["C"] * (A + 1)), THR)[1])


def test_table_of_another_width_is_refused_on_the_handle(fc):
    Y, atoms, table, _ = _case("path", 16, 9, 1)
    with fc.DeviceEnsemble(Y, center=True) as ens:
        with pytest.raises(fc.FirecodeHipInputError):
            ens.prune(THR, 2 * THR, symmetry=sr.path_table(8))
        with pytest.raises(fc.FirecodeHipInputError, match="twin"):
            ens.twin().prune(THR, 2 * THR, symmetry=table)


def test_overflowed_pair_queue_takes_the_bit_matrix(fc, monkeypatch):
    """more similar pairs than the ensemble's pair queue holds (its capacity forced down): the ladder and the labelling
    decline the incomplete list on the device and run from the bit matrix the same launch wrote"""
    Y, atoms, table, _ = _case("blocks", 150, 13, 2)
    mats, mask_sym, mask_default = _reference("blocks", 150, 13, 2)
    assert int(np.triu(mats.S, 1).sum()) > 64
    monkeypatch.setenv("FC_PAIRQ_CAP", "64")
    with fc.DeviceEnsemble(Y, center=True) as ens:
        mask, stats = ens.prune(THR, 2 * THR, symmetry=table)
        labels, reps, sizes, cstats = ens.clusters(THR, 2 * THR, symmetry=table)
        monkeypatch.delenv("FC_PAIRQ_CAP")
        mask_again, stats_again = ens.prune(THR, 2 * THR, symmetry=table)
        mask0, _ = ens.prune(THR, 2 * THR)
    l0, r0, s0 = sr.components(mats.S)
    assert np.array_equal(mask, mask_sym) and int(stats[2]) == int(np.triu(mats.S, 1).sum()) and int(stats[5]) == 30
    assert np.array_equal(labels, l0) and np.array_equal(reps, r0) and np.array_equal(sizes, s0) and int(cstats[4]) == 1
    assert np.array_equal(mask_again, mask_sym) and np.array_equal(stats_again[:4], stats[:4])
    assert np.array_equal(mask0, mask_default)


def test_overflowed_pair_queue_takes_the_bit_matrix_dbscan(fc, monkeypatch):
    """the density-based twin of the test above: the degree pass declines the incomplete list on the device and the core
    rule runs from the bit matrix the same launch wrote; without the cap the pair list gives the same answer"""
    Y, atoms, table, _ = _case("blocks", 150, 13, 2)
    mats, _, _ = _reference("blocks", 150, 13, 2)
    # the case as worked out on the CPU: a graph that quietly stopped overflowing the cap of 64 fails here
    assert int(np.triu(mats.S, 1).sum()) == 300 and int(np.triu(mats.S_default, 1).sum()) == 79 and mats.min_gap > 0.4
    assert np.array_equal(mats.S.sum(axis=1) - np.diag(mats.S), np.full(150, 4))
    want = {m: dr.dbscan_from_matrix(mats.S, m) for m in (1, 5, 6)}
    for m in (1, 5):
        assert len(want[m].representatives) == 30 and int(want[m].core.sum()) == 150
    assert len(want[6].representatives) == 0 and int((want[6].labels < 0).sum()) == 150

    def run(ens, from_bits):
        got = {m: ens.dbscan(THR, 2 * THR, m, symmetry=table) for m in (1, 5, 6)}
        for m, (labels, reps, sizes, core, degrees, stats) in got.items():
            for field, have in zip(dr.RefDbscan._fields, (labels, reps, sizes, core, degrees)):
                assert np.array_equal(have, getattr(want[m], field)), (from_bits, m, field)
            assert int(stats[2]) == 300 and int(stats[3]) == 0 and int(stats[4]) == from_bits, (from_bits, m)
            assert int(stats[5]) == len(reps) and int(stats[6]) == int(core.sum()), (from_bits, m)
            assert int(stats[7]) == int((labels < 0).sum()), (from_bits, m)
        return got

    monkeypatch.setenv("FC_PAIRQ_CAP", "64")
    with fc.DeviceEnsemble(Y, center=True) as ens:
        capped = run(ens, 1)
        components = ens.clusters(THR, 2 * THR, symmetry=table)
        monkeypatch.delenv("FC_PAIRQ_CAP")
        listed = run(ens, 0)
    assert int(components[3][4]) == 1 and np.array_equal(capped[1][0], components[0])
    for m in (1, 5, 6):
        for a, b in zip(capped[m][:5], listed[m][:5]):
            assert a.dtype == b.dtype and np.array_equal(a, b), m


# ---- 3. the OR of complete tests -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta,cross_similar", [(0.4, True), (0.7, False)])
def test_geometrically_symmetric_skeleton(fc, delta, cross_similar):
    """two arms related by a twofold axis up to ``delta``: within a family both k pass the rmsd and the swap fails on its
    max deviation; across the families the identity has the SMALLER rmsd and fails on its max deviation, while the swap
    passes completely (delta = 0.4: similar, which "the smallest rmsd, then its max deviation" would miss) or fails its
    rmsd and passes its max deviation (delta = 0.7: dissimilar, which "some r_k and some m_k pass" would miss)"""
    X, atoms, table, family = sr.two_arm_families(20, 20, delta, seed=1)
    mats = sr.similarity(X, atoms, table, THR)
    assert mats.min_gap > GAP
    iu, ju = np.triu_indices(len(X), 1)
    cross = family[iu] != family[ju]
    r, m = mats.R[:, iu, ju], mats.M[:, iu, ju]
    assert np.all(r[0][cross] < r[1][cross]) and np.all(r[0][cross] < THR) and np.all(m[0][cross] > 2 * THR)
    assert np.all(m[1][cross] < 2 * THR) and np.all((r[1][cross] < THR) == cross_similar)
    assert np.all(r[1][~cross] < THR) == (delta == 0.4) and np.all(m[1][~cross] > 2 * THR)
    assert np.all(mats.S[iu, ju][cross] == cross_similar) and np.all(mats.S[iu, ju][~cross])
    assert not mats.S_default[iu, ju][cross].any()
    mask_sym, mask_default = o.greedy_prune_from_matrix(mats.S), o.greedy_prune_from_matrix(mats.S_default)
    assert int(mask_sym.sum()) == (1 if cross_similar else 2) and int(mask_default.sum()) == 2
    _assert_parity(_device_results(fc, X, table), mats, mask_sym, mask_default, X, table, delta)


# ---- 4. energy window, ladder rule ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("drop", ["earlier", "later"])
def test_energy_window_and_ladder_rule(fc, drop):
    Y, atoms, table, _ = _case("path", 150, 9, 1)
    mats, _, _ = _reference("path", 150, 9, 1)
    en = np.random.default_rng(4).normal(size=150)
    dE = np.abs(en[:, None] - en[None, :])[np.triu_indices(150, 1)]
    assert np.abs(dE - 0.8).min() > 1e-9
    _, ref, _ = sr.prune_by_rmsd_sym(Y, atoms, table, THR, energies=en, max_dE=0.8, drop=drop, min_per_group=3)
    _, ref_default = o.prune_by_rmsd(Y, atoms, THR, energies=en, max_dE=0.8, drop=drop)
    saved = fc.pruner.CONVENTIONS["drop"]
    fc.pruner.CONVENTIONS["drop"] = drop
    try:
        kept, mask = fc.pruner.prune_by_rmsd(Y, atoms, THR, energies=en, max_dE=0.8, symmetry=table, min_per_group=3)
        _, mask_default = fc.pruner.prune_by_rmsd(Y, atoms, THR, energies=en, max_dE=0.8)
        order = np.argsort(en, kind="stable")
        with fc.DeviceEnsemble(Y[order], center=True) as ens:
            bits, grey = ens.simbits(THR, 2 * THR, energies=en[order], max_dE=0.8, symmetry=table)
            cl = fc.pruner.cluster_by_rmsd(Y, atoms, THR, energies=en, max_dE=0.8, symmetry=table)
    finally:
        fc.pruner.CONVENTIONS["drop"] = saved
        fc.pruner._thresholds(None, None, 0.0)  # (the process-wide switch back where it was)
    assert np.array_equal(mask, ref) and np.array_equal(kept, Y[ref])
    assert np.array_equal(mask_default, ref_default) and mask.sum() < mask_default.sum()
    assert grey == 0 and np.array_equal(bits, sr.pack_bits(mats.S[np.ix_(order, order)], en[order], 0.8))
    # clusters: the components of the windowed graph in processing order, reported in the caller's order
    Sw = mats.S[np.ix_(order, order)] & (np.abs(en[order][:, None] - en[order][None, :]) < 0.8)
    l0, r0, s0 = sr.components(Sw)
    labels = np.empty_like(l0)
    labels[order] = l0
    assert np.array_equal(cl.labels, labels) and np.array_equal(cl.representatives, order[r0]) and np.array_equal(cl.sizes, s0)


# ---- 5. drivers ----------------------------------------------------------------------------------------------------------
def test_drivers_and_their_log_lines(fc):
    Y, atoms, table, assign = _case("path", 150, 9, 1)
    mats, mask_sym, mask_default = _reference("path", 150, 9, 1)
    graph = nx.path_graph(9)
    assert np.array_equal(fc.symmetry.graph_automorphisms(graph, atoms), table)
    lines = []
    for sym in (table, graph):
        kept, mask = fc.pruner.prune_by_rmsd(Y, atoms, THR, symmetry=sym, debugfunction=lines.append)
        assert np.array_equal(mask, mask_sym) and np.array_equal(kept, Y[mask_sym])
        assert lines[-1].startswith("DEBUG: prune_by_rmsd [gfx950, 2 atom permutations] - 11175 pairs screened, ")
        assert f"keeping {int(mask_sym.sum())}/150" in lines[-1] and " 0 grey, " in lines[-1]
        cl = fc.pruner.cluster_by_rmsd(Y, atoms, THR, symmetry=sym, debugfunction=lines.append)
        l0, r0, s0 = sr.components(mats.S)
        assert np.array_equal(cl.labels, l0) and np.array_equal(cl.representatives, r0) and np.array_equal(cl.sizes, s0)
        assert lines[-1].startswith("DEBUG: cluster_by_rmsd [gfx950, 2 atom permutations] - 11175 pairs screened, ")
        assert f"{len(r0)} clusters" in lines[-1]
    # the default lines keep their wording
    _, mask = fc.pruner.prune_by_rmsd(Y, atoms, THR, debugfunction=lines.append)
    assert np.array_equal(mask, mask_default) and lines[-1].startswith("DEBUG: prune_by_rmsd [gfx950] - ")
    # Ensemble: the RMSD stage alone, then behind the MOI stage (stage by stage: MOI is not symmetry-aware by design)
    log = []
    e = fc.ensemble.Ensemble(atoms, Y.copy(), logfunction=log.append)
    e.similarity_pruning(moi=False, max_rmsd=THR, symmetry=graph)
    assert np.array_equal(e.coords, Y[mask_sym])
    assert any(ln.startswith(f"Discarded {150 - int(mask_sym.sum())} candidates for RMSD similarity (2 atom permutations) "
                             f"({int(mask_sym.sum())} left, ") for ln in log), log
    e2 = fc.ensemble.Ensemble(atoms, Y.copy(), logfunction=None)
    e2.similarity_pruning(max_rmsd=THR, symmetry=table)
    after_moi, m1 = fc.pruner.prune_by_moment_of_inertia(Y, atoms)
    after_both, m2 = fc.pruner.prune_by_rmsd(after_moi, atoms, THR, symmetry=table)
    assert np.array_equal(e2.coords, after_both)
    e3 = fc.ensemble.Ensemble(atoms, Y.copy(), logfunction=log.append)
    cl = e3.cluster_by_rmsd(THR, symmetry=graph)
    assert len(cl.sizes) == len(np.unique(assign)) and len(e3.coords) == 150
    # the default Ensemble path after all that
    e4 = fc.ensemble.Ensemble(atoms, Y.copy(), logfunction=None)
    e4.similarity_pruning(moi=False, max_rmsd=THR)
    assert np.array_equal(e4.coords, Y[mask_default])


def test_hydrogens_and_a_perceived_table(fc):
    """a molecule with hydrogens: the table is perceived over all atoms, the library sees heavy-atom indices"""
    rng = np.random.default_rng(2)
    #  C0H3 - C1(H) (- N3H2) - C2H3: the two methyl carbons are exchanged; 13 atoms, 4 heavy
    atoms = np.array(["C", "C", "C", "N"] + ["H"] * 9)
    edges = [(0, 1), (1, 2), (1, 3), (0, 4), (0, 5), (0, 6), (2, 7), (2, 8), (2, 9), (1, 10), (3, 11), (3, 12)]
    graph = nx.Graph(edges)
    table = fc.symmetry.graph_automorphisms(graph, atoms)
    assert len(table) == 2 and table[1, 0] == 2 and np.array_equal(table[1, 4:], np.arange(4, 13))
    X, _, assign = syn.synthetic_ensemble(60, 13, seed=3)
    Y, _ = sr.relabel_half(X, table, 3)
    sel = sr.selected(table, atoms != "H")
    mats = sr.similarity(Y, atoms, sel, THR)
    assert mats.min_gap > GAP
    ref = o.greedy_prune_from_matrix(mats.S)
    for sym in (graph, table):
        _, mask = fc.pruner.prune_by_rmsd(Y, atoms, THR, symmetry=sym)
        assert np.array_equal(mask, ref)
    _, mask_default = fc.pruner.prune_by_rmsd(Y, atoms, THR)
    assert np.array_equal(mask_default, o.prune_by_rmsd(Y, atoms, THR)[1]) and ref.sum() < mask_default.sum()
