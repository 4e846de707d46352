"""Drop-in for ``prism_pruner.pruner`` (imported at firecode/ensemble.py:31,
embedder.py:45, operators.py:33): similarity pruning on the GPU.

Every function returns ``(structures[mask], mask)`` with ``mask`` a NumPy
bool array in the caller's order, like the reference call sites expect
(ensemble.py:211-235, embedder.py:1452-1496)."""

from collections import namedtuple
from time import perf_counter

import numpy as np

from firecode_amd import _lib as L
from firecode_amd.pt import pt


# The conventions of prism_pruner's pruners that the reference tree does not show (SURVEY.md
# Appendix A: every call site treats the package as a black box), one named switch each, same names
# and defaults as the CONVENTIONS table of the test oracle.  Once `tests/golden/make_golden_prism.py` has been run
# where the package is installed (tests/test_prism_golden.py then says which values reproduce its masks)
# a differing convention is a one-line change here:
#   strict_lt        similar <=> rmsd < thr and maxdev < max_dev (True), or <= (False)
#   maxdev_factor    max_dev = maxdev_factor * max_rmsd when not given (firecode/utils.py:501: 2)
#   drop             "earlier": a structure is removed at the first later similar one; "later": mirror rule
#   default_max_rmsd threshold of a call that passes none (firecode/ensemble.py:230-235)
#   window_strict    pairs are comparable iff |dE| < max_dE (True) or <= (False)
#   moi_tolerance    relative tolerance of prune_by_moment_of_inertia (CHANGELOG.md:256: 1 %)
CONVENTIONS = {"strict_lt": True, "maxdev_factor": 2.0, "drop": "earlier", "default_max_rmsd": 0.25,
               "window_strict": True, "moi_tolerance": 0.01}


def _thresholds(max_rmsd, max_dev, max_dE):
    """The conventions as the kernels see them: `<=` is `<` against the next double up."""
    cv = CONVENTIONS
    max_rmsd = cv["default_max_rmsd"] if max_rmsd is None else float(max_rmsd)
    max_dev = cv["maxdev_factor"] * max_rmsd if max_dev is None else float(max_dev)
    if cv["drop"] not in ("earlier", "later"):
        raise L.FirecodeHipInputError(L.FC_E_INVALID, f"CONVENTIONS['drop'] = {cv['drop']!r}")
    L.call("fc_prune_conventions", int(cv["drop"] == "later"))
    if not cv["strict_lt"]:
        max_rmsd, max_dev = np.nextafter(max_rmsd, np.inf), np.nextafter(max_dev, np.inf)
    if not cv["window_strict"]:
        max_dE = np.nextafter(float(max_dE), np.inf)
    return float(max_rmsd), float(max_dev), float(max_dE)


def _sorted_by_energy(structures, energies):
    """The reference processes structures in ascending-energy order when
    energies are given; same ``np.argsort`` call."""
    if energies is None:
        return None, None
    energies = np.asarray(energies, dtype=np.float64)
    if energies.shape[0] != structures.shape[0] or structures.shape[0] == 0:
        return None, None
    # stable: a later stage that sorts the SURVIVORS of an earlier one then processes them in the order
    # the earlier stage left them in -- what makes the fused pipeline equal to the stage-by-stage calls
    order = np.argsort(energies, kind="stable")
    return order, np.ascontiguousarray(energies[order])


def _unsort(mask_sorted, order):
    if order is None:
        return mask_sorted
    mask = np.empty_like(mask_sorted)
    mask[order] = mask_sorted
    return mask


def _structures_and_atoms(structures, atoms):
    """the two array arguments of every driver, checked against each other"""
    structures = L.f64(structures)
    if structures.ndim != 3 or structures.shape[2] != 3:
        raise L.FirecodeHipInputError(L.FC_E_INVALID, f"structures must be (N, A, 3), got {structures.shape}")
    atoms = np.asarray(atoms)
    if atoms.shape[0] != structures.shape[1]:
        raise L.FirecodeHipInputError(L.FC_E_INVALID, "len(atoms) != number of atoms")
    return structures, atoms


def _graph_inputs(structures, atoms, max_rmsd, max_dev, energies, max_dE, heavy_atoms_only, enant, symmetry):
    """What ``cluster_by_rmsd`` and ``dbscan_by_rmsd`` do in front of the device, in the order in which a bad argument
    is reported: shapes, the symmetry table, the thresholds; then (not for an empty ensemble, whose caller returns at once)
    the atom selection and the ascending-energy order
    -> (structures, table, (max_rmsd, max_dev, max_dE), heavy, order, en_sorted, X = the structures in that order)"""
    from firecode_amd import symmetry as S

    structures, atoms = _structures_and_atoms(structures, atoms)
    table = S.resolve(symmetry, atoms, heavy_atoms_only)
    S.refuse_with_enantiomers(table, enant)
    if table is not None:
        S.selected_table(table, (atoms != "H") if heavy_atoms_only else None)
    thresholds = _thresholds(max_rmsd, max_dev, max_dE)
    if structures.shape[0] == 0:
        return structures, table, thresholds, None, None, None, None
    heavy = (atoms != "H") if heavy_atoms_only else np.ones(len(atoms), dtype=bool)
    order, en_sorted = _sorted_by_energy(structures, energies)
    X = structures if order is None else np.ascontiguousarray(structures[order])
    return structures, table, thresholds, heavy, order, en_sorted, X


def prune_by_rmsd(structures, atoms, max_rmsd=None, max_dev=None, energies=None, max_dE=0.0,
                  debugfunction=None, heavy_atoms_only=True, min_per_group=20, prune_enantiomers=False, symmetry=None):
    """Heavy-atom Kabsch-RMSD pruning: a pair is similar when
    ``rmsd < max_rmsd and maxdev < max_dev`` (default ``2*max_rmsd``; ``max_rmsd`` defaults to
    ``CONVENTIONS["default_max_rmsd"]``, the case of firecode/ensemble.py:230 which passes none).

    ``prune_enantiomers=True``: mirror images count as duplicates -- a pair is also similar when it passes the same
    two tests with one partner inverted through its centroid (fc_prune_rmsd_enant; the contract is written out in
    include/fc_hip.h).  Upstream's ``prune_enantiomers`` / ``ENANTIOMERS`` option, removed there for speed.

    ``symmetry=``: copies of one conformation with equivalent atoms relabelled count as duplicates -- a pair is also
    similar when it passes the two tests under any of K atom permutations (fc_prune_rmsd_perm; the contract is written
    out in include/fc_hip.h).  A networkx bond graph (its automorphisms are perceived,
    ``firecode_amd.symmetry.graph_automorphisms``) or an explicit (K, A) table over all atoms; ``None``: the path as
    it is.  Not combinable with ``prune_enantiomers``."""
    from firecode_amd import symmetry as S

    t0 = perf_counter()
    enant = L.check_flag("prune_enantiomers", prune_enantiomers)
    structures, atoms = _structures_and_atoms(structures, atoms)
    heavy = (atoms != "H") if heavy_atoms_only else np.ones(len(atoms), dtype=bool)
    table = S.resolve(symmetry, atoms, heavy_atoms_only)
    S.refuse_with_enantiomers(table, enant)
    if table is not None:
        S.selected_table(table, heavy)  # (its checks, before any device use)
    max_rmsd, max_dev, max_dE = _thresholds(max_rmsd, max_dev, max_dE)
    N = structures.shape[0]
    if N == 0:
        return structures, np.ones(0, dtype=bool)
    order, en_sorted = _sorted_by_energy(structures, energies)
    X = structures if order is None else np.ascontiguousarray(structures[order])
    if table is not None:  # the resident form, as below
        with L.DeviceEnsemble(X, atom_mask=heavy, center=True) as ens:
            m_sorted, stats = ens.prune(max_rmsd, max_dev, energies=en_sorted, max_dE=max_dE, min_per_group=min_per_group,
                                        symmetry=table)
    elif enant:  # the resident form: the one-call host path stays the default's
        with L.DeviceEnsemble(X, atom_mask=heavy, center=True) as ens:
            m_sorted, stats = ens.prune(max_rmsd, max_dev, energies=en_sorted, max_dE=max_dE, min_per_group=min_per_group,
                                        prune_enantiomers=True)
    else:
        # one C call (fc_prune_rmsd_host): upload, preparation, prune, mask
        m8 = np.zeros(N, dtype=np.uint8)
        stats = np.zeros(6, dtype=np.int64)
        hm = np.ascontiguousarray(heavy, dtype=np.uint8)
        L.call("fc_prune_rmsd_host", L.pf(X), N, X.shape[1], L.pb(hm), 1, float(max_rmsd), float(max_dev),
               L.pf(None if en_sorted is None else L.f64(en_sorted)), float(max_dE), int(min_per_group), L.pb(m8), L.pi(stats))
        m_sorted = m8.view(np.bool_)
    mask = _unsort(m_sorted, order)
    if debugfunction is not None:
        debugfunction(
            f"DEBUG: prune_by_rmsd [gfx950{', mirror images included' if enant else ''}"
            f"{'' if table is None else f', {len(table)} atom permutations'}] - {stats[0]} pairs screened, {stats[1]} refined, "
            f"{stats[2]} similar, {stats[3]} grey, {stats[4]} ladder levels, "
            f"keeping {int(mask.sum())}/{N} in {perf_counter() - t0:.3f} s")
    return structures[mask], mask


DiverseSelection = namedtuple("DiverseSelection", ["indices", "labels", "distances", "radii"])


def select_diverse(structures, atoms, n=None, stop_rmsd=None, heavy_atoms_only=True, start=None, energies=None,
                   symmetry=None, prune_enantiomers=False):
    """RMSD-diverse selection: greedy max-min (farthest point, Gonzalez k-center) under the heavy-atom Kabsch RMSD
    ``prune_by_rmsd`` uses (centred, ``rmsd_and_max(...)[0]``), on the GPU (fc_ensemble_select_diverse; the contract
    is written out in include/fc_hip.h).  Either "the ``n`` most different conformers" (``n``) or "representatives
    such that every conformer is within ``stop_rmsd`` of one" (``stop_rmsd``; with both, whichever comes first;
    with only ``stop_rmsd``, ``n`` = N).  The first representative is ``start``, else the lowest energy of
    ``energies`` (lowest index on ties), else 0.  No N x N matrix: one conformer is aligned against all N per step.

    Returns ``DiverseSelection(indices, labels, distances, radii)``: indices (K,) into ``structures`` in selection
    order; labels (N,) int32, the position in ``indices`` of each conformer's nearest representative; distances (N,)
    to it; radii (K,) the covering radius just before each pick (nonincreasing, radii[0] = inf).

    ``symmetry=`` (a bond graph or a (K, A) table over all atoms, as in ``prune_by_rmsd``) and ``prune_enantiomers=True``
    -- here the two combine -- make the distance the smallest RMSD over the atom permutations and, with the flag, over
    both handednesses (fc_ensemble_select_diverse_perm): a relabelled copy or a mirror image of a representative is at
    distance 0 from it and is not picked as "most different"."""
    from firecode_amd import symmetry as S

    enant = L.check_flag("prune_enantiomers", prune_enantiomers)
    structures, atoms = _structures_and_atoms(structures, atoms)
    N = structures.shape[0]
    if n is None and stop_rmsd is None:
        raise L.FirecodeHipInputError(L.FC_E_INVALID, "select_diverse needs n, stop_rmsd or both")
    if n is not None and (int(n) != n or int(n) < 1):
        raise L.FirecodeHipInputError(L.FC_E_INVALID, f"n={n!r}: at least one representative")
    if stop_rmsd is not None and not float(stop_rmsd) >= 0.0:
        raise L.FirecodeHipInputError(L.FC_E_INVALID, f"stop_rmsd={stop_rmsd!r} must be >= 0")
    if energies is not None:
        energies = np.asarray(energies, dtype=np.float64).reshape(-1)
        if energies.shape[0] != N:
            raise L.FirecodeHipInputError(L.FC_E_INVALID, "len(energies) != number of structures")
    if start is not None and not 0 <= int(start) < max(N, 1):
        raise L.FirecodeHipInputError(L.FC_E_INVALID, f"start={start!r} outside [0, {N})")
    heavy = (atoms != "H") if heavy_atoms_only else np.ones(len(atoms), dtype=bool)
    if not heavy.any():
        raise L.FirecodeHipInputError(L.FC_E_INVALID, "the atom selection is empty (no heavy atom)")
    table = S.resolve(symmetry, atoms, heavy_atoms_only)
    S.diverse_table(table, enant, heavy, len(atoms))  # (its checks, before any device use)
    if N == 0:
        empty = np.zeros(0, dtype=np.int64)
        return DiverseSelection(empty, np.zeros(0, dtype=np.int32), np.zeros(0), np.zeros(0))
    if start is None:
        start = int(np.argmin(energies)) if energies is not None else 0  # (argmin: the first of equal minima)
    n_max = N if n is None else int(n)
    with L.DeviceEnsemble(structures, atom_mask=heavy, center=True) as ens:
        return DiverseSelection(*ens.select_diverse(n_max, start=int(start), stop_rmsd=stop_rmsd, symmetry=table,
                                                    prune_enantiomers=enant))


class RmsdNeighbours(namedtuple("RmsdNeighbours", ["indices", "distances"])):
    """The lists of ``knn_by_rmsd``: indices (N, k) int32 and distances (N, k) float64, each row in ascending order of
    (distance, index); slots beyond N - 1 neighbours hold -1 / +inf.  The two methods are host-side NumPy."""

    __slots__ = ()

    def k_distances(self, k=None):
        """The distance of every conformer to its ``k``-th neighbour (column ``k - 1``; default: the last), sorted in
        descending order: the "k-distance" curve whose knee is the DBSCAN radius for ``min_samples = k + 1``."""
        dist = np.asarray(self.distances)
        width = dist.shape[1]
        if k is None:
            k = width
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= width:
            raise L.FirecodeHipInputError(L.FC_E_INVALID, f"k={k!r}: an integer in [1, {width}], the lists' length")
        return np.sort(dist[:, int(k) - 1])[::-1].copy()

    def pairs(self, mutual=False):
        """The neighbour graph as an undirected edge list (M, 2) int64 with ``i < j``, unique, sorted -- what
        ``clusters_from_pairs`` / ``dbscan_from_pairs`` take: {i, j} is an edge when j is in i's list or i in j's;
        ``mutual=True``: only when both hold.  Entries with index -1 are dropped."""
        mutual = L.check_flag("mutual", mutual)
        idx = np.asarray(self.indices).astype(np.int64)
        n = idx.shape[0]
        i = np.repeat(np.arange(n, dtype=np.int64), idx.shape[1])
        j = idx.reshape(-1)
        keep = j >= 0
        i, j = i[keep], j[keep]
        # (a row never names itself and names a conformer at most once: a word occurs once per direction)
        words, counts = np.unique(np.minimum(i, j) * np.int64(n) + np.maximum(i, j), return_counts=True)
        if mutual:
            words = words[counts == 2]
        return np.stack([words // max(n, 1), words % max(n, 1)], axis=1).astype(np.int64).reshape(-1, 2)


def _knn_symmetry(symmetry, prune_enantiomers, atoms, heavy, heavy_atoms_only):
    """``symmetry=`` (a bond graph or a table) and ``prune_enantiomers=`` of the nearest-neighbour drivers -> (the checked
    table over all atoms or None, the flag); every check, the LDS limit included, made before any device use"""
    from firecode_amd import symmetry as S

    enant = L.check_flag("prune_enantiomers", prune_enantiomers)
    table = S.resolve(symmetry, atoms, heavy_atoms_only)
    S.knn_table(table, enant, heavy, len(atoms))
    return table, enant


def knn_by_rmsd(structures, atoms, k, heavy_atoms_only=True, symmetry=None, prune_enantiomers=False):
    """The ``k`` nearest neighbours of every conformer under the heavy-atom Kabsch RMSD ``prune_by_rmsd`` uses (centred,
    ``rmsd_and_max(...)[0]``), on the GPU (fc_ensemble_knn; the contract is written out in include/fc_hip.h), with no
    N x N matrix: the top-k selection happens in the kernel that computes the distances.  1 <= k <= 64.

    Returns ``RmsdNeighbours(indices, distances)``: (N, k) int32 and (N, k) float64, each row in ascending order of
    (distance, index) -- on equal distances the lower index first -- the conformer itself left out by index (an exact
    duplicate of it is its first neighbour, at distance ~1e-15); when ``k > N - 1`` the rows end in -1 / +inf.
    ``.k_distances(min_samples - 1)`` is the curve one reads the ``max_rmsd`` of ``dbscan_by_rmsd`` from;
    ``.pairs()`` / ``.pairs(mutual=True)`` is the (mutual) k-NN graph in the format of ``clusters_from_pairs``.

    ``symmetry=`` (a bond graph or a (K, A) table over all atoms, as in ``prune_by_rmsd``) and ``prune_enantiomers=True``
    -- the two combine, as in ``select_diverse`` -- make the distance the smallest RMSD over the atom permutations and,
    with the flag, over both handednesses (fc_ensemble_knn_perm): a relabelled copy or a mirror image of a conformer is
    its first neighbour, at distance 0, instead of sitting far away."""
    structures, atoms = _structures_and_atoms(structures, atoms)
    k = L.check_knn_k(k)
    heavy = (atoms != "H") if heavy_atoms_only else np.ones(len(atoms), dtype=bool)
    if not heavy.any():
        raise L.FirecodeHipInputError(L.FC_E_INVALID, "the atom selection is empty (no heavy atom)")
    table, enant = _knn_symmetry(symmetry, prune_enantiomers, atoms, heavy, heavy_atoms_only)
    if structures.shape[0] == 0:
        return RmsdNeighbours(np.zeros((0, k), dtype=np.int32), np.zeros((0, k)))
    with L.DeviceEnsemble(structures, atom_mask=heavy, center=True) as ens:
        return RmsdNeighbours(*ens.knn(k, symmetry=table, prune_enantiomers=enant))


class RmsdCrossNeighbours(namedtuple("RmsdCrossNeighbours", ["indices", "distances"])):
    """The lists of ``knn_by_rmsd_against``: indices (Nq, k) int32 into the REFERENCE set and distances (Nq, k) float64,
    each row in ascending order of (distance, index); slots for which no reference qualifies hold -1 / +inf.  Rows and
    entries belong to different sets, so this is not an ``RmsdNeighbours`` (no graph, no k-distance curve).  The two
    methods are host-side NumPy."""

    __slots__ = ()

    def nearest(self):
        """``(indices[:, 0], distances[:, 0])``: every query's closest listed reference (-1 / +inf where none)"""
        return np.asarray(self.indices)[:, 0], np.asarray(self.distances)[:, 0]

    def novel(self, max_rmsd):
        """(Nq,) bool: true where NO listed reference has ``d < max_rmsd`` (strict, like the prune's ``rmsd < max_rmsd``).
        Lists made with a cap answer for radii up to that cap only.  RMSD alone: no max-deviation or energy test."""
        max_rmsd = L.check_max_rmsd_cap(max_rmsd)
        return ~(np.asarray(self.distances) < max_rmsd).any(axis=1)


def _cross_inputs(structures, references, atoms):
    """the three array arguments of the cross-ensemble drivers, checked against one another"""
    structures, atoms = _structures_and_atoms(structures, atoms)
    references = L.f64(references)
    if references.ndim != 3 or references.shape[1:] != structures.shape[1:]:
        raise L.FirecodeHipInputError(
            L.FC_E_INVALID, f"references must be (N, {structures.shape[1]}, 3) like structures, got {references.shape}")
    return structures, references, atoms


def knn_by_rmsd_against(structures, references, atoms, k, max_rmsd=None, heavy_atoms_only=True, symmetry=None,
                        prune_enantiomers=False):
    """For every conformer of ``structures`` its ``k`` nearest conformers of ``references`` -- a second set of
    conformers of the same molecule, same ``atoms`` -- under the heavy-atom Kabsch RMSD ``prune_by_rmsd`` uses (centred,
    ``rmsd_and_max(...)[0]``), on the GPU (fc_ensemble_knn_cross; the contract is written out in include/fc_hip.h): the
    kernel of ``knn_by_rmsd`` with its rows from one resident ensemble and its columns from another, no matrix of the
    union on the host.  1 <= k <= 64.  ``max_rmsd``: only references with ``d < max_rmsd`` are listed.

    Returns ``RmsdCrossNeighbours(indices, distances)``: (Nq, k) int32 indices into ``references`` and (Nq, k) float64,
    each row in ascending order of (distance, index) -- on equal distances the lower index first.  Nothing is left out:
    a query that is a copy of a reference lists it first, at ~1e-15.  Rows with fewer than ``k`` qualifying references
    (``k > len(references)``, or the cap) end in -1 / +inf.  ``.nearest()`` is column 0; ``.novel(r)`` the queries with
    no listed reference within ``r``.  RMSD only: the max-deviation and energy-window tests of the prune play no part.

    ``symmetry=`` / ``prune_enantiomers=True``: as in ``knn_by_rmsd`` (fc_ensemble_knn_cross_perm); the one table serves
    both sets, which are conformers of the same molecule."""
    structures, references, atoms = _cross_inputs(structures, references, atoms)
    k = L.check_knn_k(k)
    cap = None if max_rmsd is None else L.check_max_rmsd_cap(max_rmsd)
    heavy = (atoms != "H") if heavy_atoms_only else np.ones(len(atoms), dtype=bool)
    if not heavy.any():
        raise L.FirecodeHipInputError(L.FC_E_INVALID, "the atom selection is empty (no heavy atom)")
    table, enant = _knn_symmetry(symmetry, prune_enantiomers, atoms, heavy, heavy_atoms_only)
    Nq, Nr = structures.shape[0], references.shape[0]
    if Nq == 0 or Nr == 0:  # nothing to list, or nothing to list from: no device needed
        return RmsdCrossNeighbours(np.full((Nq, k), -1, dtype=np.int32), np.full((Nq, k), np.inf))
    with L.DeviceEnsemble(structures, atom_mask=heavy, center=True) as q, \
            L.DeviceEnsemble(references, atom_mask=heavy, center=True) as r:
        return RmsdCrossNeighbours(*q.knn_against(r, k, max_rmsd=cap, symmetry=table, prune_enantiomers=enant))


def novel_conformers(structures, references, atoms, max_rmsd, heavy_atoms_only=True, symmetry=None, prune_enantiomers=False):
    """Which conformers of ``structures`` are new against ``references``: (Nq,) bool, true where NO reference is within
    ``max_rmsd`` of the conformer (``rmsd < max_rmsd``, the RMSD test of ``prune_by_rmsd``).  One call of
    ``knn_by_rmsd_against`` with ``k = 1`` and the cap, which lets the kernel's filter rule out whole blocks of
    references from the start.  RMSD only: the max-deviation and energy-window tests of the prune are not applied, so
    this is not "would ``prune_by_rmsd`` of the union drop it".  ``symmetry=`` / ``prune_enantiomers=True``: as in
    ``knn_by_rmsd`` -- a relabelled copy or a mirror image of a reference is not new."""
    if max_rmsd is None:
        raise L.FirecodeHipInputError(L.FC_E_INVALID, "novel_conformers needs max_rmsd")
    nb = knn_by_rmsd_against(structures, references, atoms, 1, max_rmsd=max_rmsd, heavy_atoms_only=heavy_atoms_only,
                             symmetry=symmetry, prune_enantiomers=prune_enantiomers)
    return nb.indices[:, 0] < 0


class EnsembleCoverage(namedtuple("EnsembleCoverage", ["covered", "fraction", "nearest", "distances"])):
    """The answer of ``ensemble_coverage``: covered (Nr,) bool, fraction = covered.mean() (nan for an empty reference
    set), nearest (Nr,) int32 = the closest conformer of ``structures`` to each reference (-1 where there is none),
    distances (Nr,) to it (+inf where there is none)."""

    __slots__ = ()

    @classmethod
    def from_neighbours(cls, nb, max_rmsd):
        """from the lists of the references against the structures (``k >= 1``, no cap below ``max_rmsd``)"""
        max_rmsd = L.check_max_rmsd_cap(max_rmsd)
        nearest, dist = nb.nearest()
        covered = dist < max_rmsd
        return cls(covered, float(covered.mean()) if len(covered) else float("nan"), nearest, dist)

    def mean_distance(self):
        """The mean of the finite nearest distances -- the MAT figure quoted beside the coverage; nan when no distance is
        finite (no reference, or no structure)."""
        dist = np.asarray(self.distances, dtype=np.float64)
        finite = dist[np.isfinite(dist)]
        return float(finite.mean()) if finite.size else float("nan")


def ensemble_coverage(structures, references, atoms, max_rmsd, heavy_atoms_only=True, symmetry=None, prune_enantiomers=False):
    """Does ``structures`` contain every conformer of ``references`` to within ``max_rmsd`` -- the coverage (recall)
    figure of conformer-generator benchmarks: for every reference, is there a conformer of ``structures`` with
    ``rmsd < max_rmsd``?  ``knn_by_rmsd_against`` with the roles swapped (the references are the rows), ``k = 1`` and no
    cap, so that the distance to the closest conformer is reported for the uncovered references too.

    Returns ``EnsembleCoverage(covered, fraction, nearest, distances)``; its ``.mean_distance()`` is the companion
    figure (MAT).  RMSD only, as ``novel_conformers``.  ``symmetry=`` / ``prune_enantiomers=True``: as in
    ``knn_by_rmsd`` -- the symmetry-corrected RMSD on which the benchmarks define the two figures."""
    if max_rmsd is None:
        raise L.FirecodeHipInputError(L.FC_E_INVALID, "ensemble_coverage needs max_rmsd")
    max_rmsd = L.check_max_rmsd_cap(max_rmsd)
    nb = knn_by_rmsd_against(references, structures, atoms, 1, heavy_atoms_only=heavy_atoms_only, symmetry=symmetry,
                             prune_enantiomers=prune_enantiomers)
    return EnsembleCoverage.from_neighbours(nb, max_rmsd)


RmsdMedoids = namedtuple("RmsdMedoids", ["medoids", "sizes", "mean_distance", "radius", "sums", "eccentricity"])
RmsdKMedoids = namedtuple("RmsdKMedoids", ["medoids", "labels", "distances", "cost", "n_iter"])

Q32 = 2.0 ** -32  # the unit of the integer sums of the medoid calls (include/fc_hip.h: q(d) = rint(d * 2^32))


def _medoid_inputs(structures, atoms, heavy_atoms_only):
    structures, atoms = _structures_and_atoms(structures, atoms)
    heavy = (atoms != "H") if heavy_atoms_only else np.ones(len(atoms), dtype=bool)
    if not heavy.any():
        raise L.FirecodeHipInputError(L.FC_E_INVALID, "the atom selection is empty (no heavy atom)")
    return structures, heavy


def medoids_by_rmsd(structures, atoms, labels=None, heavy_atoms_only=True):
    """Which conformer stands for each group: the medoid, the member with the smallest summed heavy-atom Kabsch RMSD
    (the RMSD of ``prune_by_rmsd``: centred, ``rmsd_and_max(...)[0]``) to the other members of its group, the lowest
    index on ties -- on the GPU, without an N x N matrix (fc_ensemble_medoids; the contract is written out in
    include/fc_hip.h).  ``labels``: one integer per conformer, a negative one = in no group -- the ``labels`` of
    ``RmsdClusters``, ``RmsdDbscan`` (-1 is noise) and ``RmsdButina`` as they come; ``None``: the whole ensemble is one
    group.

    Returns ``RmsdMedoids(medoids, sizes, mean_distance, radius, sums, eccentricity)``: per group (largest label + 1 of
    them) the medoid's index, the member count, the medoid's mean distance to the other members (0 for a singleton) and
    its largest (the group's radius around it); per conformer the summed distance to the other members of its group
    in A (float64; exact multiples of 2^-32: the sums are made in integers and are the same bits on every run) and
    the largest such distance.  An empty group id has medoid -1, size 0 and NaN mean and radius."""
    structures, heavy = _medoid_inputs(structures, atoms, heavy_atoms_only)
    N = structures.shape[0]
    lab, n_groups = L.check_group_labels(labels, N)
    if N == 0:
        nan = np.full(n_groups, np.nan)
        return RmsdMedoids(np.full(n_groups, -1, dtype=np.int64), np.zeros(n_groups, dtype=np.int64), nan, nan.copy(),
                           np.zeros(0), np.zeros(0))
    with L.DeviceEnsemble(structures, atom_mask=heavy, center=True) as ens:
        med, sizes, mean, radius, sums, ecc = ens.medoids(lab, n_groups)
    return RmsdMedoids(med, sizes, mean, radius, sums.astype(np.float64) * Q32, ecc)


def kmedoids_by_rmsd(structures, atoms, n, init=None, max_iter=50, heavy_atoms_only=True):
    """``n`` representative conformers: k-medoids under the heavy-atom Kabsch RMSD of ``prune_by_rmsd`` -- the ``n``
    conformers that (locally) minimise the mean distance of every conformer to its representative -- on the GPU
    (fc_ensemble_kmedoids; the contract is written out in include/fc_hip.h): starting from ``init`` (``n`` distinct
    indices; default: the ``n`` picks of ``select_diverse(..., n=n, start=0)``, the extremes of the ensemble), assign
    every conformer to its nearest representative and move each representative to the medoid of its group, until the
    cost stops falling or ``max_iter`` moves have been made.  ``select_diverse`` answers "the n most different",
    this "the n most typical".

    Returns ``RmsdKMedoids(medoids, labels, distances, cost, n_iter)``: medoids (n,) int64; labels (N,) int32, the
    position in ``medoids`` of each conformer's representative; distances (N,) to it (0 for a representative); cost in
    A, the sum of the distances rounded to 2^-32 A each (the same bits on every run); n_iter, the assignments made."""
    structures, heavy = _medoid_inputs(structures, atoms, heavy_atoms_only)
    N = structures.shape[0]
    n = L.check_count("n", n)
    max_iter = L.check_count("max_iter", max_iter, low=0)
    if N == 0:
        return RmsdKMedoids(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), 0.0, 0)
    if n > N:
        raise L.FirecodeHipInputError(L.FC_E_INVALID, f"n={n} representatives of N={N} conformers")
    start = None if init is None else L.check_indices("init", init, N, distinct=True, count=n)
    with L.DeviceEnsemble(structures, atom_mask=heavy, center=True) as ens:
        med, lab, dist, cost, n_iter = ens.kmedoids(n, init=start, max_iter=max_iter)
    return RmsdKMedoids(med, lab, dist, cost * Q32, n_iter)


def _sums_symmetry(symmetry, prune_enantiomers, atoms, heavy, heavy_atoms_only):
    """``symmetry=`` (a bond graph or a table) and ``prune_enantiomers=`` of the ``*_sym`` medoid and silhouette drivers
    -> (the checked table over all atoms or None, the flag), resolved as ``_knn_symmetry`` does; every check, the LDS
    limit included, made before any device use"""
    from firecode_amd import symmetry as S

    enant = L.check_flag("prune_enantiomers", prune_enantiomers)
    table = S.resolve(symmetry, atoms, heavy_atoms_only)
    if table is not None or enant:
        t = S.selected_table(np.arange(len(atoms), dtype=np.int64)[None] if table is None else table, heavy)
        S.medoid_lds_check(t.shape[0], t.shape[1])
    return table, enant


def medoids_by_rmsd_sym(structures, atoms, labels=None, heavy_atoms_only=True, symmetry=None, prune_enantiomers=False):
    """``medoids_by_rmsd`` under the symmetry-corrected distance the clusterers group by (fc_ensemble_medoids_perm; the
    contract is written out in include/fc_hip.h).  ``symmetry=`` (a bond graph or a (K, A) table over all atoms, as in
    ``prune_by_rmsd``) and ``prune_enantiomers=True`` -- the two combine, as in ``knn_by_rmsd`` -- make the distance the
    smallest RMSD over the atom permutations and, with the flag, over both handednesses: a phenyl flip or a mirror
    image of a member is at distance 0 from it and no longer decides which member is the medoid.  With neither
    keyword this is ``medoids_by_rmsd``.  A name of its own because ``medoids_by_rmsd`` refuses the two keywords.
    Returns ``RmsdMedoids``."""
    structures, heavy = _medoid_inputs(structures, atoms, heavy_atoms_only)
    atoms = np.asarray(atoms)
    table, enant = _sums_symmetry(symmetry, prune_enantiomers, atoms, heavy, heavy_atoms_only)
    N = structures.shape[0]
    lab, n_groups = L.check_group_labels(labels, N)
    if N == 0:
        nan = np.full(n_groups, np.nan)
        return RmsdMedoids(np.full(n_groups, -1, dtype=np.int64), np.zeros(n_groups, dtype=np.int64), nan, nan.copy(),
                           np.zeros(0), np.zeros(0))
    with L.DeviceEnsemble(structures, atom_mask=heavy, center=True) as ens:
        med, sizes, mean, radius, sums, ecc = ens.medoids_sym(lab, n_groups, symmetry=table, prune_enantiomers=enant)
    return RmsdMedoids(med, sizes, mean, radius, sums.astype(np.float64) * Q32, ecc)


def kmedoids_by_rmsd_sym(structures, atoms, n, init=None, max_iter=50, heavy_atoms_only=True, symmetry=None,
                         prune_enantiomers=False):
    """``kmedoids_by_rmsd`` under the symmetry-corrected distance of ``medoids_by_rmsd_sym``
    (fc_ensemble_kmedoids_perm): the default start is the symmetry-aware ``select_diverse``, every conformer goes to
    its nearest representative under that distance and every representative moves to the medoid under it.  With
    neither keyword this is ``kmedoids_by_rmsd``.  Returns ``RmsdKMedoids``."""
    structures, heavy = _medoid_inputs(structures, atoms, heavy_atoms_only)
    atoms = np.asarray(atoms)
    table, enant = _sums_symmetry(symmetry, prune_enantiomers, atoms, heavy, heavy_atoms_only)
    N = structures.shape[0]
    n = L.check_count("n", n)
    max_iter = L.check_count("max_iter", max_iter, low=0)
    if N == 0:
        return RmsdKMedoids(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), 0.0, 0)
    if n > N:
        raise L.FirecodeHipInputError(L.FC_E_INVALID, f"n={n} representatives of N={N} conformers")
    start = None if init is None else L.check_indices("init", init, N, distinct=True, count=n)
    with L.DeviceEnsemble(structures, atom_mask=heavy, center=True) as ens:
        med, lab, dist, cost, n_iter = ens.kmedoids_sym(n, init=start, max_iter=max_iter, symmetry=table, prune_enantiomers=enant)
    return RmsdKMedoids(med, lab, dist, cost * Q32, n_iter)


RmsdGroupMeans = namedtuple("RmsdGroupMeans", ["means", "rmsf", "distances", "closest", "sizes", "n_iter", "rotations", "aligned"])


def group_means_by_rmsd(structures, atoms, labels=None, refs=None, max_iter=50, tol=1e-9, heavy_atoms_only=True,
                        aligned=False):
    """What each group looks like: its mean structure with the members superposed on it (generalized Procrustes per
    group, under the heavy-atom Kabsch fit of ``prune_by_rmsd``), the per-atom fluctuation about that mean (RMSF), every
    member's RMSD to it and the member closest to it -- on the GPU (fc_ensemble_group_means; the contract, the order of
    its sums included, is written out in include/fc_hip.h).  ``labels`` as for ``medoids_by_rmsd`` (negative: in no
    group; ``None``: one group).  ``refs``: the member each group's iteration starts from -- one index per group,
    ``None`` (the lowest-index member) or ``"medoids"`` (the medoids, found on the same upload).  A group turns until
    its mean moves by no more than ``tol`` A (RMS over the selected atoms), ``max_iter`` turns at most; ``max_iter=0``
    leaves the reference member as the mean.

    Returns ``RmsdGroupMeans(means, rmsf, distances, closest, sizes, n_iter, rotations, aligned)``: per group (largest
    label + 1 of them) the mean (A_sel, 3) of the centred selected atoms, rmsf (A_sel,), the index of the closest
    member, the member count and the turns taken; per conformer the RMSD to its group's mean and the rotation (3, 3)
    that superposes it.  With ``aligned=True``, ``aligned`` is the whole (N, A, 3) block, hydrogens included, every
    conformer moved rigidly by its rotation about the centroid of its selected atoms -- the members of a group lie
    superposed on their mean, ready to write out; otherwise ``None``.  An empty group id has NaN mean and rmsf, size 0
    and closest -1; a conformer in no group NaN distance, the identity, and comes back centred and unrotated."""
    structures, heavy = _medoid_inputs(structures, atoms, heavy_atoms_only)
    N = structures.shape[0]
    lab, n_groups = L.check_group_labels(labels, N)
    max_iter = L.check_count("max_iter", max_iter, low=0)
    tol = L.check_tol("tol", tol)
    want_aligned = L.check_flag("aligned", aligned)
    if isinstance(refs, str):
        if refs != "medoids":
            raise L.FirecodeHipInputError(L.FC_E_INVALID, f"refs={refs!r}: an array, None or 'medoids'")
    elif refs is not None:
        refs = L.check_group_refs(refs, lab, n_groups, N)
    if N == 0:
        a_sel = int(np.count_nonzero(heavy))
        return RmsdGroupMeans(np.full((n_groups, a_sel, 3), np.nan), np.full((n_groups, a_sel), np.nan), np.zeros(0),
                              np.full(n_groups, -1, dtype=np.int64), np.zeros(n_groups, dtype=np.int64),
                              np.zeros(n_groups, dtype=np.int64), np.zeros((0, 3, 3)),
                              structures.copy() if want_aligned else None)
    with L.DeviceEnsemble(structures, atom_mask=heavy, center=True) as ens:
        means, rmsf, dist, closest, sizes, n_iter, rot = ens.group_means(lab, n_groups, refs=refs, max_iter=max_iter, tol=tol)
    block = None
    if want_aligned:
        from firecode_amd.embeds import rototranslate

        # R (x - c) = R x + (-R c), c the centroid of the selected atoms: one launch of the rototranslate kernel
        c = structures[:, heavy].mean(axis=1)
        block = rototranslate(structures, rot, -np.einsum("nij,nj->ni", rot, c))
    return RmsdGroupMeans(means, rmsf, dist, closest, sizes, n_iter, rot, block)


RmsdClusters = namedtuple("RmsdClusters", ["labels", "representatives", "sizes"])


def cluster_by_rmsd(structures, atoms, max_rmsd=None, max_dev=None, energies=None, max_dE=0.0, debugfunction=None,
                    heavy_atoms_only=True, prune_enantiomers=False, symmetry=None):
    """Which conformers belong together: the connected components of the similarity graph ``prune_by_rmsd`` prunes
    (an edge where ``rmsd < max_rmsd and maxdev < max_dev`` [and ``|dE| < max_dE``]; with ``prune_enantiomers=True``
    also where that holds for the mirror image; with ``symmetry=``, as in ``prune_by_rmsd``, also where it holds under
    one of the atom permutations: fc_rmsd_clusters_perm), on the GPU (fc_rmsd_clusters; the contract is written out in
    include/fc_hip.h).  Unlike the greedy mask the answer does not depend on the order of the conformers, on
    ``min_per_group`` or on ``CONVENTIONS["drop"]``.

    Returns ``RmsdClusters(labels, representatives, sizes)``: labels (N,) int32 in the caller's order; representatives
    (K,) int64 indices into ``structures``; sizes (K,) int64.  A cluster's representative is its first member in
    processing order -- lowest energy (earliest on ties) when ``energies`` is usable, lowest index otherwise -- and
    clusters are numbered in the order of their representatives."""
    t0 = perf_counter()
    enant = L.check_flag("prune_enantiomers", prune_enantiomers)
    structures, table, (max_rmsd, max_dev, max_dE), heavy, order, en_sorted, X = _graph_inputs(
        structures, atoms, max_rmsd, max_dev, energies, max_dE, heavy_atoms_only, enant, symmetry)
    N = structures.shape[0]
    if N == 0:
        return RmsdClusters(np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    with L.DeviceEnsemble(X, atom_mask=heavy, center=True) as ens:
        labels_sorted, reps_sorted, sizes, stats = ens.clusters(max_rmsd, max_dev, energies=en_sorted, max_dE=max_dE,
                                                                prune_enantiomers=enant, symmetry=table)
    if order is None:
        labels, reps = labels_sorted, reps_sorted
    else:
        labels = np.empty_like(labels_sorted)
        labels[order] = labels_sorted
        reps = order[reps_sorted].astype(np.int64)
    if debugfunction is not None:
        debugfunction(
            f"DEBUG: cluster_by_rmsd [gfx950{', mirror images included' if enant else ''}"
            f"{'' if table is None else f', {len(table)} atom permutations'}] - {stats[0]} pairs screened, "
            f"{stats[2]} similar, {len(sizes)} clusters, largest {int(sizes.max())}, in {perf_counter() - t0:.3f} s")
    return RmsdClusters(labels, reps, sizes)


def _labels_from_graph(name, graph, n, min_samples=None):
    """the C entry point ``name`` on a checked pair list or bit matrix; ``min_samples``: the density-based forms'"""
    import ctypes as C

    dbscan, butina = min_samples is not None, name.startswith("fc_butina_")
    labels = np.zeros(n, dtype=np.int32)
    reps, sizes = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    k = C.c_int64(0)
    args = [L.pw(graph), int(graph.shape[0]), n] if name.endswith("_from_pairs") else [L.pw(graph), n]
    args += [min_samples] * dbscan + [L.ptr(labels, C.c_int32), L.pi(reps), L.pi(sizes)]
    if dbscan:
        core, degrees = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.int32)
        args += [L.pb(core), L.ptr(degrees, C.c_int32)]
    if butina:
        degrees = np.zeros(n, dtype=np.int32)
        args += [L.ptr(degrees, C.c_int32)]
    L.call(name, *args, C.byref(k))
    reps, sizes = reps[:k.value].copy(), sizes[:k.value].copy()
    if butina:
        return RmsdButina(labels, reps, sizes, degrees)
    return RmsdDbscan(labels, reps, sizes, core.astype(bool), degrees) if dbscan else RmsdClusters(labels, reps, sizes)


def _bit_matrix(bits, n):
    """a caller's (n, ceil(n/64)) uint64 bit matrix, checked -> contiguous"""
    bits = np.asarray(bits)
    if bits.dtype != np.uint64 or bits.ndim != 2 or bits.shape != (n, (n + 63) // 64):
        raise L.FirecodeHipInputError(
            L.FC_E_INVALID, f"bits must be ({n}, {(n + 63) // 64}) uint64, got {bits.shape} {bits.dtype}")
    return np.ascontiguousarray(bits)


def _vertex_count(n):
    if isinstance(n, (bool, np.bool_)) or int(n) != n or int(n) < 0:
        raise L.FirecodeHipInputError(L.FC_E_INVALID, f"n={n!r}: a vertex count >= 0")
    if int(n) > 2 ** 31 - 257:
        raise L.FirecodeHipInputError(L.FC_E_LIMIT, f"n={n!r}: clusters index vertices with 32 bits")
    return int(n)


def clusters_from_pairs(pairs, n):
    """The labelling of ``cluster_by_rmsd`` on a caller's graph (fc_clusters_from_pairs): ``pairs`` (P,) uint64
    ``(i << 32) | j`` -- the format of ``DeviceEnsemble.similar_pairs`` -- in either order, duplicates allowed, or a
    (P, 2) integer array of (i, j); ``n`` vertices.  ``i == j`` or an index outside [0, n) is refused before any device
    use.  Returns ``RmsdClusters``: clusters numbered by ascending smallest member, which is their representative."""
    n = _vertex_count(n)
    return _labels_from_graph("fc_clusters_from_pairs", _pair_words(pairs, n), n)


def _pair_words(pairs, n):
    """a caller's pair list, (P,) words or (P, 2) indices -> (P,) uint64 words, every check made"""
    pairs = np.asarray(pairs)
    if pairs.ndim == 2 and pairs.shape[1] == 2:
        ij = pairs.astype(np.int64)
        if ij.size and (ij.min() < 0 or ij.max() >= n):
            raise L.FirecodeHipInputError(L.FC_E_INVALID, f"a pair index outside [0, {n})")
        pairs = (ij[:, 0].astype(np.uint64) << np.uint64(32)) | ij[:, 1].astype(np.uint64)
    elif pairs.ndim != 1:
        raise L.FirecodeHipInputError(L.FC_E_INVALID, f"pairs must be (P,) uint64 or (P, 2), got {pairs.shape}")
    if pairs.size and pairs.dtype.kind not in "ui":
        raise L.FirecodeHipInputError(L.FC_E_INVALID, f"pairs must be integers, got {pairs.dtype}")
    if pairs.size and pairs.dtype.kind == "i" and pairs.min() < 0:
        raise L.FirecodeHipInputError(L.FC_E_INVALID, "negative pair word")
    pairs = np.ascontiguousarray(pairs, dtype=np.uint64)
    hi, lo = pairs >> np.uint64(32), pairs & np.uint64(0xFFFFFFFF)
    if pairs.size and ((hi == lo).any() or hi.max() >= n or lo.max() >= n):
        raise L.FirecodeHipInputError(L.FC_E_INVALID, f"a pair with i == j or an index outside [0, {n})")
    return pairs


def clusters_from_bits(bits, n):
    """The labelling of ``cluster_by_rmsd`` on a caller's (n, ceil(n/64)) uint64 bit matrix in the layout of
    ``greedy_prune_from_bits`` / ``DeviceEnsemble.simbits`` / ``fc_tfd_simbits`` (fc_clusters_from_bits): an edge
    (i, j) where bit j of row i is set; only bits j > i are read."""
    n = _vertex_count(n)
    return _labels_from_graph("fc_clusters_from_bits", _bit_matrix(bits, n), n)


RmsdDbscan = namedtuple("RmsdDbscan", ["labels", "representatives", "sizes", "core", "degrees"])


def _empty_dbscan():
    return RmsdDbscan(np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64),
                      np.zeros(0, dtype=bool), np.zeros(0, dtype=np.int32))


def dbscan_by_rmsd(structures, atoms, max_rmsd=None, max_dev=None, min_samples=5, energies=None, max_dE=0.0,
                   debugfunction=None, heavy_atoms_only=True, prune_enantiomers=False, symmetry=None):
    """Which conformers form a populated region: density-based clusters (DBSCAN) on the similarity graph of
    ``cluster_by_rmsd`` -- the same edges, the same options -- on the GPU (fc_rmsd_dbscan; the contract is written out
    in include/fc_hip.h).  A conformer is a core point when it and its neighbours number at least ``min_samples``; the
    clusters are the connected components of the core points, so a thin chain of intermediates does not weld two basins
    together; a conformer that is not core joins the cluster of its first core neighbour in processing order (border),
    or, with none, is noise.

    Returns ``RmsdDbscan(labels, representatives, sizes, core, degrees)`` in the caller's order: labels (N,) int32, -1 for
    noise; representatives (K,) int64 indices into ``structures``, the first core member of each cluster in processing
    order -- lowest energy when ``energies`` is usable, lowest index otherwise -- with clusters numbered in that order;
    sizes (K,) int64, core and border members; core (N,) bool; degrees (N,) int32, the number of neighbours of each
    conformer: its local density at ``max_rmsd``.  ``min_samples=1`` gives the clusters of ``cluster_by_rmsd``."""
    t0 = perf_counter()
    enant = L.check_flag("prune_enantiomers", prune_enantiomers)
    min_samples = L.check_min_samples(min_samples)
    structures, table, (max_rmsd, max_dev, max_dE), heavy, order, en_sorted, X = _graph_inputs(
        structures, atoms, max_rmsd, max_dev, energies, max_dE, heavy_atoms_only, enant, symmetry)
    N = structures.shape[0]
    if N == 0:
        return _empty_dbscan()
    with L.DeviceEnsemble(X, atom_mask=heavy, center=True) as ens:
        labels, reps, sizes, core, degrees, stats = ens.dbscan(max_rmsd, max_dev, min_samples, energies=en_sorted,
                                                               max_dE=max_dE, prune_enantiomers=enant, symmetry=table)
    if order is not None:
        labels, core, degrees = _unsort(labels, order), _unsort(core, order), _unsort(degrees, order)
        reps = order[reps].astype(np.int64)
    if debugfunction is not None:
        debugfunction(
            f"DEBUG: dbscan_by_rmsd [gfx950{', mirror images included' if enant else ''}"
            f"{'' if table is None else f', {len(table)} atom permutations'}] - {stats[0]} pairs screened, "
            f"{stats[2]} similar, min_samples {min_samples}: {len(sizes)} clusters, {stats[6]} core, "
            f"{N - int(stats[6]) - int(stats[7])} border, {stats[7]} noise, in {perf_counter() - t0:.3f} s")
    return RmsdDbscan(labels, reps, sizes, core, degrees)


def dbscan_from_pairs(pairs, n, min_samples, assume_unique=False):
    """The labelling of ``dbscan_by_rmsd`` on a caller's graph (fc_dbscan_from_pairs): ``pairs`` and ``n`` as
    ``clusters_from_pairs`` takes them, with the same checks before any device use.  Degrees count list entries, so
    every unordered pair must be listed once: the list is brought to (min, max) order and duplicates are removed here
    unless ``assume_unique=True`` (the output of ``DeviceEnsemble.similar_pairs`` is), in which case a pair listed twice
    counts twice.  Returns ``RmsdDbscan``."""
    n = _vertex_count(n)
    min_samples = L.check_min_samples(min_samples)
    assume_unique = L.check_flag("assume_unique", assume_unique)
    pairs = _pair_words(pairs, n)
    if not assume_unique:
        hi, lo = pairs >> np.uint64(32), pairs & np.uint64(0xFFFFFFFF)
        pairs = np.unique((np.minimum(hi, lo) << np.uint64(32)) | np.maximum(hi, lo))
    return _labels_from_graph("fc_dbscan_from_pairs", np.ascontiguousarray(pairs, dtype=np.uint64), n, min_samples)


def dbscan_from_bits(bits, n, min_samples):
    """The labelling of ``dbscan_by_rmsd`` on a caller's (n, ceil(n/64)) uint64 bit matrix (fc_dbscan_from_bits): the
    layout and the checks of ``clusters_from_bits``; only bits j > i are read, so no pair can count twice."""
    n = _vertex_count(n)
    min_samples = L.check_min_samples(min_samples)
    return _labels_from_graph("fc_dbscan_from_bits", _bit_matrix(bits, n), n, min_samples)


class RmsdButina(namedtuple("RmsdButina", ["labels", "centroids", "sizes", "degrees"])):
    """What ``butina_by_rmsd`` returns; ``members(k)``: the indices of cluster ``k``, ascending."""
    __slots__ = ()

    def members(self, k):
        if isinstance(k, (bool, np.bool_)) or int(k) != k or not 0 <= int(k) < len(self.centroids):
            raise IndexError(f"cluster {k!r}: there are {len(self.centroids)}")
        return np.flatnonzero(self.labels == int(k))


def butina_by_rmsd(structures, atoms, max_rmsd=None, max_dev=None, energies=None, max_dE=0.0, debugfunction=None,
                   heavy_atoms_only=True, prune_enantiomers=False, symmetry=None):
    """Centroids and their members: the sphere-exclusion clustering of Butina (1999) on the similarity graph of
    ``cluster_by_rmsd`` -- the same edges, the same options -- on the GPU (fc_rmsd_butina; the contract is written out
    in include/fc_hip.h).  Conformers are ranked by their number of neighbours, the lower energy (the lower index where
    ``energies`` is not usable) first on ties; the best-ranked unassigned conformer becomes a centroid and takes all of
    its unassigned neighbours, until none is left.  Every member is a neighbour of its centroid -- within ``max_rmsd``
    and ``max_dev`` of it -- which neither the components nor the density-based clusters promise.  Degrees are not
    updated while clusters form (RDKit: ``reordering=False``).  Unlike RDKit's ``Butina.ClusterData`` the threshold is
    the prune's strict ``<`` and a tie of degrees goes to the lowest, not the highest, index.

    Returns ``RmsdButina(labels, centroids, sizes, degrees)`` in the caller's order: labels (N,) int32; centroids (K,)
    int64 indices into ``structures``, clusters numbered by ascending centroid in processing order; sizes (K,) int64,
    the centroid included; degrees (N,) int32.  ``.members(k)``: the indices of cluster ``k``."""
    t0 = perf_counter()
    enant = L.check_flag("prune_enantiomers", prune_enantiomers)
    structures, table, (max_rmsd, max_dev, max_dE), heavy, order, en_sorted, X = _graph_inputs(
        structures, atoms, max_rmsd, max_dev, energies, max_dE, heavy_atoms_only, enant, symmetry)
    N = structures.shape[0]
    if N == 0:
        return RmsdButina(np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64),
                          np.zeros(0, dtype=np.int32))
    with L.DeviceEnsemble(X, atom_mask=heavy, center=True) as ens:
        labels, reps, sizes, degrees, stats = ens.butina(max_rmsd, max_dev, energies=en_sorted, max_dE=max_dE,
                                                         prune_enantiomers=enant, symmetry=table)
    if order is not None:
        labels, degrees = _unsort(labels, order), _unsort(degrees, order)
        reps = order[reps].astype(np.int64)
    if debugfunction is not None:
        debugfunction(
            f"DEBUG: butina_by_rmsd [gfx950{', mirror images included' if enant else ''}"
            f"{'' if table is None else f', {len(table)} atom permutations'}] - {stats[0]} pairs screened, "
            f"{stats[2]} similar: {len(sizes)} clusters, largest {int(sizes.max())}, {int((sizes == 1).sum())} singletons, "
            f"{stats[6]} rounds, in {perf_counter() - t0:.3f} s")
    return RmsdButina(labels, reps, sizes, degrees)


def butina_from_pairs(pairs, n, assume_unique=False):
    """The labelling of ``butina_by_rmsd`` on a caller's graph (fc_butina_from_pairs): ``pairs``, ``n`` and
    ``assume_unique`` as ``dbscan_from_pairs`` takes them, with the same checks before any device use and the same
    removal of duplicates.  Returns ``RmsdButina``; the smaller index comes first among vertices of one degree."""
    n = _vertex_count(n)
    assume_unique = L.check_flag("assume_unique", assume_unique)
    pairs = _pair_words(pairs, n)
    if not assume_unique:
        hi, lo = pairs >> np.uint64(32), pairs & np.uint64(0xFFFFFFFF)
        pairs = np.unique((np.minimum(hi, lo) << np.uint64(32)) | np.maximum(hi, lo))
    return _labels_from_graph("fc_butina_from_pairs", np.ascontiguousarray(pairs, dtype=np.uint64), n)


def butina_from_bits(bits, n):
    """The labelling of ``butina_by_rmsd`` on a caller's (n, ceil(n/64)) uint64 bit matrix (fc_butina_from_bits): the
    layout and the checks of ``clusters_from_bits``; only bits j > i are read."""
    n = _vertex_count(n)
    return _labels_from_graph("fc_butina_from_bits", _bit_matrix(bits, n), n)


RmsdSilhouette = namedtuple("RmsdSilhouette", ["values", "intra", "nearest_mean", "nearest", "cluster_means", "sizes", "score"])
SilhouetteScanRecord = namedtuple("SilhouetteScanRecord", ["max_rmsd", "n_clusters", "n_noise", "score"])


def silhouette_by_rmsd(structures, atoms, labels, heavy_atoms_only=True):
    """How good is a labelling: the silhouette of every labelled conformer under the heavy-atom Kabsch RMSD of
    ``prune_by_rmsd`` (centred, ``rmsd_and_max(...)[0]``), on the GPU, without an N x N matrix
    (fc_ensemble_silhouette; the contract is written out in include/fc_hip.h).  ``labels``: one integer per conformer, a
    negative one = in no group -- the ``labels`` of ``RmsdClusters``, ``RmsdDbscan`` (-1 is noise), ``RmsdButina`` and
    ``RmsdKMedoids`` as they come; ``None``: the whole ensemble is one group.

    Returns ``RmsdSilhouette(values, intra, nearest_mean, nearest, cluster_means, sizes, score)``: per conformer the
    silhouette ``s = (b - a) / max(a, b)`` in [-1, 1] (0 for the only member of a group), ``a`` = the mean distance to
    the other members of its own group, ``b`` = the smallest mean distance to the members of another group and
    ``nearest`` (int32) = that group, the lowest label on ties -- a conformer with ``s`` near 0 sits between its own
    group and ``nearest``; per group (largest label + 1 of them) the mean of ``s`` and the member count; ``score``,
    the mean of ``s`` over the labelled conformers.  A conformer in no group has NaN values and ``nearest`` -1, an empty
    group id a NaN mean; with fewer than two non-empty groups ``values``, ``nearest_mean`` and ``score`` are NaN."""
    structures, heavy = _medoid_inputs(structures, atoms, heavy_atoms_only)
    N = structures.shape[0]
    lab, n_groups = L.check_group_labels(labels, N)
    if N == 0:
        return RmsdSilhouette(np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.int32), np.full(n_groups, np.nan),
                              np.zeros(n_groups, dtype=np.int64), float("nan"))
    with L.DeviceEnsemble(structures, atom_mask=heavy, center=True) as ens:
        return RmsdSilhouette(*ens.silhouette(lab, n_groups))


def silhouette_scan(structures, atoms, thresholds, method="butina", max_dev=None, min_samples=5, heavy_atoms_only=True):
    """Which ``max_rmsd`` should I cluster at: for every threshold of ``thresholds`` the clusters of ``method`` --
    ``"butina"`` (``butina_by_rmsd``), ``"components"`` (``cluster_by_rmsd``) or ``"dbscan"`` (``dbscan_by_rmsd`` with
    ``min_samples``) -- and their silhouette score, with the ensemble uploaded ONCE: the clusterer and the silhouette
    of every step run on the same resident ensemble.  ``max_dev``: as in the clusterers (default: twice the step's
    ``max_rmsd``).

    Returns one ``SilhouetteScanRecord(max_rmsd, n_clusters, n_noise, score)`` per threshold, in their order:
    ``n_noise`` counts the conformers in no cluster (DBSCAN's noise; 0 otherwise), ``score`` is that of
    ``silhouette_by_rmsd`` under the step's labels (NaN with fewer than two clusters)."""
    if method not in ("butina", "components", "dbscan"):
        raise L.FirecodeHipInputError(L.FC_E_INVALID, f"method={method!r}: 'butina', 'components' or 'dbscan'")
    structures, heavy = _medoid_inputs(structures, atoms, heavy_atoms_only)
    min_samples = L.check_min_samples(min_samples)
    ts = np.asarray(thresholds, dtype=np.float64)
    if ts.ndim != 1:
        raise L.FirecodeHipInputError(L.FC_E_INVALID, f"thresholds must be a 1-D sequence of max_rmsd values, got {ts.shape}")
    steps = [_thresholds(L.check_max_rmsd_cap(t), max_dev, 0.0) for t in ts]
    if structures.shape[0] == 0:
        return [SilhouetteScanRecord(float(t), 0, 0, float("nan")) for t in ts]
    records = []
    with L.DeviceEnsemble(structures, atom_mask=heavy, center=True) as ens:
        for t, (max_rmsd, dev, _) in zip(ts, steps):
            if method == "butina":
                out = ens.butina(max_rmsd, dev)
            elif method == "components":
                out = ens.clusters(max_rmsd, dev)
            else:
                out = ens.dbscan(max_rmsd, dev, min_samples)
            labels, sizes = out[0], out[2]  # (every clusterer: labels, representatives, sizes, ...)
            score = ens.silhouette(labels, max(len(sizes), 1))[6]
            records.append(SilhouetteScanRecord(float(t), len(sizes), int((labels < 0).sum()), score))
    return records


def silhouette_by_rmsd_sym(structures, atoms, labels, heavy_atoms_only=True, symmetry=None, prune_enantiomers=False):
    """``silhouette_by_rmsd`` under the symmetry-corrected distance of ``medoids_by_rmsd_sym``
    (fc_ensemble_silhouette_perm): the distance the labelling of ``cluster_by_rmsd(..., symmetry=)`` or
    ``butina_by_rmsd(..., prune_enantiomers=True)`` was made under, so that a group of flipped or mirrored copies is
    judged tight, not ångströms wide.  With neither keyword this is ``silhouette_by_rmsd``.  Returns ``RmsdSilhouette``."""
    structures, heavy = _medoid_inputs(structures, atoms, heavy_atoms_only)
    atoms = np.asarray(atoms)
    table, enant = _sums_symmetry(symmetry, prune_enantiomers, atoms, heavy, heavy_atoms_only)
    N = structures.shape[0]
    lab, n_groups = L.check_group_labels(labels, N)
    if N == 0:
        return RmsdSilhouette(np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.int32), np.full(n_groups, np.nan),
                              np.zeros(n_groups, dtype=np.int64), float("nan"))
    with L.DeviceEnsemble(structures, atom_mask=heavy, center=True) as ens:
        return RmsdSilhouette(*ens.silhouette_sym(lab, n_groups, symmetry=table, prune_enantiomers=enant))


def silhouette_scan_sym(structures, atoms, thresholds, method="butina", max_dev=None, min_samples=5, heavy_atoms_only=True,
                        symmetry=None, prune_enantiomers=False):
    """``silhouette_scan`` where the clusterer AND the silhouette of every step work under the same symmetry-corrected
    distance, with the ensemble uploaded once: ``symmetry=`` (a bond graph or a (K, A) table) or
    ``prune_enantiomers=True`` is passed on to both.  The clusterers take one of the two, not both, so the combination
    is refused here with their error.  With neither keyword this is ``silhouette_scan``.  Returns one
    ``SilhouetteScanRecord`` per threshold."""
    from firecode_amd import symmetry as S

    if method not in ("butina", "components", "dbscan"):
        raise L.FirecodeHipInputError(L.FC_E_INVALID, f"method={method!r}: 'butina', 'components' or 'dbscan'")
    structures, heavy = _medoid_inputs(structures, atoms, heavy_atoms_only)
    atoms = np.asarray(atoms)
    enant = L.check_flag("prune_enantiomers", prune_enantiomers)
    S.refuse_with_enantiomers(S.resolve(symmetry, atoms, heavy_atoms_only), enant)
    table, enant = _sums_symmetry(symmetry, enant, atoms, heavy, heavy_atoms_only)
    min_samples = L.check_min_samples(min_samples)
    ts = np.asarray(thresholds, dtype=np.float64)
    if ts.ndim != 1:
        raise L.FirecodeHipInputError(L.FC_E_INVALID, f"thresholds must be a 1-D sequence of max_rmsd values, got {ts.shape}")
    steps = [_thresholds(L.check_max_rmsd_cap(t), max_dev, 0.0) for t in ts]
    if structures.shape[0] == 0:
        return [SilhouetteScanRecord(float(t), 0, 0, float("nan")) for t in ts]
    records = []
    with L.DeviceEnsemble(structures, atom_mask=heavy, center=True) as ens:
        for t, (max_rmsd, dev, _) in zip(ts, steps):
            if method == "butina":
                out = ens.butina(max_rmsd, dev, prune_enantiomers=enant, symmetry=table)
            elif method == "components":
                out = ens.clusters(max_rmsd, dev, prune_enantiomers=enant, symmetry=table)
            else:
                out = ens.dbscan(max_rmsd, dev, min_samples, prune_enantiomers=enant, symmetry=table)
            labels, sizes = out[0], out[2]  # (every clusterer: labels, representatives, sizes, ...)
            score = ens.silhouette_sym(labels, max(len(sizes), 1), symmetry=table, prune_enantiomers=enant)[6]
            records.append(SilhouetteScanRecord(float(t), len(sizes), int((labels < 0).sum()), score))
    return records


def rotation_mask(graph, torsion, n_atoms=None):
    """``_get_rotation_mask`` (firecode/torsion_module.py:354-382): the atoms that rotate
    with i4 -- reachable from i4 once the i2-i3 edge is removed -- with i3 excluded."""
    import networkx as nx

    _, i2, i3, i4 = (int(t) for t in torsion)
    n = graph.number_of_nodes() if n_atoms is None else n_atoms
    had = graph.has_edge(i2, i3)
    if had:
        graph.remove_edge(i2, i3)
    try:
        reach = nx.node_connected_component(graph, i4)
    finally:
        if had:
            graph.add_edge(i2, i3)
    mask = np.zeros(n, dtype=bool)
    mask[list(reach)] = True
    mask[i3] = False
    return mask


def prune_many_by_rmsd(ensembles, max_rmsd=None, max_dev=None, heavy_atoms_only=True, min_per_group=20):
    """``prune_by_rmsd`` for a queue of ensembles: ``ensembles`` is a list of
    ``(structures, atoms)``; returns a list of ``(structures[mask], mask)``, each identical to
    what ``prune_by_rmsd(structures, atoms, max_rmsd, max_dev)`` returns.  All ensembles are made
    resident, their prunes are enqueued together (``fc_prune_rmsd_many``) and the host waits once;
    the reference prunes one ensemble per call (the loop a maintainer would write around
    firecode/ensemble.py:230-235)."""
    max_rmsd, max_dev, _ = _thresholds(max_rmsd, max_dev, 0.0)
    items, resident = [], []
    try:
        for structures, atoms in ensembles:
            structures = L.f64(structures)
            if structures.ndim != 3 or structures.shape[2] != 3:
                raise L.FirecodeHipInputError(L.FC_E_INVALID, f"structures must be (N, A, 3), got {structures.shape}")
            atoms = np.asarray(atoms)
            if atoms.shape[0] != structures.shape[1]:
                raise L.FirecodeHipInputError(L.FC_E_INVALID, "len(atoms) != number of atoms")
            items.append(structures)
            if structures.shape[0] == 0:
                resident.append(None)
                continue
            heavy = (atoms != "H") if heavy_atoms_only else np.ones(len(atoms), dtype=bool)
            resident.append(L.DeviceEnsemble(structures, atom_mask=heavy, center=True))
        live = [e for e in resident if e is not None]
        masks, _ = L.prune_many(live, max_rmsd, max_dev, min_per_group) if live else ([], None)
    finally:
        for e in resident:
            if e is not None:
                e.close()
    out, it = [], iter(masks)
    for structures, e in zip(items, resident):
        mask = np.ones(0, dtype=bool) if e is None else next(it)
        out.append((structures[mask], mask))
    return out


def prune_by_rmsd_rot_corr(structures, atoms, graph=None, max_rmsd=0.25, max_dev=None, energies=None, max_dE=0.0,
                           logfunction=None, debugfunction=None, torsions=None, rotation_masks=None,
                           min_per_group=20, return_bits=False):
    """``prune_by_rmsd_rot_corr`` (prism_pruner.pruner; call sites firecode/ensemble.py:253-260,
    embedder.py:1489-1496, operators.py:626-632): RMSD pruning that is invariant to rotations of
    locally symmetric groups (tBu, Ph, NMe2 ...).

    Called as the reference calls it -- ``(structures, atoms, graph, max_rmsd=..., energies=...,
    max_dE=..., logfunction=..., debugfunction=...)`` -- the locally symmetric torsions are
    perceived from ``graph`` (``firecode_amd.torsion_perception.symmetric_torsions``: the in-tree
    ``_get_torsions(..., keepdummy=True, mode="symmetry")`` filtered to dummy rotations).
    ``torsions=`` may instead give them explicitly as ``(i1, i2, i3, i4, n_fold)`` (an empty list:
    the molecule has none, plain heavy-atom RMSD prune); without both ``graph`` and ``torsions``
    the call is refused -- it never runs as an uncorrected prune under this name.
    ``rotation_masks`` (T, A) may be given, or are derived from ``graph`` like
    ``_get_rotation_mask`` does.  PARITY UNPINNED (third-party algorithm restated, see
    include/fc_hip.h)."""
    from firecode_amd.torsion_module import N_FOLD_ANGLES

    t0 = perf_counter()
    structures = L.f64(structures)
    if structures.ndim != 3 or structures.shape[2] != 3:
        raise L.FirecodeHipInputError(L.FC_E_INVALID, f"structures must be (N, A, 3), got {structures.shape}")
    atoms = np.asarray(atoms)
    N, A = structures.shape[:2]
    if atoms.shape[0] != A:
        raise L.FirecodeHipInputError(L.FC_E_INVALID, "len(atoms) != number of atoms")
    max_rmsd, max_dev, max_dE = _thresholds(max_rmsd, max_dev, max_dE)
    if N == 0:
        return structures, np.ones(0, dtype=bool)
    if torsions is None:
        if graph is None:
            raise L.FirecodeHipInputError(
                L.FC_E_INVALID, "prune_by_rmsd_rot_corr needs the molecular graph (third positional argument, as "
                "firecode/ensemble.py:253 passes it) or torsions=: without them no symmetry correction is possible")
        from firecode_amd.torsion_perception import symmetric_torsions

        torsions = symmetric_torsions(graph, structures[0], atoms)
    torsions = list(torsions)
    T = len(torsions)
    quads = L.i64(np.array([t[:4] for t in torsions], dtype=np.int64).reshape(T, 4))
    if rotation_masks is None:
        if T and graph is None:
            raise L.FirecodeHipInputError(L.FC_E_INVALID, "rotation_masks or graph is required with torsions")
        rotation_masks = [rotation_mask(graph, t[:4], A) for t in torsions]
    masks = L.u8(np.asarray(rotation_masks, dtype=bool).reshape(T, A))
    sets = [N_FOLD_ANGLES[int(t[4])] for t in torsions]
    max_angles = max([len(a) for a in sets] + [1])
    angles = np.zeros((T, max_angles))
    n_angles = np.zeros(T, dtype=np.int32)
    for k, a in enumerate(sets):
        angles[k, : len(a)] = a
        n_angles[k] = len(a)
    heavy = L.u8(atoms != "H")
    order, en_sorted = _sorted_by_energy(structures, energies)
    X = structures if order is None else np.ascontiguousarray(structures[order])
    mask_sorted = np.zeros(N, dtype=np.uint8)
    W = (N + 63) // 64
    bits = np.zeros((N, W), dtype=np.uint64) if return_bits else None
    import ctypes as C

    L.call("fc_prune_rmsd_rot_corr", L.pf(X), N, A, L.pb(heavy), L.pi(quads), T, L.pb(masks), L.pf(angles),
           n_angles.ctypes.data_as(C.POINTER(C.c_int32)), max_angles, float(max_rmsd), float(max_dev),
           None if en_sorted is None else L.pf(L.f64(en_sorted)), float(max_dE), int(min_per_group),
           L.pb(mask_sorted), None if bits is None else L.pw(bits))
    mask = _unsort(mask_sorted.astype(bool), order)
    for fn in (logfunction, debugfunction):
        if fn is not None:
            fn(f"DEBUG: prune_by_rmsd_rot_corr [gfx950] - {T} symmetric torsions, keeping {int(mask.sum())}/{N} "
               f"in {perf_counter() - t0:.3f} s")
    if return_bits:
        return structures[mask], mask, bits
    return structures[mask], mask


def prune_by_moment_of_inertia(structures, atoms, max_deviation=None, energies=None, max_dE=0.0,
                               debugfunction=None, min_per_group=20):
    """MOI pruning: similar when all three principal moments differ by less
    than ``max_deviation`` relative to the earlier structure of the pair."""
    t0 = perf_counter()
    structures = L.f64(structures)
    if structures.ndim != 3 or structures.shape[2] != 3:
        raise L.FirecodeHipInputError(L.FC_E_INVALID, f"structures must be (N, A, 3), got {structures.shape}")
    N, A = structures.shape[0], structures.shape[1]
    if N == 0:
        return structures, np.ones(0, dtype=bool)
    if max_deviation is None:
        max_deviation = CONVENTIONS["moi_tolerance"]
    masses = np.array([pt.mass(a) for a in atoms], dtype=np.float64)
    order, en_sorted = _sorted_by_energy(structures, energies)
    X = structures if order is None else np.ascontiguousarray(structures[order])
    mask8 = np.zeros(N, dtype=np.uint8)
    L.call("fc_prune_moi", L.pf(X), N, A, L.pf(masses), float(max_deviation), L.pf(en_sorted),
           float(max_dE), int(min_per_group), L.pb(mask8))
    mask = _unsort(mask8.astype(bool), order)
    if debugfunction is not None:
        debugfunction(f"DEBUG: prune_by_moment_of_inertia [gfx950] - keeping {int(mask.sum())}/{N} "
                      f"in {perf_counter() - t0:.3f} s")
    return structures[mask], mask


def prune_similarity(structures, atoms, moi=True, rmsd=True, max_rmsd=None, max_dev=None, max_deviation=None,
                     energies=None, max_dE=0.0, heavy_atoms_only=True, min_per_group=20, prune_enantiomers=False):
    """The MOI and RMSD stages of ``Ensemble.similarity_pruning`` (firecode/ensemble.py:205-235) /
    ``Embedder.similarity_refining`` (embedder.py:1445-1474) on ONE upload of the coordinates
    (``fc_prune_similarity``): the MOI stage runs on the resident structures, its survivors are gathered
    on the device into the RMSD stage's layout, the masks are composed on the way out.  Stage by
    stage the masks equal ``prune_by_moment_of_inertia`` followed by ``prune_by_rmsd`` on its output.
    Returns ``(mask_after_moi, mask_after_both, (n_in, n_after_moi, n_after_rmsd))`` in the caller's order.

    ``prune_enantiomers=True``: the MOI stage as it is, then the enantiomer-aware RMSD stage (``prune_by_rmsd(...,
    prune_enantiomers=True)``) on its survivors -- two uploads; same masks / counts contract."""
    enant = L.check_flag("prune_enantiomers", prune_enantiomers)
    structures = L.f64(structures)
    if structures.ndim != 3 or structures.shape[2] != 3:
        raise L.FirecodeHipInputError(L.FC_E_INVALID, f"structures must be (N, A, 3), got {structures.shape}")
    atoms = np.asarray(atoms)
    N, A = structures.shape[:2]
    if atoms.shape[0] != A:
        raise L.FirecodeHipInputError(L.FC_E_INVALID, "len(atoms) != number of atoms")
    max_rmsd, max_dev, max_dE = _thresholds(max_rmsd, max_dev, max_dE)
    if max_deviation is None:
        max_deviation = CONVENTIONS["moi_tolerance"]
    counts = np.array([N, N, N], dtype=np.int64)
    if N == 0:
        return np.ones(0, dtype=bool), np.ones(0, dtype=bool), counts
    heavy = L.u8((atoms != "H") if heavy_atoms_only else np.ones(A, dtype=bool))
    masses = np.array([pt.mass(a) for a in atoms], dtype=np.float64)
    order, en_sorted = _sorted_by_energy(structures, energies)
    X = structures if order is None else np.ascontiguousarray(structures[order])
    m1, m2 = np.zeros(N, dtype=np.uint8), np.zeros(N, dtype=np.uint8)
    if enant and rmsd:
        if moi:
            L.call("fc_prune_similarity", L.pf(X), N, A, L.pb(heavy), L.pf(masses), 1, float(max_deviation), 0, max_rmsd,
                   max_dev, L.pf(en_sorted), max_dE, int(min_per_group), L.pb(m1), L.pb(m2), L.pi(counts))
        else:
            m1[:] = 1
        keep = m1.astype(bool)
        with L.DeviceEnsemble(np.ascontiguousarray(X[keep]), atom_mask=heavy.astype(bool), center=True) as ens:
            sub, _ = ens.prune(max_rmsd, max_dev, energies=None if en_sorted is None else en_sorted[keep], max_dE=max_dE,
                               min_per_group=min_per_group, prune_enantiomers=True)
        m2[:] = 0
        m2[np.flatnonzero(keep)[sub]] = 1
        counts[:] = (N, int(keep.sum()), int(m2.sum()))
        return _unsort(m1.astype(bool), order), _unsort(m2.astype(bool), order), counts
    L.call("fc_prune_similarity", L.pf(X), N, A, L.pb(heavy), L.pf(masses), int(bool(moi)), float(max_deviation),
           int(bool(rmsd)), max_rmsd, max_dev, L.pf(en_sorted), max_dE, int(min_per_group), L.pb(m1), L.pb(m2),
           L.pi(counts))
    return _unsort(m1.astype(bool), order), _unsort(m2.astype(bool), order), counts


def prune(structures, atoms, max_rmsd=0.25, energies=None, max_dE=0.0, logfunction=None,
          debugfunction=None, prune_enantiomers=False):
    """Combined pipeline used by firecode/interfaces/goat.py:399: MOI, then RMSD.
    (The symmetry-corrected stage is a later row of SURVEY.md section 8f.)
    ``prune_enantiomers``: as in ``prune_similarity``."""
    structures = L.f64(structures)
    n0 = len(structures)
    _, mask, _ = prune_similarity(structures, atoms, max_rmsd=max_rmsd, energies=energies, max_dE=max_dE,
                                  prune_enantiomers=prune_enantiomers)
    for fn in (logfunction, debugfunction):
        if fn is not None:
            fn(f"Discarded {n0 - int(mask.sum())} candidates for MOI+RMSD similarity ({int(mask.sum())} left)")
    return structures[mask], mask


def greedy_prune_from_bits(bits, n, min_per_group=20):
    """k-ladder replay over a caller-supplied (n, ceil(n/64)) uint64 bit matrix."""
    bits = np.ascontiguousarray(bits, dtype=np.uint64)
    mask = np.zeros(n, dtype=np.uint8)
    L.call("fc_greedy_prune_from_bits", L.pw(bits), int(n), int(min_per_group), L.pb(mask))
    return mask.astype(bool)
