"""``Ensemble`` with the interface of firecode/ensemble.py:46-297, its
similarity pruning routed to the GPU pruner."""

from __future__ import annotations

import re
from dataclasses import dataclass, field
from pathlib import Path
from time import perf_counter
from typing import Callable

import numpy as np

from firecode_amd.pruner import prune_by_moment_of_inertia, prune_by_rmsd
from firecode_amd.pt import pt


_ENERGY = re.compile(r"-*\d+\.\d+")


def _comment_line_energies(text, n_frames):
    """The first decimal number of every frame's comment line (firecode/ensemble.py:58-98 reads the energies of
    a multi-frame .xyz from there), frame by frame through the line list: count line, comment line, that many
    atom lines.  A truncated last frame ends the walk (the reference swallows the end of the file the same way);
    a comment line without a number raises ValueError (the reference then trips over the atom lines)."""
    lines = text.splitlines()
    out, k = [], 0
    while k < len(lines) and len(out) < n_frames:
        if not lines[k].strip():
            k += 1
            continue
        n_atoms = int(lines[k])
        if k + 1 >= len(lines):
            break
        found = _ENERGY.search(lines[k + 1])
        if found is None:
            raise ValueError(f"no energy in the comment line of frame {len(out)}: {lines[k + 1]!r}")
        out.append(float(found.group()))
        k += 2 + n_atoms
    return out


@dataclass
class Ensemble:
    atoms: np.ndarray
    coords: np.ndarray
    filename: str = ""
    basename: str = ""
    atomnos: np.ndarray = field(default_factory=lambda: np.array([], dtype=int))
    energies: np.ndarray = field(default_factory=lambda: np.array([], dtype=float))
    logfunction: Callable[[str], None] | None = print

    @classmethod
    def from_xyz(cls, file, read_energies=False):
        """firecode/ensemble.py:58-98.  Coordinates are parsed by the library's
        C++ reader (same text rules, same values as float()); the energy regex
        of ``read_energies=True`` stays in Python (one line per conformer)."""
        from firecode_amd._lib import xyz_read

        atoms, coords = xyz_read(file)
        energies = np.array(_comment_line_energies(Path(file).read_text(), len(coords)) if read_energies else [])
        return cls(atoms=atoms, coords=coords, filename=str(file), basename=Path(str(file)).stem,
                   atomnos=np.array([pt.number(letter) for letter in atoms]), energies=energies)

    def to_xyz(self, file):
        """firecode/ensemble.py:284-297 -- byte-identical text, written by the library."""
        from firecode_amd._lib import xyz_write

        xyz_write(file, self.atoms, self.coords, label=self.basename, mode=0)

    @property
    def rel_energies(self):
        return self.energies - np.min(self.energies)

    def apply_mask(self, attributes, mask):
        """firecode/ensemble.py:175-183: keep the masked entries of every named array that has one entry
        per structure; attributes that are missing or of another length (empty ``energies``) stay as they are."""
        mask = np.asarray(mask)
        for name in attributes:
            values = getattr(self, name, None)
            if values is not None and (mask.dtype != bool or len(values) == len(mask)):
                setattr(self, name, values[mask])

    def dynamic_energy_thr(self, kcal_thr=10.0, keep_min=0.1, verbose=True):
        """firecode/ensemble.py:134-169: ``kcal_thr`` if it keeps more than ``keep_min`` of the structures,
        otherwise the first energy (in ensemble order) above it that does."""
        from firecode_amd.refining import first_threshold_keeping

        thr, kept = first_threshold_keeping(self.rel_energies, kcal_thr, keep_min)
        if kept is not None and verbose and self.logfunction is not None:
            self.logfunction(f"--> Dynamically adjusted energy threshold to {thr:.1f} kcal/mol to retain "
                             f"at least {kept * 100:.2f}% of structures.")
        return thr

    def energy_pruning(self, kcal_thr=10.0, verbose=True):
        """firecode/ensemble.py:117-132."""
        energy_thr = self.dynamic_energy_thr(kcal_thr, verbose=verbose)
        keep = self.rel_energies < energy_thr
        self.apply_mask(("coords", "energies"), keep)
        n_kept = int(np.count_nonzero(keep))
        if n_kept < len(keep) and verbose and self.logfunction is not None:
            self.logfunction(f"Discarded {len(keep) - n_kept} candidates for energy "
                             f"({n_kept} left, threshold {energy_thr:.1f} kcal/mol)")

    def sort_by_energy(self):
        order = np.argsort(self.energies)
        self.energies = self.energies[order]
        self.coords = self.coords[order]

    def diversity_selection(self, n=None, stop_rmsd=None, heavy_atoms_only=True, verbose=True, symmetry=None,
                            prune_enantiomers=False):
        """Keep the ``n`` most diverse structures, or representatives within ``stop_rmsd`` of every structure, by
        greedy max-min selection under the heavy-atom RMSD (``firecode_amd.pruner.select_diverse``; no reference
        counterpart: FIRECODE's ``most_diverse_conformers`` is a random draw).  Starts at the lowest energy when
        energies are known, else at the first structure; the kept structures stay in selection order and
        ``energies`` follow them.  ``symmetry=`` / ``prune_enantiomers=True``: as in ``select_diverse`` -- relabelled
        copies and mirror images count as the same structure.  Returns the ``DiverseSelection`` of the ensemble as it
        was."""
        from firecode_amd import symmetry as S
        from firecode_amd._lib import check_flag
        from firecode_amd.pruner import select_diverse

        enant = check_flag("prune_enantiomers", prune_enantiomers)
        table = S.resolve(symmetry, np.asarray(self.atoms), heavy_atoms_only)
        log = self.logfunction if verbose else None
        n0, t0 = len(self.coords), perf_counter()
        use_en = len(self.energies) == n0 and n0 > 0
        sel = select_diverse(self.coords, self.atoms, n=n, stop_rmsd=stop_rmsd, heavy_atoms_only=heavy_atoms_only,
                             energies=self.energies if use_en else None, symmetry=table, prune_enantiomers=enant)
        self.coords = self.coords[sel.indices]
        if use_en:
            self.apply_mask(("energies",), sel.indices)
        if log is not None:
            cover = float(sel.distances.max()) if n0 else 0.0
            aware = ("" if table is None else f", {len(table)} atom permutations") + (", mirror images included" if enant else "")
            log(f"Kept {len(sel.indices)} of {n0} candidates for RMSD diversity{aware} (covering radius {cover:.3f} A, "
                f"{perf_counter() - t0:.3f} s)")
        return sel

    def medoids(self, labels=None, heavy_atoms_only=True):
        """The structure that stands for each group: the member with the smallest summed heavy-atom RMSD to the other
        members (``firecode_amd.pruner.medoids_by_rmsd``).  ``labels``: the ``labels`` of ``cluster_by_rmsd``,
        ``dbscan_by_rmsd`` or ``butina_by_rmsd`` (negative: in no group); ``None``: the whole ensemble is one group.
        Returns the ``RmsdMedoids``; the ensemble is not masked."""
        from firecode_amd.pruner import medoids_by_rmsd

        return medoids_by_rmsd(self.coords, self.atoms, labels=labels, heavy_atoms_only=heavy_atoms_only)

    def silhouette(self, labels, heavy_atoms_only=True):
        """How good is a grouping of the structures: the silhouette of every labelled structure under the heavy-atom
        RMSD, per group and overall (``firecode_amd.pruner.silhouette_by_rmsd``).  ``labels``: the ``labels`` of
        ``cluster_by_rmsd``, ``dbscan_by_rmsd``, ``butina_by_rmsd`` or ``kmedoids_by_rmsd`` (negative: in no group).
        Returns the ``RmsdSilhouette``; the ensemble is not masked."""
        from firecode_amd.pruner import silhouette_by_rmsd

        return silhouette_by_rmsd(self.coords, self.atoms, labels, heavy_atoms_only=heavy_atoms_only)

    def kmedoids_selection(self, n, heavy_atoms_only=True, max_iter=50, verbose=True):
        """Keep the ``n`` most representative structures: k-medoids under the heavy-atom RMSD
        (``firecode_amd.pruner.kmedoids_by_rmsd``), started from the ``n`` most diverse ones.  Where
        ``diversity_selection`` keeps the extremes, this keeps the centres: the ``n`` structures with the smallest mean
        distance of every structure to its representative.  The kept structures stay in the order of the
        representatives and ``energies`` follow them.  Returns the ``RmsdKMedoids`` of the ensemble as it was."""
        from firecode_amd._lib import check_count
        from firecode_amd.pruner import kmedoids_by_rmsd

        n = check_count("n", n)
        n0, t0 = len(self.coords), perf_counter()
        use_en = len(self.energies) == n0 and n0 > 0
        sel = kmedoids_by_rmsd(self.coords, self.atoms, min(n, n0) if n0 else n, max_iter=max_iter,  # (n > N: all of them)
                               heavy_atoms_only=heavy_atoms_only)
        self.coords = self.coords[sel.medoids]
        if use_en:
            self.apply_mask(("energies",), sel.medoids)
        if verbose and self.logfunction is not None:
            mean = sel.cost / n0 if n0 else 0.0
            self.logfunction(f"Kept {len(sel.medoids)} of {n0} candidates as RMSD medoids (mean distance to the representative "
                             f"{mean:.3f} A, {sel.n_iter} assignments, {perf_counter() - t0:.3f} s)")
        return sel

    def medoids_sym(self, labels=None, heavy_atoms_only=True, symmetry=None, prune_enantiomers=False):
        """``medoids`` under the symmetry-corrected distance (``firecode_amd.pruner.medoids_by_rmsd_sym``): ``symmetry=`` /
        ``prune_enantiomers=True`` as in ``nearest_neighbours`` -- flipped or mirrored copies of a member are at distance
        0 from it.  Returns the ``RmsdMedoids``; the ensemble is not masked."""
        from firecode_amd.pruner import medoids_by_rmsd_sym

        return medoids_by_rmsd_sym(self.coords, self.atoms, labels=labels, heavy_atoms_only=heavy_atoms_only, symmetry=symmetry,
                                   prune_enantiomers=prune_enantiomers)

    def silhouette_sym(self, labels, heavy_atoms_only=True, symmetry=None, prune_enantiomers=False):
        """``silhouette`` under the symmetry-corrected distance (``firecode_amd.pruner.silhouette_by_rmsd_sym``): the one
        to judge the ``labels`` of a clusterer that was given ``symmetry=`` or ``prune_enantiomers=True`` by.  Returns
        the ``RmsdSilhouette``; the ensemble is not masked."""
        from firecode_amd.pruner import silhouette_by_rmsd_sym

        return silhouette_by_rmsd_sym(self.coords, self.atoms, labels, heavy_atoms_only=heavy_atoms_only, symmetry=symmetry,
                                      prune_enantiomers=prune_enantiomers)

    def kmedoids_selection_sym(self, n, heavy_atoms_only=True, max_iter=50, verbose=True, symmetry=None,
                               prune_enantiomers=False):
        """``kmedoids_selection`` under the symmetry-corrected distance (``firecode_amd.pruner.kmedoids_by_rmsd_sym``):
        relabelled copies and mirror images count as the same structure.  Returns the ``RmsdKMedoids`` of the ensemble
        as it was."""
        from firecode_amd._lib import check_count
        from firecode_amd.pruner import kmedoids_by_rmsd_sym

        n = check_count("n", n)
        n0, t0 = len(self.coords), perf_counter()
        use_en = len(self.energies) == n0 and n0 > 0
        sel = kmedoids_by_rmsd_sym(self.coords, self.atoms, min(n, n0) if n0 else n, max_iter=max_iter,  # (n > N: all of them)
                                   heavy_atoms_only=heavy_atoms_only, symmetry=symmetry, prune_enantiomers=prune_enantiomers)
        self.coords = self.coords[sel.medoids]
        if use_en:
            self.apply_mask(("energies",), sel.medoids)
        if verbose and self.logfunction is not None:
            mean = sel.cost / n0 if n0 else 0.0
            self.logfunction(f"Kept {len(sel.medoids)} of {n0} candidates as symmetry-aware RMSD medoids (mean distance to the "
                             f"representative {mean:.3f} A, {sel.n_iter} assignments, {perf_counter() - t0:.3f} s)")
        return sel

    def mean_structures(self, labels=None, refs=None, max_iter=50, tol=1e-9, heavy_atoms_only=True, aligned=False):
        """What each group looks like: its mean structure with the members superposed on it, the per-atom fluctuation
        about that mean, every member's RMSD to it and the closest member (``firecode_amd.pruner.group_means_by_rmsd``).
        ``labels``: the ``labels`` of a clusterer (negative: in no group); ``None``: the whole ensemble is one group;
        ``refs``: where each group starts (``None``, indices or ``"medoids"``).  Returns the ``RmsdGroupMeans``; the
        ensemble is not changed."""
        from firecode_amd.pruner import group_means_by_rmsd

        return group_means_by_rmsd(self.coords, self.atoms, labels=labels, refs=refs, max_iter=max_iter, tol=tol,
                                   heavy_atoms_only=heavy_atoms_only, aligned=aligned)

    def align_by_groups(self, labels, refs=None, max_iter=50, tol=1e-9, heavy_atoms_only=True):
        """Superpose the members of every group on their group's mean structure: ``coords`` is replaced by the
        ``aligned`` block of ``mean_structures`` (all atoms; every structure centred on its selected atoms, structures in
        no group unrotated), so that ``to_xyz`` writes each cluster as one bundle.  Returns the ``RmsdGroupMeans``."""
        res = self.mean_structures(labels=labels, refs=refs, max_iter=max_iter, tol=tol, heavy_atoms_only=heavy_atoms_only,
                                   aligned=True)
        self.coords = res.aligned
        return res

    def nearest_neighbours(self, k, heavy_atoms_only=True, symmetry=None, prune_enantiomers=False):
        """The ``k`` nearest neighbours of every structure under the heavy-atom RMSD of the other RMSD stages
        (``firecode_amd.pruner.knn_by_rmsd``).  Returns the ``RmsdNeighbours``, whose ``k_distances(min_samples - 1)`` is
        the curve one reads the ``max_rmsd`` of ``dbscan_by_rmsd`` from; the ensemble is not masked.  ``symmetry=`` /
        ``prune_enantiomers=True``: as in ``knn_by_rmsd`` -- relabelled copies and mirror images are at distance 0."""
        from firecode_amd.pruner import knn_by_rmsd

        return knn_by_rmsd(self.coords, self.atoms, k, heavy_atoms_only=heavy_atoms_only, symmetry=symmetry,
                           prune_enantiomers=prune_enantiomers)

    def _same_atoms(self, other):
        from firecode_amd._lib import FC_E_INVALID, FirecodeHipInputError

        if not isinstance(other, Ensemble):
            raise FirecodeHipInputError(FC_E_INVALID, f"the other ensemble must be an Ensemble, got {type(other).__name__}")
        mine, theirs = np.asarray(self.atoms), np.asarray(other.atoms)
        if mine.shape != theirs.shape or not np.array_equal(mine, theirs):
            raise FirecodeHipInputError(FC_E_INVALID, "the two ensembles do not have the same atoms")

    def nearest_in(self, other, k=1, max_rmsd=None, heavy_atoms_only=True, symmetry=None, prune_enantiomers=False):
        """For every structure its ``k`` nearest structures of ``other`` -- an ensemble of the same molecule, same
        ``atoms`` -- under the heavy-atom RMSD (``firecode_amd.pruner.knn_by_rmsd_against``); ``max_rmsd``: only those
        with ``rmsd < max_rmsd``.  Returns the ``RmsdCrossNeighbours`` (indices into ``other``); neither ensemble is
        masked.  RMSD only: no max-deviation or energy test.  ``symmetry=`` / ``prune_enantiomers=True``: as in
        ``knn_by_rmsd``."""
        from firecode_amd.pruner import knn_by_rmsd_against

        self._same_atoms(other)
        return knn_by_rmsd_against(self.coords, other.coords, self.atoms, k, max_rmsd=max_rmsd,
                                   heavy_atoms_only=heavy_atoms_only, symmetry=symmetry, prune_enantiomers=prune_enantiomers)

    def novel_against(self, other, max_rmsd, heavy_atoms_only=True, symmetry=None, prune_enantiomers=False):
        """(N,) bool: the structures with NO structure of ``other`` within ``max_rmsd`` of them
        (``firecode_amd.pruner.novel_conformers``); the ensemble is not masked.  RMSD only: the max-deviation and
        energy-window tests of ``similarity_pruning`` are not applied.  ``symmetry=`` / ``prune_enantiomers=True``: as
        in ``knn_by_rmsd`` -- a relabelled copy or a mirror image of a structure of ``other`` is not new."""
        from firecode_amd.pruner import novel_conformers

        self._same_atoms(other)
        return novel_conformers(self.coords, other.coords, self.atoms, max_rmsd, heavy_atoms_only=heavy_atoms_only,
                                symmetry=symmetry, prune_enantiomers=prune_enantiomers)

    def cluster_by_rmsd(self, max_rmsd=None, heavy_atoms_only=True, prune_enantiomers=False, verbose=True, symmetry=None):
        """Which conformers belong together (``firecode_amd.pruner.cluster_by_rmsd``): the connected components of the
        graph the RMSD stage of ``similarity_pruning`` prunes, with its energies and window (``max_dE = 1.0`` when there is
        one energy per conformer).  ``symmetry=``: as in ``similarity_pruning``.  Returns the ``RmsdClusters``; the ensemble is
        not masked."""
        from firecode_amd.pruner import cluster_by_rmsd

        use_en = len(self.energies) == len(self.coords)
        return cluster_by_rmsd(self.coords, self.atoms, max_rmsd, energies=self.energies if use_en else None,
                               max_dE=1.0 if use_en else 0.0, debugfunction=self.logfunction if verbose else None,
                               heavy_atoms_only=heavy_atoms_only, prune_enantiomers=prune_enantiomers, symmetry=symmetry)

    def dbscan_by_rmsd(self, max_rmsd=None, min_samples=5, heavy_atoms_only=True, prune_enantiomers=False, verbose=True,
                       symmetry=None):
        """Which conformers form a populated region (``firecode_amd.pruner.dbscan_by_rmsd``): density-based clusters on
        the graph of ``cluster_by_rmsd``, with its energies and window (``max_dE = 1.0`` when there is one energy per
        conformer).  Returns the ``RmsdDbscan``; the ensemble is not masked."""
        from firecode_amd.pruner import dbscan_by_rmsd

        use_en = len(self.energies) == len(self.coords)
        return dbscan_by_rmsd(self.coords, self.atoms, max_rmsd, min_samples=min_samples,
                              energies=self.energies if use_en else None, max_dE=1.0 if use_en else 0.0,
                              debugfunction=self.logfunction if verbose else None, heavy_atoms_only=heavy_atoms_only,
                              prune_enantiomers=prune_enantiomers, symmetry=symmetry)

    def butina_by_rmsd(self, max_rmsd=None, heavy_atoms_only=True, prune_enantiomers=False, verbose=True, symmetry=None):
        """Centroids and populations (``firecode_amd.pruner.butina_by_rmsd``): sphere-exclusion clusters on the graph of
        ``cluster_by_rmsd``, with its energies and window (``max_dE = 1.0`` when there is one energy per conformer).
        Returns the ``RmsdButina``; the ensemble is not masked."""
        from firecode_amd.pruner import butina_by_rmsd

        use_en = len(self.energies) == len(self.coords)
        return butina_by_rmsd(self.coords, self.atoms, max_rmsd, energies=self.energies if use_en else None,
                              max_dE=1.0 if use_en else 0.0, debugfunction=self.logfunction if verbose else None,
                              heavy_atoms_only=heavy_atoms_only, prune_enantiomers=prune_enantiomers, symmetry=symmetry)

    def similarity_pruning(self, moi=True, rmsd=True, rmsd_rot_corr=False, verbose=True, max_rmsd=None,
                           symmetric_torsions=None, graph=None, rotation_masks=None, prune_enantiomers=False,
                           symmetry=None):
        """firecode/ensemble.py:185-276: MOI prune, RMSD prune, then (``rmsd_rot_corr``, at
        most 1000 structures, :246-270) the symmetry-corrected RMSD prune; masks propagated to
        ``energies``.  Log messages as the reference words them, except the elapsed-time field: its
        ``time_to_string`` is third-party (prism_pruner.utils), seconds with three decimals here.
        ``max_rmsd=None``: the pruner's default, like the reference, which passes none (:230).  The rot-corr stage needs the locally symmetric torsions
        ``(i1, i2, i3, i4, n_fold)``: like the reference (:250) the graph is built with
        ``graphize(atoms, coords[0])`` when none is given, and ``prune_by_rmsd_rot_corr`` perceives the
        torsions from it (``symmetric_torsions=`` / ``rotation_masks=`` override the perception).
        ``prune_enantiomers=True``: the RMSD stage (only that stage) counts mirror images as duplicates
        (``prune_by_rmsd(..., prune_enantiomers=True)``); its log line then reads "RMSD similarity (mirror images
        included)".
        ``symmetry=`` (a bond graph or a (K, A) table of atom permutations, ``prune_by_rmsd``): the RMSD stage (only that
        stage) counts relabelled copies as duplicates; the MOI stage then runs as a call of its own, and the RMSD log line
        reads "RMSD similarity (K atom permutations)"."""
        from firecode_amd import _lib as L
        from firecode_amd import symmetry as S

        enant = L.check_flag("prune_enantiomers", prune_enantiomers)
        table = S.resolve(symmetry, self.atoms, True)
        S.refuse_with_enantiomers(table, enant)
        rmsd_label = "RMSD similarity (mirror images included)" if enant else "RMSD similarity"
        if table is not None:
            rmsd_label = f"RMSD similarity ({len(table)} atom permutations)"
        log = self.logfunction if verbose else None
        if log is not None:
            log("--> Similarity Processing")
        before = len(self.coords)
        use_en = len(self.energies) == len(self.coords)
        max_dE = 1.0
        fused = moi and rmsd and table is None
        if fused:
            # both stages on ONE upload of the coordinates (fc_prune_similarity): the MOI stage's survivors
            # are gathered on the device for the RMSD stage; same masks and the same two log lines as the
            # stage-by-stage calls of firecode/ensemble.py:205-244
            from firecode_amd.pruner import prune_similarity

            n0, t0 = len(self.coords), perf_counter()
            m_moi, m_both, counts = prune_similarity(self.coords, self.atoms, max_rmsd=max_rmsd,
                                                     energies=self.energies if use_en else None, max_dE=max_dE,
                                                     prune_enantiomers=enant)
            dt = perf_counter() - t0
            if counts[1] < n0 and log is not None:
                log(f"Discarded {n0 - int(counts[1])} candidates for MOI similarity ({int(counts[1])} left, {dt:.3f} s)")
            if counts[2] < counts[1] and log is not None:
                log(f"Discarded {int(counts[1] - counts[2])} candidates for {rmsd_label} ({int(counts[2])} left, {dt:.3f} s)")
            self.coords = self.coords[m_both]
            self.apply_mask(("energies",), m_both)
        if moi and not fused:
            n0, t0 = len(self.coords), perf_counter()
            self.coords, mask = prune_by_moment_of_inertia(
                self.coords, self.atoms, energies=self.energies if use_en else None, max_dE=max_dE)
            self.apply_mask(("energies",), mask)
            if n0 > len(self.coords) and log is not None:
                log(f"Discarded {n0 - len(self.coords)} candidates for MOI similarity "
                    f"({len(self.coords)} left, {perf_counter() - t0:.3f} s)")
        if rmsd and not fused:
            n0, t0 = len(self.coords), perf_counter()
            use_en = len(self.energies) == len(self.coords)
            self.coords, mask = prune_by_rmsd(
                self.coords, self.atoms, max_rmsd, energies=self.energies if use_en else None, max_dE=max_dE,
                prune_enantiomers=enant, symmetry=table)
            self.apply_mask(("energies",), mask)
            if n0 > len(self.coords) and log is not None:
                log(f"Discarded {n0 - len(self.coords)} candidates for {rmsd_label} "
                    f"({len(self.coords)} left, {perf_counter() - t0:.3f} s)")
        if rmsd:
            if rmsd_rot_corr:
                if len(self.coords) <= 1e3:
                    from firecode_amd.pruner import prune_by_rmsd_rot_corr

                    n0, t0 = len(self.coords), perf_counter()
                    if graph is None:
                        from firecode_amd.torsion_perception import graphize

                        graph = graphize(self.atoms, self.coords[0])  # firecode/ensemble.py:250
                    self.coords, mask = prune_by_rmsd_rot_corr(
                        self.coords, self.atoms, graph, max_rmsd=max_rmsd,
                        energies=self.energies if use_en else None, max_dE=max_dE, torsions=symmetric_torsions,
                        rotation_masks=rotation_masks)
                    self.apply_mask(("energies",), mask)
                    if n0 > len(self.coords) and log is not None:
                        log(f"Discarded {n0 - len(self.coords)} candidates for symmetry-corrected RMSD similarity "
                            f"({len(self.coords)} left, {perf_counter() - t0:.3f} s)")
                elif log is not None:
                    log("Skipped rotationally-corrected RMSD pruning (>1k structures)")
        if len(self.coords) == before and log is not None:
            log(f"All structures passed the similarity check.{' ' * 15}")
        if log is not None:
            log("")
