"""What the tests of the ensemble preparation (tests/test_gpu_prep.py) need beside the oracle: the preparation kernel's
LDS arithmetic restated from its constants, the atom selections, the test ensembles in their three placements, the
all-pairs reference of a SELECTED sub-array, and the choice of a threshold that no pair sits on.  Pure NumPy, test
infrastructure: the product never imports it, and the oracle never sees an atom mask -- it is handed ``X[:, sel]``.
tests/test_prep_ref.py checks this module on the CPU, every case of the GPU module included."""

import functools

import numpy as np

from firecode_amd import synthetic as syn
from oracle import cpu_ref as o

import support_ref as R

TOL = 1e-10

# ---------------------------------------------------------------------------------------------------------
# the preparation kernel's branch points (fc_kabsch.hip: k_prep_tile<32>, prep_by_tiles, launch_prep_tiles)
# ---------------------------------------------------------------------------------------------------------
# One workgroup holds PREP_TILE conformers in LDS, each as a row of 3 * A_all doubles plus one double that spreads the
# rows over the banks, then the selection (one int per atom; the launcher sizes it by A_all) and 8 bytes of slack:
#     lds_tile(A_all) = PREP_TILE * (3 * A_all + 1) * 8 + 4 * A_all + 8 = 772 * A_all + 264   bytes
# * above LDS_DEFAULT (64 KB) the launcher has to raise the kernel's dynamic-LDS attribute first:  A_all >= 85
# * the tile kernel runs while lds_tile + LDS_HEADROOM (its static arrays) <= LDS_LIMIT (160 KB):   A_all <= 209
#   beyond, the one-lane-per-conformer kernel k_prep takes over (also whenever FC_PREP_LANES is set).
PREP_TILE = 32
LDS_DEFAULT = 64 * 1024
LDS_LIMIT = 160 * 1024
LDS_HEADROOM = 2048
# the complete alignments of all pairs (rmsd_and_max_all): column tiles of 64 conformers up to 104 selected atoms, of 32
# up to 208, of 16 up to 416 (fc_api_ensemble.cpp: rmsd_and_max_tiled); from 417 selected atoms on k_matrix_exact
TILED_MAX_ATOMS = 416
# the values alone (rmsd_values) keep the 64-column tile: (A4 * 3 * 64 + 64 + 128) * 8 + 488 bytes of LDS, A4 = A rounded
# up to 4, fit LDS_LIMIT up to 104 selected atoms; beyond, the call reports FC_E_LIMIT
VALUES_MAX_ATOMS = 104


def prep_lds_bytes(a_all):
    return PREP_TILE * (3 * a_all + 1) * 8 + 4 * a_all + 8


def prep_raises_lds_attribute(a_all):
    return prep_lds_bytes(a_all) > LDS_DEFAULT


def prep_by_tiles(a_all):
    return prep_lds_bytes(a_all) + LDS_HEADROOM <= LDS_LIMIT


def complete_tile_bytes(a_sel):
    """LDS of the tiled complete-alignment kernel at its narrowest column tile (rmsd_and_max_tiled)."""
    return (((a_sel + 3) // 4 + 1) // 2 * 384 + 16 + 128) * 8 + 1024


def complete_is_tiled(a_sel):
    return complete_tile_bytes(a_sel) <= LDS_LIMIT


def load_tail_is_odd(n, a_all):
    """Whether the last (partial or whole) tile of the 16-byte load path ends on a single double: ``cnt & 1`` with
    cnt = n_here * 3 * A_all, n_here the number of conformers of that tile."""
    n_here = n % PREP_TILE or min(n, PREP_TILE)
    return (n_here * 3 * a_all) % 2 == 1


# ---------------------------------------------------------------------------------------------------------
# atom selections
# ---------------------------------------------------------------------------------------------------------
MASKS = ("none", "drop_first", "drop_last", "every_other", "single", "three", "mod1", "mod2", "mod3")


def atom_mask(kind, a_all, seed=0):
    """Boolean selection over ``a_all`` atoms, or None for "none".  "single": one atom in the middle; "three": the second,
    the middle and the last atom; "modK": a random subset of about half the atoms whose size leaves K modulo 4;
    "nK" (n104, n105, ...): a random subset of exactly K atoms."""
    if kind == "none":
        return None
    m = np.zeros(a_all, dtype=bool)
    if kind == "drop_first":
        m[1:] = True
    elif kind == "drop_last":
        m[:-1] = True
    elif kind == "every_other":
        m[::2] = True
    elif kind == "single":
        m[a_all // 2] = True
    elif kind == "three":
        m[[1, a_all // 2, a_all - 1]] = True
    elif kind.startswith("mod") or kind.startswith("n"):
        if kind.startswith("mod"):
            want = int(kind[3:])
            k = a_all // 2
            k += (want - k) % 4
        else:
            k = int(kind[1:])
        assert 1 <= k <= a_all
        m[np.random.default_rng(1000 + a_all + seed).choice(a_all, size=k, replace=False)] = True
    else:
        raise ValueError(kind)
    return m


def selection(mask, a_all):
    return np.arange(a_all) if mask is None else np.flatnonzero(mask)


# ---------------------------------------------------------------------------------------------------------
# test ensembles
# ---------------------------------------------------------------------------------------------------------
FAR_SHIFT = 1000.0 * np.array([1.0, -0.7, 0.3])
PLACEMENTS = ("centred", "origin", "raw", "far")


def build(a_all, n, kind="clusters", placement="centred", seed=0, duplicate=False):
    """-> (X (n, a_all, 3) C-contiguous float64, center flag for DeviceEnsemble).

    kind       "clusters": ``synthetic_ensemble`` with clusters of three (pairs 0.07 A and ~1.5 A apart: both verdicts of
               a prune occur; beyond 210 atoms its compact form, whose centres need no clash rejection: the walk's take
               minutes there); "blob" / "far250" / "linear": ``support_ref.ensemble`` ("far250" is its "far")
    placement  "centred": as generated (every conformer somewhere else), center=True
               "origin":  center=False; every conformer moved so that its first atom is the origin -- the members of a
                          cluster are then rotated copies of each other ABOUT THE ORIGIN and their uncentred RMSDs stay small
               "raw":     center=False on the coordinates as generated (RMSDs of the size of the translations)
               "far":     center=True, every conformer shifted by 1000 A x (1, -0.7, 0.3)
    duplicate  the last conformer is a copy of the second (the first when n == 2): a pair whose RMSD is 0 (``duplicated``)"""
    if kind == "clusters":
        X = syn.synthetic_ensemble(n, a_all, seed=seed, cluster_size=3, compact=a_all > 210)[0]
    else:
        X = R.ensemble("far" if kind == "far250" else kind, n, a_all, seed=seed)
    X = np.array(X, dtype=np.float64)
    if placement == "origin":
        X = X - X[:, :1]
    elif placement == "far":
        X = X + FAR_SHIFT
    elif placement not in ("centred", "raw"):
        raise ValueError(placement)
    if duplicate and n >= 2:
        X[-1] = X[duplicated(n)]
    return np.ascontiguousarray(X), placement in ("centred", "far")


# ---------------------------------------------------------------------------------------------------------
# the oracle on the selected sub-array
# ---------------------------------------------------------------------------------------------------------
class PairRef:
    """The oracle's values of all pairs i < j of ``Xsel`` (N, A, 3): ``r``, ``d`` (P,), the conditioning bound of the max
    deviation ``bound`` (P,), and the symmetric matrices ``R``, ``D`` (zero diagonal) with ``B`` (bound, zero diagonal)."""

    def __init__(self, Xsel, center, block=2048):
        Xsel = np.asarray(Xsel, dtype=np.float64)
        n = len(Xsel)
        self.n, self.center = n, center
        self.iu, self.ju = np.triu_indices(n, 1)
        P = len(self.iu)
        self.r, self.d, self.bound = np.zeros(P), np.zeros(P), np.zeros(P)
        for s in range(0, P, block):
            i, j = self.iu[s:s + block], self.ju[s:s + block]
            self.r[s:s + block], self.d[s:s + block] = o.rmsd_and_max_batch(Xsel[i], Xsel[j], center=center)
            self.bound[s:s + block] = o.rotation_error_bound_batch(Xsel[i], Xsel[j], center=center)
        self.R, self.D, self.B = (self._square(v) for v in (self.r, self.d, self.bound))

    def _square(self, v):
        M = np.zeros((self.n, self.n))
        M[self.iu, self.ju] = v
        return M + M.T

    def similar(self, thr, max_dev=None):
        """The oracle's similarity matrix (``rmsd_similarity_matrix``'s rule: strict, symmetric, False on the diagonal)."""
        S = (self.R < thr) & (self.D < (2 * thr if max_dev is None else max_dev))
        np.fill_diagonal(S, False)
        return S


def split_threshold(r):
    """A threshold in the widest gap of the middle half of the pair RMSDs ``r`` -> (threshold, half-width of the gap).
    Fewer than four pairs: between the only values there are (half-width from the nearest)."""
    r = np.sort(np.asarray(r, dtype=np.float64))
    if len(r) < 4:
        if len(r) == 0:
            return 0.5, np.inf
        thr = 0.5 * (r[0] + r[-1]) if r[-1] > r[0] else 1.5 * r[0] + 0.25
        return float(thr), float(np.abs(r - thr).min())
    mid = r[len(r) // 4: len(r) - len(r) // 4]
    k = int(np.argmax(np.diff(mid)))
    return float(0.5 * (mid[k] + mid[k + 1])), float(0.5 * (mid[k + 1] - mid[k]))


DUPLICATE_AT = 4  # position of the pair (last conformer, the one ``build(duplicate=True)`` copied) in ``pair_list``


def duplicated(n):
    """The conformer ``build(duplicate=True)`` copies into the last one."""
    return max(min(1, n - 2), 0)


def pair_list(n, rng, length=257):
    """``length`` index pairs over n conformers in no order: (0, 0), (n-1, n-1), (n-1, 0) twice, (n-1, duplicated(n)),
    then random ones -- i > j, i == j and repeated pairs all occur."""
    i = rng.integers(0, n, size=length)
    j = rng.integers(0, n, size=length)
    i[:5] = (0, n - 1, n - 1, n - 1, n - 1)
    j[:5] = (0, n - 1, 0, 0, duplicated(n))
    return i.astype(np.int64), j.astype(np.int64)


def rotation_is_unique(kind, a_sel, center):
    """Whether the optimal rotation of a pair is unique by the structures' kind: not for atoms on a line, for one
    atom, or for two atoms about their centroid (two atoms and the origin span a plane: unique).  Where it is not, every
    ``rotation_error_bound_batch`` is infinite and the max deviation is not compared."""
    return kind != "linear" and a_sel > (2 if center else 1)


def case_threshold(ref, all_zero=False):
    """The RMSD threshold of a case: in the widest gap of the middle half of the oracle's pair RMSDs, asserted to be more
    than 1e-6 from every pair's RMSD, with the doubled threshold as far from the max deviation of every pair below it,
    and -- from four pairs on -- with both verdicts among the pairs.  ``all_zero`` (one selected atom about itself: every
    value is exactly 0): 0.5, everything similar."""
    if all_zero:
        assert not ref.r.any() and not ref.d.any()
        return 0.5
    thr, half = split_threshold(ref.r)
    assert half > 1e-6
    assert np.abs(ref.d[ref.r < thr] - 2 * thr).min(initial=1.0) > 1e-6
    if len(ref.r) >= 4:
        assert 0 < np.triu(ref.similar(thr), 1).sum() < len(ref.r)
    return thr


def check_bounds(ref, kind, a_sel, center):
    """At least 95 % of a case's pairs have a conditioning bound below the tolerance itself -- or, where the rotation
    is not unique by construction, none has a finite one."""
    if not rotation_is_unique(kind, a_sel, center):
        assert np.isinf(ref.bound).all()
    elif len(ref.bound):
        assert (ref.bound < TOL).mean() >= 0.95


def far_self_agreement(X, sel, ref):
    """The oracle alone, evaluated with the atoms in reverse order, against itself on a "far" case -> (largest RMSD
    difference, largest max-deviation difference over the pairs whose bound is below the tolerance).  Asserted a
    decimal order below the bars of the comparison (measured: 2e-15 and 2.2e-12)."""
    back = PairRef(X[:, sel[::-1]], ref.center)
    ok = ref.bound < TOL
    dr, dd = np.abs(back.r - ref.r).max(initial=0.0), np.abs(back.d - ref.d)[ok].max(initial=0.0)
    assert dr < 1e-13 and dd < 1e-11
    return float(dr), float(dd)


@functools.lru_cache(maxsize=None)
def case(a_all, n, kind, placement, duplicate, mask_kind):
    """One case's input and reference, computed once and shared read-only: (X, center, mask, sel, ref)."""
    X, center = build(a_all, n, kind, placement, seed=case_seed(a_all, n, mask_kind), duplicate=duplicate)
    mask = atom_mask(mask_kind, a_all)
    sel = selection(mask, a_all)
    ref = PairRef(X[:, sel], center)
    for arr in (X, ref.r, ref.d, ref.bound, ref.R, ref.D, ref.B):
        arr.setflags(write=False)
    return X, center, mask, sel, ref


# ---------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_prep.py
# ---------------------------------------------------------------------------------------------------------
# (A_all, N, kind, placement, duplicate) with no atom mask.  Which case reaches which branch of the preparation:
#   aligned-load tail (cnt & 1: odd conformer count of the last tile x odd A_all)
#                        (1, 33) (3, 63) (5, 33) (5, 97) (7, 31) (7, 65) (33, 33) (33, 63) (33, 129) (85, 33) (85, 65) (85, 97)
#                        (209, 33) (209, 129); the even side: every case with an even A_all or N in (2, 64)
#   partial last tile    every N that is no multiple of 32; whole tiles only: N = 64
#   padding columns      every N but 64 (Npad = 64, 128 or 192 > N); none: N = 64
#   padding rows         A_all = 1, 2, 3, 5, 7, 33, 85, 209, 210, 417 (A % 4 != 0); none: 84
#   more than 64 KB LDS  84 below, 85 and 209 above (the tile kernel with the raised attribute)
#   tile / lane switch   209 tile kernel, 210 and 417 lane kernel
#   k_matrix_exact       417 unmasked: two column tiles (N = 97) and three (N = 129), the diagonal skip in both
BASE_CASES = [
    (1, 2, "clusters", "raw", False), (1, 33, "clusters", "raw", False), (1, 64, "clusters", "centred", False),
    (2, 1, "clusters", "centred", False), (2, 31, "clusters", "centred", False), (2, 65, "clusters", "raw", True),
    (3, 2, "clusters", "centred", True), (3, 63, "clusters", "origin", False), (3, 129, "clusters", "centred", False),
    (5, 1, "clusters", "origin", False), (5, 33, "clusters", "far", False), (5, 97, "clusters", "origin", True),
    (7, 31, "clusters", "centred", False), (7, 64, "linear", "centred", False), (7, 65, "clusters", "origin", False),
    (33, 33, "clusters", "origin", False), (33, 63, "blob", "centred", False), (33, 129, "clusters", "far", True),
    (84, 31, "clusters", "origin", False), (84, 64, "clusters", "centred", True),
    (85, 33, "clusters", "centred", False), (85, 65, "far250", "centred", False), (85, 97, "clusters", "origin", True),
    (209, 33, "clusters", "far", False), (209, 64, "clusters", "origin", False), (209, 129, "clusters", "centred", True),
    (210, 31, "linear", "centred", False), (210, 65, "clusters", "origin", True), (210, 97, "clusters", "centred", False),
    (417, 2, "clusters", "origin", False), (417, 97, "clusters", "centred", True), (417, 129, "clusters", "origin", False),
]

# (A_all, N) of the masked cases: each mask of MASKS but "none" at each of these, centred and about the origin; N gives an
# odd last tile at the two odd atom counts, a partial tile and padding columns at all three
MASK_SHAPES = [(33, 33), (85, 65), (210, 97)]
# a selection whose size crosses the 64- / 32-column switch of the complete alignments while A_all stays: 104, then 105
BOUNDARY_MASKS = [(210, 97, "n104"), (210, 97, "n105")]
# the "far" placement under a mask, at each shape
FAR_MASKED = [(33, 33, "every_other"), (85, 65, "mod3"), (210, 97, "drop_first")]


def masked_cases():
    out = []
    for a_all, n in MASK_SHAPES:
        for mask in MASKS[1:]:
            for placement in ("centred", "origin"):
                out.append((a_all, n, mask, placement))
    out += [(a, n, m, p) for a, n, m in BOUNDARY_MASKS for p in ("centred", "origin")]
    out += [(a, n, m, "far") for a, n, m in FAR_MASKED]
    return out


def case_seed(a_all, n, mask="none"):
    return 7000 + 13 * a_all + n + 101 * (MASKS + ("n104", "n105")).index(mask)


# the cases built once by each preparation kernel (A_all <= 209: beyond, both runs are the lane kernel)
TWIN_CASES = [
    (5, 33, "none", "far"), (7, 65, "none", "origin"), (33, 33, "none", "centred"), (33, 33, "every_other", "origin"),
    (33, 129, "mod3", "far"), (84, 64, "none", "centred"), (85, 65, "three", "centred"), (85, 97, "drop_last", "origin"),
    (209, 33, "none", "far"), (209, 129, "mod1", "centred"),
]


# ---------------------------------------------------------------------------------------------------------
# the gather of prune_similarity
# ---------------------------------------------------------------------------------------------------------
def gather_ensemble(a_all, n):
    """(X, atoms) for the fused MOI + RMSD prune: clusters of five compact structures with hydrogens in the atom list;
    two of every five conformers 2 % larger -- 4 % in the moments, which the MOI stage (1 %) tells apart, 0.1 A in the
    RMSD, which the stage behind it does not.  The MOI stage removes some conformers, the RMSD stage some of the rest."""
    X = syn.synthetic_ensemble(n, a_all, seed=900 + a_all, cluster_size=5, compact=True)[0]
    grow = np.arange(n) % 5 < 2
    X[grow] = X[grow] * 1.02
    atoms = np.array((["C", "H", "N", "O", "H"] * (a_all // 5 + 1))[:a_all])
    return np.ascontiguousarray(X), atoms


def gather_reference(X, atoms, thr):
    """The oracle's two stages one after the other -> (mask after MOI, mask after both), in the caller's order."""
    _, m1 = o.prune_by_moment_of_inertia(X, atoms)
    S, _, _ = o.rmsd_similarity_matrix(X[m1], atoms, thr)
    both = np.zeros(len(X), dtype=bool)
    both[np.flatnonzero(m1)[o.greedy_prune_from_matrix(S)]] = True
    return m1, both
