"""References of the embed family -- per-molecule pose transforms, the pre-transformed tables, the all-pose clash
grid with its counts contract, the sequential in-group de-duplication and the sequential torsion-fingerprint
novelty filter of the string embed -- written from the operations' definitions, plus the inputs of the GPU tests
(tests/test_gpu_embed_kernels.py) so that tests/test_embed_ref.py can check, without a GPU, the conditions those
tests rely on for exactly the seeds and shapes they use.  Test infrastructure: it never imports the product.

Three kinds of reference live here:

* **bit-level contracts.**  The tables are rebuilt with the kernel's literal expression
  ``((r0*x0 + r1*x1) + r2*x2) + t0`` elementwise in float64 (no ``@``, no einsum: nothing may re-associate or
  fuse), the distances go through ``scipy.spatial.distance.cdist`` and are compared with ``< thresh``: pass flags
  and counts are compared for equality.
* **sequential walks with an exclusion margin.**  The de-duplication and the novelty filter are chaotic: one
  flipped comparison changes everything behind it.  Their references record the smallest distance of any
  comparison they made from the threshold(s); a group (a case) closer than the margin is *undecidable* and the
  tests assert that there is none.
* **oracle restatements.**  The per-molecule transforms are ``oracle.cpu_ref.bimol_pose_transforms`` called
  once per (conformer, orientation, angle)."""

import numpy as np
from scipy.spatial.distance import cdist

from oracle import cpu_ref as o
from support_ref import EXTENDED, LD

TOL = 1e-10            # the project's coordinate tolerance
DEDUPE_MARGIN = 1e-9   # Angstrom: exclusion margin of the in-group de-duplication (not a pass criterion)
TFD_MARGIN = 1e-7      # degrees: exclusion margin of the string embed's novelty filter (not a pass criterion)
MI355X_CUS = 256       # the CPU tests build the device-dependent cases for this many compute units


# ---------------------------------------------------------------------------------------------------------
# per-molecule transforms: the oracle, one (conformer, orientation, angle) at a time
# ---------------------------------------------------------------------------------------------------------
_OTHER = (np.array([[0.5, 0.25, 0.0], [1.0, 2.0, 3.0]]), np.array([0]), (np.array([1.0, 2.0, 3.0]), np.zeros(3)))


def mol_transforms(coords, reactive, pivots, mol, angles):
    """R (n, 2, na, 3, 3), t (n, 2, na, 3) of molecule ``mol`` (0: first, 1: second of the pair).  The transform
    of a molecule depends on nothing of the other one (polygonize() gives each its own pivot length), so the
    other slot of the oracle call holds a fixed stand-in."""
    coords, angles = np.asarray(coords, dtype=np.float64), np.asarray(angles, dtype=np.float64)
    n, na = len(coords), len(angles)
    R, t = np.empty((n, 2, na, 3, 3)), np.empty((n, 2, na, 3))
    for c in range(n):
        me = (coords[c], np.asarray(reactive), (pivots[c][0], pivots[c][1]))
        a, b = (me, _OTHER) if mol == 0 else (_OTHER, me)
        for ori in (0, 1):
            for i, ang in enumerate(angles):
                out = o.bimol_pose_transforms(a[0], b[0], a[1], b[1], a[2], b[2], (ang, ang), ori)
                R[c, ori, i], t[c, ori, i] = out[2 * mol], out[2 * mol + 1]
    return R, t


def tables(coords, R, t):
    """X (n, 2, na, A, 3): every pre-transformed structure, by the kernel's literal expression."""
    x = np.asarray(coords, dtype=np.float64)[:, None, None, :, :]
    out = np.empty(R.shape[:3] + (x.shape[3], 3))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(3):
            r0, r1, r2 = (R[:, :, :, k, j, None] for j in range(3))
            out[..., k] = ((r0 * x[..., 0] + r1 * x[..., 1]) + r2 * x[..., 2]) + t[:, :, :, k, None]
    return out


# ---------------------------------------------------------------------------------------------------------
# pose grid: pass flags and counts
# ---------------------------------------------------------------------------------------------------------
def grid_distances(X1, X2):
    """per orientation, ONE cdist over the flattened tables: D[o] of shape (n2, na2, A2, n1, na1, A1)"""
    n1, _, na1, A1, _ = X1.shape
    n2, _, na2, A2, _ = X2.shape
    with np.errstate(invalid="ignore", over="ignore"):
        return [cdist(X2[:, ori].reshape(-1, 3), X1[:, ori].reshape(-1, 3)).reshape(n2, na2, A2, n1, na1, A1)
                for ori in (0, 1)]


def grid_from_distances(D, thresh, max_clashes):
    """pass, counts (n2, n1, 2, na2, na1).  counts contract: molecule-2 atoms b in order, the whole row b (all
    molecule-1 atoms) is added while the running count is <= max_clashes, then counting stops -- the cumulative
    sum over b cut at the first index where it exceeds max_clashes.  NaN and inf distances never count."""
    n2, na2, _, n1, na1, _ = D[0].shape
    counts = np.empty((n2, n1, 2, na2, na1), dtype=np.int32)
    for ori in (0, 1):
        with np.errstate(invalid="ignore"):
            rows = (D[ori] < thresh).sum(axis=-1)             # (n2, na2, A2, n1, na1)
        cum = np.cumsum(rows, axis=2)
        over = cum > max_clashes
        first = np.where(over.any(axis=2), over.argmax(axis=2), cum.shape[2] - 1)
        cnt = np.take_along_axis(cum, first[:, :, None], axis=2)[:, :, 0]   # (n2, na2, n1, na1)
        counts[:, :, ori] = cnt.transpose(0, 2, 1, 3)
    return counts <= max_clashes, counts


def grid_reference(X1, X2, thresh, max_clashes):
    return grid_from_distances(grid_distances(X1, X2), thresh, max_clashes)


def grid_literal(X1, X2, thresh, max_clashes):
    """the same contract as plain loops (tiny shapes only): what grid_reference is checked against"""
    n1, _, na1, A1, _ = X1.shape
    n2, _, na2, A2, _ = X2.shape
    counts = np.zeros((n2, n1, 2, na2, na1), dtype=np.int32)
    for c2 in range(n2):
        for c1 in range(n1):
            for ori in (0, 1):
                for a2 in range(na2):
                    for a1 in range(na1):
                        cnt = 0
                        for b in range(A2):
                            if cnt > max_clashes:
                                break
                            with np.errstate(invalid="ignore"):
                                cnt += int(np.count_nonzero(cdist(X2[c2, ori, a2, b][None], X1[c1, ori, a1]) < thresh))
                        counts[c2, c1, ori, a2, a1] = cnt
    return counts <= max_clashes, counts


def pose_index(n1, n2, na1, na2, c2, c1, ori, a2, a1):
    return ((c2 * n1 + c1) * 2 + ori) * (na1 * na2) + a2 * na1 + a1


# ---------------------------------------------------------------------------------------------------------
# in-group de-duplication
# ---------------------------------------------------------------------------------------------------------
def kabsch_rmsd_max(p, Q):
    """(rmsd, maxdev) of p (A, 3) against each of Q (K, A, 3) after the best proper rotation of Q[k] about the
    origin (no centring): covariance B = p^T q, B = u s v^T, R = u diag(1, 1, det(u v^T)) v^T.  Covariance and
    residuals are accumulated in extended precision where the platform has it; the 3x3 SVD is float64."""
    acc = LD if EXTENDED else np.float64
    pl, Ql = np.asarray(p, dtype=acc), np.asarray(Q, dtype=acc)
    B = (pl[None, :, :, None] * Ql[:, :, None, :]).sum(axis=1).astype(np.float64)
    u, _, vh = np.linalg.svd(B)
    flip = np.linalg.det(u @ vh) < 0
    u[flip, :, -1] *= -1.0
    M = (u @ vh).astype(acc)
    diff = pl[None] - (M[:, None, :, :] * Ql[:, :, None, :]).sum(axis=-1)
    sq = (diff * diff).sum(axis=-1)
    return np.sqrt(sq.sum(axis=-1) / pl.shape[0]).astype(np.float64), np.sqrt(sq.max(axis=-1)).astype(np.float64)


def dedupe_reference(X1, X2, ok, thr):
    """The sequential rule: a group (c2, c1, o) is walked in angle order (a2 slowest); a clash-free pose is kept
    iff no kept pose of the group has rmsd < thr and maxdev < 2*thr to it.
    -> dict: ``acc`` like ok; ``margin`` (n2, n1, 2): smallest |rmsd - thr| or |maxdev - 2 thr| over every
    comparison made (inf where none was); ``first_hit`` like ok: kept index of the first hit of a rejected pose,
    -1 elsewhere; ``n_kept`` (n2, n1, 2); ``values``: (rmsd, maxdev) of all comparisons in walk order, (K, 2)."""
    n2, n1, _, na2, na1 = ok.shape
    A = X1.shape[3] + X2.shape[3]
    acc = np.zeros_like(ok, dtype=bool)
    margin = np.full((n2, n1, 2), np.inf)
    first_hit = np.full(ok.shape, -1, dtype=np.int64)
    n_kept = np.zeros((n2, n1, 2), dtype=np.int64)
    values = []
    kept = np.empty((na1 * na2, A, 3))
    for c2 in range(n2):
        for c1 in range(n1):
            for ori in (0, 1):
                nk = 0
                for a2, a1 in zip(*np.nonzero(ok[c2, c1, ori])):
                    pose = np.concatenate([X1[c1, ori, a1], X2[c2, ori, a2]])
                    hit = np.zeros(0, dtype=bool)
                    if nk:
                        r, m = kabsch_rmsd_max(pose, kept[:nk])
                        values.append(np.stack([r, m], axis=1))
                        margin[c2, c1, ori] = min(margin[c2, c1, ori], np.abs(r - thr).min(), np.abs(m - 2 * thr).min())
                        hit = (r < thr) & (m < 2 * thr)
                    if hit.any():
                        first_hit[c2, c1, ori, a2, a1] = int(hit.argmax())
                    else:
                        kept[nk] = pose
                        nk += 1
                        acc[c2, c1, ori, a2, a1] = True
                n_kept[c2, c1, ori] = nk
    return {"acc": acc, "margin": margin, "first_hit": first_hit, "n_kept": n_kept,
            "values": np.concatenate(values) if values else np.zeros((0, 2))}


# ---------------------------------------------------------------------------------------------------------
# string embed: fingerprints of the poses and the sequential novelty filter
# ---------------------------------------------------------------------------------------------------------
def string_transforms(centers1, orbvecs1, centers2, orbvecs2, angles):
    """R2 (P, 3, 3), t2 (P, 3), c1, c2 (P,) in the reference's loop order, by the oracle's own functions"""
    n1, K1 = centers1.shape[:2]
    n2, K2 = centers2.shape[:2]
    R, t, i1, i2 = [], [], [], []
    for c1, c2 in o.cartesian_product(np.arange(n1), np.arange(n2)):
        for k1, k2 in o.cartesian_product(np.arange(K1), np.arange(K2)):
            for angle in angles:
                rot = o.rotation_matrix_from_vectors(orbvecs2[c2, k2], -orbvecs1[c1, k1])
                if angle != 0:
                    rot = o.rot_mat_from_pointer(orbvecs1[c1, k1], angle) @ rot
                R.append(rot)
                t.append(centers1[c1, k1] - rot @ centers2[c2, k2])
                i1.append(c1)
                i2.append(c2)
    return np.array(R), np.array(t), np.array(i1), np.array(i2)


def string_pose_index(n1, n2, K1, K2, nA, c1, c2, k1, k2, ia):
    return ((c2 * n1 + c1) * (K1 * K2) + (k2 * K1 + k1)) * nA + ia


def _dihedrals(p):
    """p (..., 4, 3) -> degrees in (-180, 180], the published one-sqrt form of the dihedral"""
    b0 = -1.0 * (p[..., 1, :] - p[..., 0, :])
    b1 = p[..., 2, :] - p[..., 1, :]
    b2 = p[..., 3, :] - p[..., 2, :]
    b1 = b1 / np.sqrt((b1 * b1).sum(axis=-1))[..., None]
    v = b0 - (b0 * b1).sum(axis=-1)[..., None] * b1
    w = b2 - (b2 * b1).sum(axis=-1)[..., None] * b1
    return np.degrees(np.arctan2((np.cross(b1, v) * w).sum(axis=-1), (v * w).sum(axis=-1)))


def string_fingerprints(m1, m2, c1, c2, R2, t2, quads):
    """tf (P, Q): torsion fingerprint of every pose (molecule 1 as it is, molecule 2 through R2, t2), float64"""
    A1 = m1.shape[1]
    x2 = m2[c2]                                                            # (P, A2, 3)
    moved = np.empty_like(x2)
    for k in range(3):
        moved[..., k] = ((R2[:, k, 0, None] * x2[..., 0] + R2[:, k, 1, None] * x2[..., 1])
                         + R2[:, k, 2, None] * x2[..., 2]) + t2[:, k, None]
    pose = np.concatenate([m1[c1], moved], axis=1)                         # (P, A1 + A2, 3)
    assert pose.shape[1] == A1 + m2.shape[1]
    return _dihedrals(pose[:, np.asarray(quads).reshape(-1, 4)])


def string_filter(tf, ok, thresh, chunk=256):
    """The novelty filter over the poses in order: a clash-free pose is kept iff no fingerprint kept so far has
    sum_q min(|d|, 360 - |d|) < thresh to its own.
    -> dict: ``acc`` (P,); ``margin``: smallest |sum - thresh| over every comparison made; ``kept_before`` /
    ``kept_in``: per chunk of ``chunk`` poses, fingerprints kept before it / inside it; ``early`` (P,): the pose
    passed the clash test and is similar to a fingerprint kept BEFORE its chunk."""
    P = len(tf)
    acc, early = np.zeros(P, dtype=bool), np.zeros(P, dtype=bool)
    cache = np.empty_like(tf)
    nk, margin = 0, np.inf
    kept_before, kept_in = [], []
    for p in range(P):
        if p % chunk == 0:
            kept_before.append(nk)
            kept_in.append(0)
        if not ok[p]:
            continue
        d = np.abs(tf[p] - cache[:nk])
        d = np.abs(d - (d > 180) * 360)
        s = d.sum(axis=1)
        if nk:
            margin = min(margin, np.abs(s - thresh).min())
        early[p] = bool((s[:kept_before[-1]] < thresh).any())
        if not (s < thresh).any():
            cache[nk] = tf[p]
            nk += 1
            kept_in[-1] += 1
            acc[p] = True
    return {"acc": acc, "margin": margin, "kept_before": kept_before, "kept_in": kept_in, "early": early}


# ---------------------------------------------------------------------------------------------------------
# inputs of the GPU tests
# ---------------------------------------------------------------------------------------------------------
def bimol_case(seed, n1, n2, A1, A2, nr1=2, nr2=1, scale=1.8, spread=1.0):
    """two small random ensembles with one pivot per conformer: two pseudo-orbital centres near the reactive
    atoms (indices 0 and A-1), pushed outwards.  -> m1, r1, pv1, m2, r2, pv2"""
    rng = np.random.default_rng(seed)

    def mol(n, A, nr):
        m = rng.normal(scale=scale, size=(n, A, 3))
        r = np.array([0, A - 1][:min(nr, A)])
        pv = np.empty((n, 2, 3))
        for c in range(n):
            pv[c, 0] = m[c, r[0]] * 1.6 + rng.normal(scale=0.3, size=3)
            pv[c, 1] = m[c, r[-1]] * 1.6 + rng.normal(scale=0.3, size=3) + (0 if len(r) == 2 else 1.2)
        return m, r, pv * spread

    m1, r1, pv1 = mol(n1, A1, nr1)
    m2, r2, pv2 = mol(n2, A2, nr2)
    return m1, r1, pv1, m2, r2, pv2


def stride_n(n_cu):
    """smallest n1 = n2 whose 2 n^2 groups exceed the 4 * (8 * n_cu) the de-duplication launch covers at once"""
    n = 1
    while 2 * n * n <= 32 * n_cu:
        n += 1
    return n


ANG12 = np.arange(12) * 27.5 - 150.0

# name -> (seed, n1, n2, A1, A2, angles1, angles2, clash thresh, rmsd_thr)
_DEDUPE = {
    "kept": (301, 1, 2, 5, 4, ANG12, ANG12 + 3.0, 0.05, 0.02),
    "late_hit": (302, 2, 1, 4, 5, ANG12, np.where(np.arange(12) == 11, (ANG12 + 3.0)[6], ANG12 + 3.0), 0.05, 0.02),
    "most_rejected": (303, 2, 2, 6, 5, ANG12, ANG12 + 3.0, 0.6, 2.5),
    "all_clash": (304, 2, 2, 6, 5, ANG12[:5], ANG12[:4], 1.0e3, 1.0),
    "lds_limit": (306, 1, 1, 3, 2, np.linspace(-90.0, 90.0, 64), np.linspace(-80.0, 85.0, 64), 0.3, 1.0e3),
}
DEDUPE_CASES = tuple(_DEDUPE) + ("stride",)


def dedupe_case(name, n_cu=MI355X_CUS):
    """-> dict(m1, r1, pv1, m2, r2, pv2, angles1, angles2, thresh, rmsd_thr)"""
    if name == "stride":
        n = stride_n(n_cu)
        seed, n1, n2, A1, A2, a1, a2, thresh, thr = 305, n, n, 3, 2, np.array([-30.0, 40.0]), np.array([-20.0, 55.0]), 2.5, 1.5
    else:
        seed, n1, n2, A1, A2, a1, a2, thresh, thr = _DEDUPE[name]
    m1, r1, pv1, m2, r2, pv2 = bimol_case(seed, n1, n2, A1, A2, nr1=2, nr2=1)
    return {"m1": m1, "r1": r1, "pv1": pv1, "m2": m2, "r2": r2, "pv2": pv2, "angles1": np.asarray(a1, dtype=np.float64),
            "angles2": np.asarray(a2, dtype=np.float64), "thresh": thresh, "rmsd_thr": thr}


def dedupe_tables(case, transforms=mol_transforms):
    """the two tables of a case from ``transforms(coords, reactive, pivots, mol, angles) -> R, t``"""
    R1, t1 = transforms(case["m1"], case["r1"], case["pv1"], 0, case["angles1"])
    R2, t2 = transforms(case["m2"], case["r2"], case["pv2"], 1, case["angles2"])
    return tables(case["m1"], R1, t1), tables(case["m2"], R2, t2)


# name -> (seed, n1, n2, K1, K2, nA, Q, clash thresh, tfd_thresh, m1 conformer that repeats conformer 0 or None)
_STRING = {
    "P255": (401, 3, 5, 1, 1, 17, 4, 2.2, 0.5, None),
    "P256": (402, 2, 4, 2, 2, 8, 4, 2.2, 0.5, None),
    "P257": (403, 1, 1, 1, 1, 257, 4, 2.2, 0.05, None),
    "P700": (404, 5, 2, 2, 1, 35, 4, 3.6, 0.5, 3),
    "Q1": (411, 3, 2, 1, 1, 50, 1, 2.2, 0.5, None),
    "Q7": (412, 3, 2, 1, 1, 50, 7, 2.2, 0.5, 2),
    "Q8": (413, 3, 2, 1, 1, 50, 8, 2.2, 0.5, 2),
    "Q9": (414, 3, 2, 1, 1, 50, 9, 2.2, 0.5, 2),
    "Q128": (415, 3, 2, 1, 1, 50, 128, 2.2, 0.5, 2),
}
STRING_CASES = tuple(_STRING)
STRING_A1, STRING_A2 = 6, 5


def string_case(name):
    """-> dict(m1, c1, v1, m2, c2, v2, angles, quads, thresh, tfd_thresh): molecule 1 of 6 atoms (reactive atom
    2), molecule 2 of 5 (reactive atom 3); the first quadruplets straddle the A1 - 1 | A1 boundary, lie entirely
    in molecule 1 and entirely in molecule 2, the others are random"""
    seed, n1, n2, K1, K2, nA, Q, thresh, tfd, dup = _STRING[name]
    rng = np.random.default_rng(seed)
    A1, A2, ra, rb = STRING_A1, STRING_A2, 2, 3
    m1 = rng.normal(scale=1.5, size=(n1, A1, 3))
    m2 = rng.normal(scale=1.5, size=(n2, A2, 3))
    if dup is not None:
        m1[dup] = m1[0]
    f1, f2 = 1.7 + 0.4 * np.arange(K1), 1.7 - 2.6 * np.arange(K2)
    c1 = m1[:, [ra]] * f1[None, :, None] + rng.normal(scale=0.2, size=(n1, K1, 3))
    c2 = m2[:, [rb]] * f2[None, :, None] + rng.normal(scale=0.2, size=(n2, K2, 3))
    if dup is not None:
        c1[dup] = c1[0]
    v1, v2 = c1 - m1[:, [ra]], c2 - m2[:, [rb]]
    fixed = [[A1 - 2, A1 - 1, A1, A1 + 1], [0, A1 - 1, A1, A1 + A2 - 1], [0, 1, 2, 3], [A1, A1 + 1, A1 + 2, A1 + 4],
             [1, ra, A1 + rb, A1]]
    quads = fixed[:Q] + [list(rng.choice(A1 + A2, 4, replace=False)) for _ in range(Q - len(fixed))]
    return {"m1": m1, "c1": c1, "v1": v1, "m2": m2, "c2": c2, "v2": v2, "angles": np.arange(nA) * (360.0 / nA),
            "quads": np.array(quads, dtype=np.int64), "thresh": thresh, "tfd_thresh": tfd}


def string_clash_pass(case, R2, t2, i1, i2):
    """clash verdict of every pose, as compenetration_check does it: no pair of cdist(molecule 2, molecule 1)
    below thresh"""
    m1, m2 = case["m1"], case["m2"]
    ok = np.empty(len(R2), dtype=bool)
    for p in range(len(R2)):
        ok[p] = not (cdist((R2[p] @ m2[i2[p]].T).T + t2[p], m1[i1[p]]) < case["thresh"]).any()
    return ok


def special_mols():
    """name -> (coords (n, A, 3), reactive, pivots (n, 2, 3)): inputs of the alignment that random numbers do
    not reach.  All coordinates are dyadic, so the equalities below hold exactly in floating point.
    * degenerate1 / degenerate2: conformer 1 has the mean of its reactive atom(s), (2, 1, 1), exactly on the
      midpoint of its pivot: the molecule direction is replaced by the midpoint itself.
    * parallel: one reactive atom at the origin, pivot = start - end = 2 d and midpoint - atom = 2 d: the two
      vectors the alignment sees are parallel and its covariance has rank one.
    * antiparallel_x: the pivot points along -x, the molecule direction lies in the y-z plane: a 180-degree
      alignment for orientation 0."""
    generic = np.array([[0.5, -1.25, 2.0], [1.5, 0.75, -0.5], [-2.0, 0.25, 1.0]])
    gpv = np.array([[1.0, -2.0, 3.5], [2.5, 1.0, -1.0]])
    deg2 = np.array([[1.0, 2.0, 0.5], [0.25, -1.5, 2.0], [3.0, 0.0, 1.5]])
    deg1 = np.array([[2.0, 1.0, 1.0], [0.25, -1.5, 2.0], [3.0, 0.5, 1.5]])
    dpv = np.array([[2.5, 1.25, 1.0], [1.5, 0.75, 1.0]])
    d = np.array([1.0, 0.5, 0.25])
    par = np.array([[0.0, 0.0, 0.0], [1.5, -0.5, 2.0], [-1.0, 0.75, 0.5]])
    anti = np.array([[0.0, -1.0, 0.25], [1.5, -0.5, 2.0], [-1.0, 0.75, 0.5]])
    return {
        "degenerate2": (np.array([generic, deg2]), np.array([0, 2]), np.array([gpv, dpv])),
        "degenerate1": (np.array([generic, deg1]), np.array([0]), np.array([gpv, dpv])),
        "parallel": (np.array([par]), np.array([0]), np.array([[3 * d, d]])),
        "antiparallel_x": (np.array([anti]), np.array([0]), np.array([[[-1.0, 0.5, 0.0], [1.0, 0.5, 0.0]]])),
    }
