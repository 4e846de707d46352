"""High-precision NumPy / SciPy references of the "second tier" operations -- clash counts, rigid poses, the
fitness error, moments of inertia and the MOI similarity rule -- written from the operations' definitions, not
from the kernels, plus the generator of the test ensembles.  Test infrastructure: the product never imports it.

Two kinds of reference live here:

* **bit-level contracts.**  The clash counts go through ``scipy.spatial.distance.cdist`` exactly as
  ``oracle.cpu_ref.count_clashes`` / ``compenetration_check`` do; the kernels write cdist's expression literally
  (no fused multiply-add), so counts and verdicts are compared for equality.
* **extended precision.**  Moments, fitness errors and rototranslated coordinates are evaluated in
  ``np.longdouble`` (64-bit significand here; ``EXTENDED`` says whether the platform has more than a double),
  so that the reference's own rounding is three decimal orders below the float64 tolerances of the tests."""

import numpy as np
from scipy.spatial.distance import cdist

LD = np.longdouble
EXTENDED = np.finfo(LD).eps < np.finfo(np.float64).eps
EPS = 2.0 ** -52


# ---------------------------------------------------------------------------------------------------------
# clash family: cdist, literal
# ---------------------------------------------------------------------------------------------------------
def self_count(x, lo=0.0, hi=0.5, d=None):
    """count_clashes with its two bounds as parameters: ordered pairs with lo < d < hi.
    ``d``: cdist(x, x) when the caller already holds it (every function below; an element of cdist(x[r], x[c])
    is the same expression on the same two rows as that element of cdist(x, x), so a block of ``d`` has its bits)."""
    d = cdist(x, x) if d is None else d
    return int(np.count_nonzero((d < hi) & (d > lo)))


def fragment_bounds(n_atoms, ids):
    """[start, end) of each fragment by the reference's slicing: the last fragment takes the rest, whatever its
    listed length, and a slice that starts beyond the end is empty."""
    ids = [int(i) for i in ids]
    cuts = [0, min(ids[0], n_atoms)] if len(ids) == 2 else [0, min(ids[0], n_atoms), min(ids[0] + ids[1], n_atoms)]
    return list(zip(cuts, cuts[1:] + [n_atoms]))


def _block(x, d, rows, cols):
    if d is not None:
        return d[rows[0]:rows[1], cols[0]:cols[1]]
    a, b = x[rows[0]:rows[1]], x[cols[0]:cols[1]]
    return cdist(a, b) if len(a) and len(b) else np.zeros((len(a), len(b)))


def fragment_count(x, ids, thresh, d=None):
    """Two fragments: pairs of cdist(m2, m1) < thresh.  Three: pairs <= thresh summed over (m2, m1), (m3, m2),
    (m1, m3).  The reference's early exits only shorten the sum: its verdict is ``count <= max_clashes``."""
    f = fragment_bounds(len(x), ids)
    if len(f) == 2:
        return int(np.count_nonzero(_block(x, d, f[1], f[0]) < thresh))
    return int(sum(np.count_nonzero(_block(x, d, r, c) <= thresh) for r, c in ((f[1], f[0]), (f[2], f[1]), (f[0], f[2]))))


def graph_count(x, adj, thresh, d=None):
    """Ordered, off-diagonal, non-bonded pairs with d < thresh; adj (A, A) boolean adjacency."""
    hit = (cdist(x, x) if d is None else d) < thresh
    np.fill_diagonal(hit, False)
    return int(np.count_nonzero(hit & ~np.asarray(adj, dtype=bool)))


def adjacency(edges, n):
    adj = np.zeros((n, n), dtype=bool)
    for i, j in edges:
        adj[int(i), int(j)] = adj[int(j), int(i)] = True
    return adj


def pose_count(p1, p2, thresh):
    """Clash count of one rigid pose: pairs of cdist(molecule 2, molecule 1) < thresh."""
    return int(np.count_nonzero(cdist(p2, p1) < thresh))


# ---------------------------------------------------------------------------------------------------------
# extended precision
# ---------------------------------------------------------------------------------------------------------
def rototranslate_ld(X, R, t):
    """(R @ X.T).T + t per block in extended precision: X (n, A, 3), R (n, 3, 3), t (n, 3)."""
    X, R, t = np.asarray(X, dtype=LD), np.asarray(R, dtype=LD), np.asarray(t, dtype=LD)
    out = np.zeros(X.shape, dtype=LD)
    for i in range(3):
        out[..., i] = (R[:, None, i, 0] * X[..., 0] + R[:, None, i, 1] * X[..., 1] + R[:, None, i, 2] * X[..., 2]
                       + t[:, None, i])
    return out


def pose_ld(m1, m2, c1, c2, R1, t1, R2, t2):
    """Poses (P, A1 + A2, 3) of embed_poses_clash in extended precision."""
    a = rototranslate_ld(np.asarray(m1)[c1], R1, t1)
    b = rototranslate_ld(np.asarray(m2)[c2], R2, t2)
    return np.concatenate([a, b], axis=1)


def fitness_error_ld(X, pairs, targets):
    """sum over the constraints with a target of (|x_a - x_b| - target): X (N, A, 3), pairs (N, C, 2) or
    (C, 2), targets (N, C) or (C,) with NaN / None = no target.  Returns (error (N,) longdouble, scale (N,)):
    the scale is max(largest distance, largest |target|) over the structure's constraints, the size the
    rounding bound of the float64 evaluation is stated in."""
    X = np.asarray(X, dtype=LD)
    N = X.shape[0]
    pairs = np.asarray(pairs, dtype=np.int64)
    if pairs.ndim == 2:
        pairs = np.broadcast_to(pairs, (N,) + pairs.shape)
    tg = np.array([[np.nan if v is None else v for v in row] for row in np.atleast_2d(np.asarray(targets, dtype=object))],
                  dtype=np.float64)
    tg = np.broadcast_to(tg, (N, pairs.shape[1]))
    err = np.zeros(N, dtype=LD)
    scale = np.zeros(N)
    rows = np.arange(N)
    for c in range(pairs.shape[1]):
        diff = X[rows, pairs[:, c, 0]] - X[rows, pairs[:, c, 1]]
        d = np.sqrt((diff * diff).sum(axis=1))
        on = ~np.isnan(tg[:, c])
        err = err + np.where(on, d - np.where(on, tg[:, c], 0.0).astype(LD), LD(0))
        scale = np.maximum(scale, np.where(on, np.maximum(d.astype(np.float64), np.abs(np.where(on, tg[:, c], 0.0))), 0.0))
    return err, scale


def inertia_tensor_ld(X, masses):
    """I = sum m (|r|^2 1 - r r^T) about the centre of mass, accumulated in extended precision: (N, 3, 3)."""
    X = np.asarray(X, dtype=LD)
    m = np.asarray(masses, dtype=LD)
    com = (X * m[None, :, None]).sum(axis=1) / m.sum()
    r = X - com[:, None, :]
    r2 = (r * r).sum(axis=2)
    T = np.zeros((X.shape[0], 3, 3), dtype=LD)
    for i in range(3):
        for j in range(3):
            T[:, i, j] = (m[None, :] * ((r2 if i == j else LD(0)) - r[:, :, i] * r[:, :, j])).sum(axis=1)
    return T


def inertia_moments_ld(X, masses):
    """Principal moments, ascending, (N, 3) float64: ``eigvalsh`` of the extended-precision tensor rounded to
    float64 (symmetric eigenvalues are perfectly conditioned: the eigensolver's error is a few eps of the
    largest moment, the tensor's own error is one rounding)."""
    T = inertia_tensor_ld(X, masses).astype(np.float64)
    return np.linalg.eigvalsh(T)


def moi_similar(moments, tol, rows=None):
    """S[a, b]: the oracle's early exit, literally -- a pair is told apart by a moment with rel >= tol and is
    similar when no moment does (nan >= tol is false).  ``rows``: only these a (an (R, N) block)."""
    m = np.asarray(moments)
    a = m if rows is None else m[np.asarray(rows)]
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs(a[:, None, :] - m[None, :, :]) / a[:, None, :]
        return ~(rel >= tol).any(axis=2)


def moi_band(moments, tol, band=1e-10, rows=None):
    """Pairs a correct float64 evaluation may decide either way: some component's relative deviation lies
    within ``band`` of the tolerance.  Same shape as ``moi_similar``."""
    m = np.asarray(moments, dtype=LD)
    a = m if rows is None else m[np.asarray(rows)]
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs(a[:, None, :] - m[None, :, :]) / a[:, None, :]
        return (np.abs(rel - LD(tol)) <= LD(band)).any(axis=2)


# ---------------------------------------------------------------------------------------------------------
# test ensembles
# ---------------------------------------------------------------------------------------------------------
KINDS = ("blob", "molecule", "far", "linear", "axis", "one", "two")


def random_rotations(rng, n):
    q, r = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[np.linalg.det(q) < 0, :, 0] *= -1.0
    return q


def ensemble(kind, n, a, seed, scale=2.0):
    """(n, a, 3) float64 test structures.

    blob      independent normal coordinates of width ``scale`` A (clashes at every distance)
    molecule  conformers of one compact branched molecule (tests/molecule_gen.py; a >= 12): the molecule
              with normal noise of 0.05 A, each in a random orientation and position
    far       ``blob`` shifted by (250, -250, 250) A: coordinates of size 1e2 around a structure of size 1
    linear    atoms on a line along (1, 1, 1)/sqrt(3), spacing 1.2-1.6 A, through a random point
    axis      atoms on the x axis itself (y = z = 0 exactly): the smallest moment is an exact zero
    one, two  ``blob`` with a = 1 or 2 whatever ``a`` says"""
    rng = np.random.default_rng(seed)
    if kind == "one":
        return rng.normal(scale=scale, size=(n, 1, 3))
    if kind == "two":
        return rng.normal(scale=scale, size=(n, 2, 3))
    if kind == "blob":
        return rng.normal(scale=scale, size=(n, a, 3))
    if kind == "far":
        return rng.normal(scale=scale, size=(n, a, 3)) + 250.0 * np.array([1.0, -1.0, 1.0])
    if kind == "molecule":
        from molecule_gen import random_branched_molecule

        _, base, _ = random_branched_molecule(a, seed)
        X = base[None] + rng.normal(scale=0.05, size=(n, a, 3))
        X = X - X.mean(axis=1, keepdims=True)
        return np.ascontiguousarray(np.einsum("nij,naj->nai", random_rotations(rng, n), X) + rng.normal(scale=3.0, size=(n, 1, 3)))
    if kind in ("linear", "axis"):
        s = np.cumsum(rng.uniform(1.2, 1.6, size=(n, a)), axis=1)
        if kind == "axis":
            X = np.zeros((n, a, 3))
            X[:, :, 0] = s
            return X
        u = np.ones(3) / np.sqrt(3.0)
        return s[:, :, None] * u + rng.normal(scale=scale, size=(n, 1, 3))
    raise ValueError(kind)


def tie_structures(t, n, seed, n_frag=2, max_offset=100.0):
    """``n`` structures of ``n_frag`` single-atom fragments whose neighbouring atoms are ``t * (1 + k 2^-52)``
    apart, k in -4..4, along random unit vectors, half of them at the origin and half at random offsets up to
    ``max_offset`` A: after the rounding
    of the coordinates and of cdist the distance lands on, just below or just above ``t``.  (n, n_frag, 3)."""
    rng = np.random.default_rng(seed)
    X = np.empty((n, n_frag, 3))
    X[:, 0] = rng.uniform(-max_offset, max_offset, size=(n, 3)) * rng.integers(0, 2, size=(n, 1))
    for f in range(1, n_frag):
        u = rng.normal(size=(n, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        k = rng.integers(-4, 5, size=(n, 1))
        X[:, f] = X[:, f - 1] + u * (t * (1.0 + k * EPS))
    return X
