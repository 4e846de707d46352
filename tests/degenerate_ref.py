"""Degenerate geometries for the nearest-neighbour and diverse-selection kernels (k_knn_tile, k_knn_tile_sym,
k_diverse_step and its symmetry form) and for the prunes, the refine and the medoids (test_gpu_degenerate_prunes.py), with
closed-form distances where the geometry has one.  Test infrastructure: the product never imports it.

Every generator is seeded and gives every conformer a random proper rotation and a translation; the chains are also
reversed in atom order for a random half.  The kinds and what makes them hard:

  one_atom      the centred conformer is the origin: G = 0, B = 0, every d(i, j) is exactly 0
  two_atoms     after centring the atoms sit at +-v_i: B = 2 v_i v_j^T has rank one, the largest eigenvalue of the
                quaternion matrix is double; d(i, j) = | |v_i| - |v_j| |
  collinear     conformer i is t_i (x) u_i with t_i centred and u_i a unit vector: rank one again;
                d(i, j) = sqrt(min(mean((t_i - t_j)^2), mean((t_i + t_j)^2))) -- the line may be turned end over end
  planar        z = 0 before the rotation: det B = 0 exactly in exact arithmetic, a planar structure is its own mirror
                image (the oracle's rows are the reference)
  mirrored_tops C3-symmetric chiral structures, longest along the axis, and their mirror images: a structure against its
                own image has B = diag(c1, c2, -c2), a DOUBLE largest root c1 on a covariance of full rank; without the
                mirror flag the image is far, with it at 0 (the oracle's rows are the reference)

  scaled        one centred base structure b times a_i = 1 +- d_i / rms(b), the last conformer b itself ("the reference"):
                a_i a_j b^T b is symmetric positive semidefinite, the best rotation is the identity whatever the rank of b;
                rmsd(i, j) = |a_i - a_j| rms(b), maxdev(i, j) = |a_i - a_j| max_a |b_a|.  With d a hair on either side of
                a cap, every (conformer, reference) pair sits at a known distance from a threshold of the prune

tests/test_degenerate_ref.py checks the closed forms against the oracle's rows."""

import numpy as np

from firecode_amd import synthetic as syn


def place(X, rng, shift=5.0):
    """every conformer of X (N, A, 3) under a random proper rotation and a translation N(0, shift^2)"""
    X = np.asarray(X, dtype=np.float64)
    out = np.empty_like(X)
    for n in range(len(X)):
        out[n] = X[n] @ syn.random_rotation(rng).T + rng.normal(scale=shift, size=3)
    return np.ascontiguousarray(out)


# ---- one atom --------------------------------------------------------------------------------------------------------------
def one_atom(N, seed=1):
    """(N, 1, 3): a lone atom anywhere"""
    return place(np.zeros((N, 1, 3)), np.random.default_rng(seed))


# ---- two atoms -------------------------------------------------------------------------------------------------------------
def two_atoms(N, lengths, seed=2):
    """(N, 2, 3): atoms at +-v_i about the centroid, |v_i| = lengths[i]"""
    rng = np.random.default_rng(seed)
    r = np.asarray(lengths, dtype=np.float64).reshape(N)
    X = np.zeros((N, 2, 3))
    X[:, 0, 0], X[:, 1, 0] = r, -r
    return place(X, rng)


def two_atoms_lengths(N, seed=2, lo=0.5, hi=1.1):
    """N half-lengths spread over [lo, hi) A"""
    return np.random.default_rng(1000 + seed).uniform(lo, hi, size=N)


def two_atoms_distances(lengths_q, lengths_r=None):
    """(Nq, Nr): | |v_i| - |v_j| |"""
    a = np.asarray(lengths_q, dtype=np.float64)
    b = a if lengths_r is None else np.asarray(lengths_r, dtype=np.float64)
    return np.abs(a[:, None] - b[None, :])


# ---- atoms on a line -------------------------------------------------------------------------------------------------------
def chain_positions(N, A, params, seed=3):
    """(N, A) centred positions along the line: a chain of ``spacing`` with relative bond-length jitter ``jitter``, an
    overall stretch of up to +-``stretch``; a random half reversed in atom order"""
    rng = np.random.default_rng(seed)
    spacing, jitter = float(params.get("spacing", 1.5)), float(params.get("jitter", 0.02))
    stretch, scale = float(params.get("stretch", 0.05)), float(params.get("scale", 1.0))
    t = np.zeros((N, A))
    if A > 1:
        bonds = spacing * (1.0 + jitter * rng.uniform(-1.0, 1.0, size=(N, A - 1)))
        t[:, 1:] = np.cumsum(bonds, axis=1)
    t *= scale * (1.0 + stretch * rng.uniform(-1.0, 1.0, size=(N, 1)))
    rev = rng.random(N) < 0.5
    t[rev] = t[rev, ::-1]
    return t - t.mean(axis=1, keepdims=True)


def on_lines(t, seed=3):
    """(N, A, 3): conformer i = t_i (x) u_i, u_i a random unit vector, then translated"""
    rng = np.random.default_rng(seed + 7)
    t = np.asarray(t, dtype=np.float64)
    X = np.zeros(t.shape + (3,))
    X[:, :, 0] = t
    return place(X, rng)


def collinear(N, A, params, seed=3):
    """-> (X (N, A, 3), t (N, A)): the chains and their centred positions along the line, as laid out"""
    t = chain_positions(N, A, params, seed)
    return on_lines(t, seed), t


def collinear_distances(tq, tr=None, reversal=False):
    """(Nq, Nr) in float64, evaluated in np.longdouble: sqrt(min(mean((t_i - t_j)^2), mean((t_i + t_j)^2))) on
    re-centred positions; ``reversal``: also the minimum over t_j read backwards (the path's reversal table)"""
    a = np.asarray(tq, dtype=np.longdouble)
    b = a if tr is None else np.asarray(tr, dtype=np.longdouble)
    a = a - a.mean(axis=1, keepdims=True)
    b = b - b.mean(axis=1, keepdims=True)

    def msd(b_):
        minus = ((a[:, None, :] - b_[None, :, :]) ** 2).mean(axis=2)
        plus = ((a[:, None, :] + b_[None, :, :]) ** 2).mean(axis=2)
        return np.minimum(minus, plus)

    m = msd(b)
    if reversal:
        m = np.minimum(m, msd(b[:, ::-1]))
    return np.sqrt(m).astype(np.float64)


# ---- atoms in a plane ------------------------------------------------------------------------------------------------------
def planar(N, A, seed=4, sigma=0.35):
    """(N, A, 3): one planar skeleton displaced in its plane, z exactly 0 before the rotation"""
    rng = np.random.default_rng(seed)
    base = np.zeros((A, 3))
    base[:, :2] = rng.normal(scale=2.0, size=(A, 2)) * np.array([1.6, 1.0])
    X = np.repeat(base[None], N, axis=0)
    X[:, :, :2] += rng.normal(scale=sigma, size=(N, A, 2))
    return place(X, rng)


# ---- symmetric tops and their mirror images --------------------------------------------------------------------------------
def mirrored_tops(N, A, seed=5, sigma=0.15):
    """-> (X (N, A, 3), image_of (N,)): n0 = (N + 1) // 2 chiral C3-symmetric structures (A a multiple of 3: rings of three
    atoms about the z axis, each ring with its own radius, height and twist, the heights spread wider than the radii; the
    noise moves a ring's radius, height and twist, so the symmetry stays) followed by the mirror images (x -> -x before the
    rotation) of the first N - n0 of them.  image_of[i]: the index of i's mirror image, -1 where it has none."""
    assert A % 3 == 0 and A >= 6
    rng = np.random.default_rng(seed)
    rings, n0 = A // 3, (N + 1) // 2
    radius = rng.uniform(0.8, 1.6, size=rings)
    height = np.linspace(-1.0, 1.0, rings) * 1.9 * rings + rng.normal(scale=0.2, size=rings)
    twist = rng.uniform(0.0, 2.0 * np.pi / 3.0, size=rings)
    r = radius[None] + rng.normal(scale=sigma, size=(n0, rings))
    z = height[None] + rng.normal(scale=sigma, size=(n0, rings))
    th = twist[None] + rng.normal(scale=sigma, size=(n0, rings))
    X = np.zeros((n0, rings, 3, 3))
    for m in range(3):
        ang = th + 2.0 * np.pi * m / 3.0
        X[:, :, m, 0], X[:, :, m, 1], X[:, :, m, 2] = r * np.cos(ang), r * np.sin(ang), z
    X = X.reshape(n0, A, 3)
    Y = X[:N - n0].copy()
    Y[:, :, 0] *= -1.0
    image_of = np.full(N, -1, dtype=np.int64)
    image_of[:N - n0] = np.arange(n0, N)
    image_of[n0:] = np.arange(N - n0)
    return place(np.concatenate([X, Y]), rng), image_of


# ---- one structure at many scales: pairs at a known distance from a threshold ---------------------------------------------
SCALED_BASES = ("full", "planar", "line", "full224")
KNIFE_DELTA = (1e-8, 3e-5)  # A: how far inside / outside the cap the knife-edge families put their pairs


def scaled_base(name, seed=7):
    """(A, 3), centred: ``full`` 23 atoms of full rank (an odd count: a padded row), ``planar`` 12 atoms with z = 0,
    ``line`` 40 atoms 1.4 A apart on the x axis, ``full224`` 224 atoms of full rank (the 32-column screen tiles)"""
    if name in ("full", "full224"):
        b = syn.continuous_ensemble(1, 23 if name == "full" else 224, seed)[0]
    elif name == "planar":
        b = np.zeros((12, 3))
        b[:, :2] = np.random.default_rng(seed).normal(scale=2.0, size=(12, 2)) * np.array([1.6, 1.0])
    elif name == "line":
        b = np.zeros((40, 3))
        b[:, 0] = 1.4 * np.arange(40)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(b - b.mean(axis=0, keepdims=True))


def base_rms(base):
    return float(np.sqrt((np.asarray(base, dtype=np.float64) ** 2).sum(axis=1).mean()))


def base_reach(base):
    """max_a |b_a|: the atom farthest from the centroid"""
    return float(np.sqrt((np.asarray(base, dtype=np.float64) ** 2).sum(axis=1).max()))


def knife_offsets(cap, n):
    """(n,) distances from the reference: the first half at cap - delta, the second at cap + delta, delta log-spaced over
    KNIFE_DELTA"""
    delta = np.logspace(np.log10(KNIFE_DELTA[0]), np.log10(KNIFE_DELTA[1]), n // 2)
    return np.concatenate([cap - delta, cap + delta[:n - n // 2]])


def scaled_family(base, d, seed):
    """-> (X (n + 1, A, 3), a (n + 1,)): conformer i = a_i b under a random proper rotation and a translation,
    a_i = 1 +- d_i / rms(b) with the sign drawn per conformer; the last conformer, a = 1, is the reference"""
    rng = np.random.default_rng(seed)
    b, d = np.asarray(base, dtype=np.float64), np.asarray(d, dtype=np.float64)
    a = np.append(1.0 + rng.choice([-1.0, 1.0], size=len(d)) * d / base_rms(b), 1.0)
    return place(a[:, None, None] * b[None], rng), a


def scaled_rmsd(base, a):
    """(n, n): |a_i - a_j| rms(b)"""
    a = np.asarray(a, dtype=np.float64)
    return np.abs(a[:, None] - a[None, :]) * base_rms(base)


def scaled_maxdev(base, a):
    """(n, n): |a_i - a_j| max_a |b_a|"""
    a = np.asarray(a, dtype=np.float64)
    return np.abs(a[:, None] - a[None, :]) * base_reach(base)


def knife_thresholds(base, cap, edge):
    """(max_rmsd, max_dev) that put the (conformer, reference) pairs of ``knife_offsets(cap, .)`` at the edge of the RMSD
    test (``edge="rmsd"``: the max deviation, about 1.5 RMSD on these bases, is clear) or of the max-deviation test
    (``edge="dev"``: the RMSD is clear, and pairs of opposite sign, 2 cap apart, are out on the RMSD)"""
    if edge == "rmsd":
        return cap, 4.0 * cap
    return 1.5 * cap, base_reach(base) / base_rms(base) * cap
