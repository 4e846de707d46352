"""An arbitrary-precision reference of the Kabsch superposition, and one fixed ladder of pairs for everything that checks
firecode_amd/csrc/fc_kabsch_math.h (tests/test_kabsch_math_cpu.py on the host, tests/test_gpu_kabsch_math.py on the device)
and the float64 oracle with its tolerance (oracle/cpu_ref.py).  Test infrastructure: the product never imports it.

The reference works in mpmath at 60 digits from the float64 coordinates taken exactly, in the header's own convention:
B[x][y] = sum_a p_a[x] q_a[y], Horn's S_xy = B[y][x], K the 4 x 4 quaternion matrix of kabsch_rotation, R = R(q) of its
dominant unit eigenvector q applied as q' = R q.  With the singular values f1 >= f2 >= |f3| of B (f3 signed by det B) the
eigenvalues of K are f1+f2+f3 >= f1-f2-f3 >= -f1+f2-f3 >= -f1-f2+f3, so

    gap = (lambda1 - lambda2) / 2 = f2 + f3                     (the smallest gap of the polar factor)
    gap product = (l1 - l2)(l1 - l3)(l1 - l4) = P'(lambda1)     (what the adjugate's certificates are about)
    the mirror image (-B) has the eigenvalues of -K: lambda1(-B) = -lambda4(B)

kabsch_ladder() is seeded and fixed; every family states where the reference's gap, msd or q0^2 must lie, and
check_ladder_claims() asserts that from the reference alone, before anything under test is called."""

import functools

import mpmath as mp
import numpy as np

mp.mp.dps = 60

EPS = float(np.finfo(np.float64).eps)


# ---- the reference ---------------------------------------------------------------------------------------------------------
def _mpf_rows(x):
    return [[mp.mpf(float(v)) for v in row] for row in np.asarray(x, dtype=np.float64)]


def _centred(rows):
    n = len(rows)
    c = [mp.fsum(r[k] for r in rows) / n for k in range(3)]
    return [[r[k] - c[k] for k in range(3)] for r in rows]


def horn_matrix(B):
    """K of kabsch_rotation from B (3 x 3 nested lists or mp.matrix entries B[x][y])"""
    Sxx, Sxy, Sxz = B[0][0], B[1][0], B[2][0]
    Syx, Syy, Syz = B[0][1], B[1][1], B[2][1]
    Szx, Szy, Szz = B[0][2], B[1][2], B[2][2]
    K = mp.matrix(4, 4)
    K[0, 0] = Sxx + Syy + Szz
    K[0, 1] = K[1, 0] = Syz - Szy
    K[0, 2] = K[2, 0] = Szx - Sxz
    K[0, 3] = K[3, 0] = Sxy - Syx
    K[1, 1] = Sxx - Syy - Szz
    K[1, 2] = K[2, 1] = Sxy + Syx
    K[1, 3] = K[3, 1] = Szx + Sxz
    K[2, 2] = -Sxx + Syy - Szz
    K[2, 3] = K[3, 2] = Syz + Szy
    K[3, 3] = -Sxx - Syy + Szz
    return K


def rotation_of(q):
    q0, q1, q2, q3 = q
    return [[q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
            [2 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 - q0 * q1)],
            [2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3]]


class Ref:
    """What the reference knows of one pair.  Attributes in mpmath: B (3 x 3 lists), G (= Gp + Gq), S (= G / 2), A, lam
    (the four eigenvalues, descending), q (unit eigenvector of lam[0], q0 >= 0), R, msd, rmsd, maxdev, gap, gap_product,
    C2, C1, C0, n2, det, e2; and the same for the mirror image: lam_m, msd_m, rmsd_m, gap_m, gap_product_m."""

    def poly(self, L, mirror=False):
        """-> (P(L), P'(L), P''(L)) of the characteristic polynomial x^4 + C2 x^2 + C1 x + C0 (of -B: C1 negated)"""
        L = mp.mpf(L)
        C1 = -self.C1 if mirror else self.C1
        return (((L * L + self.C2) * L + C1) * L + self.C0, (4 * L * L + 2 * self.C2) * L + C1, 12 * L * L + 2 * self.C2)

    def screen_values(self, L, enant=False):
        """the three values kabsch_may_be_below tests, exactly: (P, P'/4, P''/4) at |det B| under ENANT"""
        mirror = enant and self.det < 0
        P0, P1, P2 = self.poly(L, mirror)
        return P0, P1 / 4, P2 / 4


def reference(p, q, center=True, with_maxdev=True):
    """-> Ref of the pair (p, q): (A, 3) float64 arrays taken exactly"""
    pr, qr = _mpf_rows(p), _mpf_rows(q)
    if center:
        pr, qr = _centred(pr), _centred(qr)
    r = Ref()
    r.A = len(pr)
    r.B = [[mp.fdot([a[x] for a in pr], [b[y] for b in qr]) for y in range(3)] for x in range(3)]
    r.G = mp.fsum(v * v for a in pr for v in a) + mp.fsum(v * v for b in qr for v in b)
    r.S = r.G / 2
    B = r.B
    r.n2 = mp.fsum(B[x][y] ** 2 for x in range(3) for y in range(3))
    cof = [[B[(x + 1) % 3][(y + 1) % 3] * B[(x + 2) % 3][(y + 2) % 3] - B[(x + 1) % 3][(y + 2) % 3] * B[(x + 2) % 3][(y + 1) % 3]
            for y in range(3)] for x in range(3)]
    r.det = mp.fsum(B[0][y] * cof[0][y] for y in range(3))
    r.e2 = mp.fsum(cof[x][y] ** 2 for x in range(3) for y in range(3))
    r.C2, r.C1, r.C0 = -2 * r.n2, -8 * r.det, r.n2 * r.n2 - 4 * r.e2
    if r.n2 == 0:
        ev, vec = [mp.mpf(0)] * 4, mp.eye(4)
    else:
        E, V = mp.eigsy(horn_matrix(B))
        order = sorted(range(4), key=lambda k: -E[k])
        ev = [E[k] for k in order]
        vec = V[:, order[0]]
    r.lam = ev
    qv = [vec[k, 0] for k in range(4)]
    nrm = mp.sqrt(mp.fsum(v * v for v in qv))
    qv = [v / nrm for v in qv]
    if qv[0] < 0:
        qv = [-v for v in qv]
    r.q = qv
    r.R = rotation_of(qv)
    r.msd = (r.G - 2 * ev[0]) / r.A
    r.msd = max(r.msd, mp.mpf(0))
    r.rmsd = mp.sqrt(r.msd)
    r.gap = (ev[0] - ev[1]) / 2
    r.gap_product = (ev[0] - ev[1]) * (ev[0] - ev[2]) * (ev[0] - ev[3])
    r.lam_m = [-v for v in reversed(ev)]
    r.msd_m = max((r.G - 2 * r.lam_m[0]) / r.A, mp.mpf(0))
    r.rmsd_m = mp.sqrt(r.msd_m)
    r.gap_m = (r.lam_m[0] - r.lam_m[1]) / 2
    r.gap_product_m = (r.lam_m[0] - r.lam_m[1]) * (r.lam_m[0] - r.lam_m[2]) * (r.lam_m[0] - r.lam_m[3])
    r.maxdev = None
    if with_maxdev:
        R, worst = r.R, mp.mpf(0)
        for a, b in zip(pr, qr):
            d2 = mp.fsum((a[x] - (R[x][0] * b[0] + R[x][1] * b[1] + R[x][2] * b[2])) ** 2 for x in range(3))
            worst = max(worst, d2)
        r.maxdev = mp.sqrt(worst)
    r.rmax = mp.sqrt(max(mp.fsum(v * v for v in a) for a in pr + qr))
    return r


# ---- float64 inputs of the routines under test -----------------------------------------------------------------------------
def record_inputs(p, q, center=True):
    """-> (B (3, 3), Gp + Gq) in float64 as a caller hands them to the header: sums accumulated in extended precision
    and rounded once, so that what a test measures is the header's error and not that of its inputs"""
    p, q = np.asarray(p, dtype=np.longdouble), np.asarray(q, dtype=np.longdouble)
    if center:
        p, q = p - p.mean(axis=0), q - q.mean(axis=0)
    return (p.T @ q).astype(np.float64), float((p * p).sum() + (q * q).sum())


# ---- the ladder ------------------------------------------------------------------------------------------------------------
def rotation_about(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    w = np.cos(0.5 * angle)
    x, y, z = np.sin(0.5 * angle) * axis
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def random_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return rotation_about(q[1:] if np.linalg.norm(q[1:]) > 0 else [1.0, 0.0, 0.0], 2.0 * np.arccos(np.clip(q[0], -1.0, 1.0)))


def _c(x):
    return np.ascontiguousarray(x - x.mean(axis=0))


def _top(rng, A):
    """a chiral C3-symmetric structure, longest along its axis (tests/degenerate_ref.py: mirrored_tops)"""
    rings = A // 3
    radius = rng.uniform(0.8, 1.6, size=rings)
    height = np.linspace(-1.0, 1.0, rings) * 0.9 * rings + rng.normal(scale=0.2, size=rings)
    twist = rng.uniform(0.0, 2.0 * np.pi / 3.0, size=rings)
    X = np.zeros((rings, 3, 3))
    for m in range(3):
        ang = twist + 2.0 * np.pi * m / 3.0
        X[:, m, 0], X[:, m, 1], X[:, m, 2] = radius * np.cos(ang), radius * np.sin(ang), height
    return _c(X.reshape(A, 3))


class Pair:
    def __init__(self, family, p, q, center=True, thr=None, **claim):
        self.family, self.p, self.q, self.center, self.thr, self.claim = family, p, q, center, thr, claim
        self.A = p.shape[0]

    @functools.cached_property
    def ref(self):
        return reference(self.p, self.q, self.center)

    @functools.cached_property
    def inputs(self):
        return record_inputs(self.p, self.q, self.center)


KNIFE_THR = (0.05, 0.25, 0.5)
KNIFE_DELTA = (1e-14, 1e-12, 1e-10, 1e-8, 1e-6, 1e-4, 1e-2)


def _knife(make, t, thr, target_rel):
    """the pair make(t) -> (p, q) with t tuned until the reference's msd is thr^2 (1 + target_rel): a fixed-point iteration on
    the mpmath msd (make's msd grows as t^2), then single steps in the last places of t until the msd lies on the side
    asked for"""
    want = mp.mpf(thr) ** 2 * (1 + mp.mpf(target_rel))

    def at(t):
        p, q = make(t)
        return p, q, reference(p, q, True, with_maxdev=False).msd

    for _ in range(6):
        p, q, m = at(t)
        t = float(t * mp.sqrt(want / m))
    p, q, m = at(t)
    side = 1 if target_rel > 0 else -1
    for _ in range(200):
        if (m - mp.mpf(thr) ** 2) * side > 0:
            break
        t = float(np.nextafter(t, np.inf if side > 0 else 0.0))
        p, q, m = at(t)
    return p, q


@functools.lru_cache(maxsize=None)
def kabsch_ladder():
    """-> tuple of Pair: the fixed ladder (see the module's docstring and DESIGN.md, "What the math-header tests pin down")"""
    out = []
    rng = np.random.default_rng(20240607)

    # 1. unrelated structures, and noisy rotated copies
    for A in (3, 4, 13, 50, 260):
        for noise in np.geomspace(1e-8, 2.0, 40):
            p = _c(rng.normal(scale=2.0, size=(A, 3)) * np.array([1.5, 1.0, 0.7]))
            q = _c((p + rng.normal(size=(A, 3)) * noise) @ random_rotation(rng).T)
            out.append(Pair("noisy", p, q, noise=noise))
        for _ in range(8):
            p, q = _c(rng.normal(scale=2.0, size=(A, 3))), _c(rng.normal(scale=2.0, size=(A, 3)) @ random_rotation(rng).T)
            out.append(Pair("unrelated", p, q))

    # 2. nearly collinear: a line plus transverse noise eps
    for A in (3, 13, 40):
        for eps in np.geomspace(1e-12, 1e-1, 12):
            for _ in range(6):
                def line():
                    x = np.zeros((A, 3))
                    x[:, 0] = 1.5 * np.arange(A) * (1.0 + 0.05 * rng.uniform(-1, 1)) + 0.03 * rng.uniform(-1, 1, size=A)
                    x[:, 1:] = eps * rng.uniform(-1.0, 1.0, size=(A, 2))
                    return _c(x)
                p, q = _c(line() @ random_rotation(rng).T), _c(line() @ random_rotation(rng).T)
                out.append(Pair("collinear", p, q, eps=eps))

    # 3. nearly double largest root: symmetric tops against their mirror images, perturbed by eps
    for A in (12, 24):
        for eps in (0.0,) + tuple(np.geomspace(1e-14, 1e-2, 13)):
            for _ in range(6):
                p = _top(rng, A)
                img = p * np.array([-1.0, 1.0, 1.0]) + eps * rng.uniform(-1.0, 1.0, size=(A, 3))
                out.append(Pair("double-root", _c(p @ random_rotation(rng).T), _c(img @ random_rotation(rng).T), eps=eps))

    # 4. planar pairs and their reflections
    for k in range(60):
        def flat():
            x = np.zeros((12, 3))
            x[:, :2] = base2 + rng.normal(scale=0.35, size=(12, 2))
            return x
        base2 = rng.normal(scale=2.0, size=(12, 2)) * np.array([1.6, 1.0])
        p, q = flat(), flat()
        if k % 2:
            q[:, 0] *= -1.0
        out.append(Pair("planar", _c(p @ random_rotation(rng).T), _c(q @ random_rotation(rng).T)))

    # 5. one atom; two atoms about their centroid; an all-zero covariance
    for _ in range(4):
        out.append(Pair("tiny", rng.normal(scale=5.0, size=(1, 3)), rng.normal(scale=5.0, size=(1, 3)), kind="one-atom"))
    for _ in range(20):
        def pair2():
            v = rng.uniform(0.5, 1.1) * random_rotation(rng)[:, 0]
            return np.stack([v, -v])
        out.append(Pair("tiny", pair2(), pair2(), kind="two-atoms"))
    for _ in range(6):
        out.append(Pair("tiny", _c(rng.normal(scale=2.0, size=(4, 3))), np.zeros((4, 3)), kind="zero-covariance"))

    # 6. half turns about x, y, z and a random axis, and q0^2 through the column-0 certificate's boundary.  No rigid move
    # here: the rotation between the two structures IS what is swept
    Q0SQ = (0.3, 0.45, 0.49, 0.5, 0.51, 0.55, 0.58, 0.6, 0.62, 0.65, 0.69, 0.7, 0.71, 0.8, 0.9, 0.99, 1.0)
    for A in (13, 50):
        for axis in ([1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], rng.normal(size=3)):
            angles = [np.pi + s * d for d in (0.0, 1e-12, 1e-8, 1e-4, 1e-2, 0.3) for s in (1, -1)][1:]
            angles += [2.0 * np.arccos(np.sqrt(v)) for v in Q0SQ]
            for ang in angles:
                p = _c(rng.normal(scale=2.0, size=(A, 3)) * np.array([1.5, 1.0, 0.7]))
                q = _c((p + rng.normal(scale=0.01, size=(A, 3))) @ rotation_about(axis, ang))  # rows q_a = R^T p_a: R q = p
                out.append(Pair("half-turn", p, q, q0sq=float(np.cos(0.5 * ang) ** 2)))

    # 7. knife-edge at a threshold: true msd = thr^2 (1 +- delta), arbitrary best rotations; and on the double-root family
    for A in (23, 50, 224):
        for thr in KNIFE_THR:
            for delta in KNIFE_DELTA:
                for side in (-1.0, 1.0):
                    base, noise, Rm = _c(rng.normal(scale=0.7, size=(A, 3))), rng.normal(size=(A, 3)), random_rotation(rng)
                    p, q = _knife(lambda t: (base, _c((base + t * noise) @ Rm.T)), thr / np.sqrt(3.0), thr, side * delta)
                    out.append(Pair("knife", p, q, thr=thr, delta=side * delta))
    for thr in KNIFE_THR:
        for delta in KNIFE_DELTA:
            for side in (-1.0, 1.0):
                # (a top against its image, both scaled by t: the msd is t^2 times that of the pair as drawn)
                top, Rm = _top(rng, 24), random_rotation(rng)
                img = _c((top * np.array([-1.0, 1.0, 1.0])) @ Rm.T)
                p, q = _knife(lambda t: (_c(top * t), _c(img * t)), 0.3 * thr, thr, side * delta)
                out.append(Pair("knife-double", p, q, thr=thr, delta=side * delta))

    # 8. scale and offset: the same pairs at 1e-3 x, 1 x, 300 x, and uncentred 300 A away (center=False callers)
    for k in range(20):
        p = _c(rng.normal(scale=2.0, size=(50, 3)) * np.array([1.5, 1.0, 0.7]))
        q = _c((p + rng.normal(size=(50, 3)) * float(np.geomspace(1e-3, 1.0, 20)[k])) @ random_rotation(rng).T)
        for scale in (1e-3, 1.0, 300.0):
            out.append(Pair("scale", p * scale, q * scale, scale=scale))
        out.append(Pair("offset", p + 300.0, q + 300.0, center=False))
    return tuple(out)


FAMILIES = ("noisy", "unrelated", "collinear", "double-root", "planar", "tiny", "half-turn", "knife", "knife-double", "scale",
            "offset")


def check_ladder_claims(ladder=None):
    """every family's claim about gap, msd and q0^2, from the reference alone"""
    for e in ladder or kabsch_ladder():
        r, c = e.ref, e.claim
        S = r.S
        if e.family == "noisy":
            assert r.rmsd <= 2.0 * c["noise"] * mp.sqrt(3), (e.family, c)
            if c["noise"] <= 0.1 and e.A >= 4:
                assert r.gap > 1e-3 * S
        elif e.family == "collinear":
            assert r.gap <= 4 * e.A * c["eps"] ** 2 and r.gap <= 1e-2 * S, (c, float(r.gap / S))
        elif e.family == "double-root":
            assert r.lam[0] - r.lam[1] <= (40 * c["eps"] + 1e-13) * r.lam[0], (c, float((r.lam[0] - r.lam[1]) / r.lam[0]))
            assert r.lam[1] - r.lam[2] > 1e-2 * r.lam[0]  # (a covariance of full rank: not the collinear case)
        elif e.family == "planar":
            assert abs(r.det) <= 1e-13 * S ** 3
        elif e.family == "tiny":
            if c["kind"] == "two-atoms":
                assert r.lam[0] - r.lam[1] <= 1e-14 * S and r.lam[0] > 0
            else:
                assert r.n2 == 0 and r.lam[0] == 0
        elif e.family == "half-turn":
            assert abs(r.q[0] ** 2 - c["q0sq"]) <= 0.02, (c, float(r.q[0] ** 2))
            assert r.gap > 1e-2 * S
        elif e.family in ("knife", "knife-double"):
            rel = r.msd / mp.mpf(e.thr) ** 2 - 1
            d = c["delta"]
            assert rel * d > 0 and abs(rel) <= 4 * abs(d) + 1e-14, (e.family, e.thr, d, float(rel))
            A_thr2 = e.A * mp.mpf(e.thr) ** 2
            assert A_thr2 >= 1e-3 * S and A_thr2 < 0.5 * S, (e.family, e.thr, float(A_thr2 / S))
            if e.family == "knife-double":
                assert r.lam[0] - r.lam[1] <= 1e-13 * r.lam[0]
        elif e.family == "scale":
            assert r.gap > 1e-3 * S
        elif e.family == "offset":
            assert S > 50 * 3 * 300.0 ** 2
