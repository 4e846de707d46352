"""The one-sidedness the filters of the nearest-neighbour kernels and of the symmetry-aware steps lean on
(csrc/fc_knn.hip: k_knn_tile, k_knn_tile_sym; csrc/fc_diverse.hip: k_diverse_step_sym), checked in NumPy (no GPU):

a (pair, p, h) is left out of the explicit pass when the eigenvalue form of its A msd, (Gp + Gq) - 2 lambda, exceeds a
bound by more than a margin --

    k_knn_tile (and `tau` in _sym)   A tau^2 + A kScreenMargin + kKnnFilterRel (Gp + Gq)
    the `best` rule of the _sym kernels      best + A kScreenMargin

-- so no pair whose EXPLICIT sum is at most A tau^2 (at most `best`) may be ruled out: the eigenvalue form may exceed the
explicit sum by no more than the margin.  Here fc_kabsch_math.h is restated in float64 (per-lane stopping, no fused
multiply-adds: the device's contraction is not modelled, tests/test_gpu_degenerate_neighbours.py asks the device itself)
-- kabsch_lambda_max with the slope and the last step it reports, kabsch_lambda_is_settled and kabsch_lambda_upper --
against the sum of squares from the oracle's rmsd (closed forms where tests/degenerate_ref.py has one), on random
full-rank pairs, planar pairs, symmetric tops and their mirror images (a double root on a covariance of full rank),
two-atom pairs and atoms on a line -- chains of 3, 13, 20, 30 and 40 atoms at 1.4 ... 1.5 A -- at 1 x and at 30 x; the first
three in both handednesses (the -B of kabsch_lambda_max_both).

What it found, and keeps (test_bare_newton_value_is_two_sided): where the largest root is (nearly) double the bare
iteration ends on EITHER side of it -- the eigenvalue form up to 9e-9 (Gp + Gq) above the explicit sum on rank-one
covariances, which passes A kScreenMargin + kKnnFilterRel (Gp + Gq) from about 20 atoms on a line at 1.5 A and from 2
atoms at 30 x, and up to 9e-7 (Gp + Gq) on the tops, where a step over a vanishing slope throws the iterate far away and
the 64 steps end before it is back -- or converge on the third or fourth root, cleanly.  The rules therefore use
kabsch_lambda_upper: the Newton value where kabsch_lambda_is_settled certifies it as the largest root (settled, right of
the inflection points of P, on a positive slope), (Gp + Gq)/2 -- A msd = 0, nothing ruled out -- elsewhere;
test_no_accepted_value_lies_below_a_double_largest_root sweeps 4e6 (nearly) double roots for that certificate."""

import numpy as np
import pytest

import degenerate_ref as dg
import diverse_sym_ref as ds
from firecode_amd import synthetic as syn
from oracle import cpu_ref as o

K_SCREEN_MARGIN = 1e-6        # fc_common.h: kScreenMargin
K_KNN_FILTER_REL = 1e-10      # fc_knn.hip: kKnnFilterRel
K_SETTLED_STEP = 1e-12        # fc_kabsch_math.h: kLambdaSettledStep
K_SETTLED_SLOPE = 1e-3        # fc_kabsch_math.h: kLambdaSettledSlope


def lambda_newton(B, gg):
    """kabsch_lambda_max, vectorised over pairs with its per-lane stopping rule -> (lambda, slope, last step, |B|_F^2)"""
    B = np.asarray(B, dtype=np.float64)
    n2 = (B * B).sum(axis=(1, 2))
    c = np.empty_like(B)
    for i in range(3):
        for j in range(3):
            r = [k for k in range(3) if k != i]
            s = [k for k in range(3) if k != j]
            c[:, i, j] = B[:, r[0], s[0]] * B[:, r[1], s[1]] - B[:, r[0], s[1]] * B[:, r[1], s[0]]
    # the expansion along the first row, signs as the kernel writes them
    det = B[:, 0, 0] * c[:, 0, 0] - B[:, 0, 1] * c[:, 0, 1] + B[:, 0, 2] * c[:, 0, 2]
    e2 = (c * c).sum(axis=(1, 2))
    C2, C1, C0 = -2.0 * n2, -8.0 * det, n2 * n2 - 4.0 * e2
    x = 0.5 * np.asarray(gg, dtype=np.float64).copy()
    den = np.zeros_like(x)
    last = np.full_like(x, np.inf)  # (+inf: no step taken -- den == 0 at the start)
    live = np.ones(len(x), dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for _ in range(64):
            x2 = x * x
            b = (x2 + C2) * x
            a = b + C1
            d = 2.0 * x2 * x + b + a
            den = np.where(live, d, den)
            live &= d != 0.0
            delta = np.where(live, (a * x + C0) / np.where(d == 0.0, 1.0, d), 0.0)
            x = x - delta
            last = np.where(live, delta, last)
            live &= ~(np.abs(delta) <= 4e-16 * np.abs(x))
            if not live.any():
                break
    return x, den, last, n2


def is_settled(lam, slope, step, n2):
    """kabsch_lambda_is_settled: settled, right of the inflection points of P, on a positive slope -- the largest root"""
    with np.errstate(invalid="ignore"):
        return ((lam > 0.0) & (np.abs(step) <= K_SETTLED_STEP * lam) & (3.0 * (lam * lam) > n2)
                & (slope >= K_SETTLED_SLOPE * (lam * lam * lam)))


def settled_on_some_simple_root(lam, slope, step):
    """the weaker test that is NOT enough (test_no_accepted_value_lies_below_a_double_largest_root)"""
    ax = np.abs(lam)
    return (np.abs(step) <= K_SETTLED_STEP * ax) & (np.abs(slope) >= K_SETTLED_SLOPE * (ax * ax * ax))


class Pairs:
    """a set of pairs (one handedness): what the rules see of each, and its exact sum of squares"""

    def __init__(self, P, Q, ssq_exact):
        P = P - P.mean(axis=1, keepdims=True)
        Q = Q - Q.mean(axis=1, keepdims=True)
        self.A = P.shape[1]
        self.gg = (P * P).sum(axis=(1, 2)) + (Q * Q).sum(axis=(1, 2))
        lam, slope, step, n2 = lambda_newton(np.einsum("nai,naj->nij", P, Q), self.gg)
        self.settled = is_settled(lam, slope, step, n2)
        self.bare = (self.gg - 2.0 * lam) - ssq_exact                                           # the parent's value
        self.used = (self.gg - 2.0 * np.where(self.settled, lam, 0.5 * self.gg)) - ssq_exact    # kabsch_lambda_upper's
        self.tile_margin = self.A * K_SCREEN_MARGIN + K_KNN_FILTER_REL * self.gg
        self.best_margin = self.A * K_SCREEN_MARGIN


def _oracle_ssq(P, Q):
    return o.rmsd_and_max_batch(P, Q, center=True)[0] ** 2 * P.shape[1]


def _draw(n, n_pairs, rng):
    return rng.integers(0, n, size=n_pairs), rng.integers(0, n, size=n_pairs)


def _set(kind, scale):
    """-> [Pairs, ...]: one entry per handedness"""
    rng = np.random.default_rng(11)
    if kind in ("full-rank", "planar", "mirrored-tops"):
        if kind == "full-rank":
            X = np.concatenate([syn.continuous_ensemble(100, 20, seed=5), ds.ensemble("clusters", 100, 20, "identity", False)[0]])
            i, j = _draw(len(X), 4000, rng)
        elif kind == "planar":
            X = dg.planar(100, 12)
            i, j = _draw(len(X), 4000, rng)
        else:
            X, image_of = dg.mirrored_tops(100, 12)
            i, j = _draw(len(X), 3000, rng)
            own = np.flatnonzero(image_of >= 0)  # every structure against its own image: the double root itself
            i, j = np.concatenate([i, own]), np.concatenate([j, image_of[own]])
        X = X - X.mean(axis=1, keepdims=True)
        P, Q = X[i] * scale, X[j] * scale
        return [Pairs(P, Q, _oracle_ssq(P, Q)), Pairs(P, -Q, _oracle_ssq(P, -Q))]
    if kind == "two-atoms":
        r = dg.two_atoms_lengths(200) * scale
        X = dg.two_atoms(200, r)
        i, j = _draw(200, 4000, rng)
        return [Pairs(X[i], X[j], 2.0 * dg.two_atoms_distances(r)[i, j] ** 2)]
    A = int(kind.split("-")[1])
    params = {"spacing": 1.5 if A % 2 else 1.4, "jitter": 0.02, "stretch": 0.05, "scale": scale}
    X, t = dg.collinear(200, A, params, seed=A)
    i, j = _draw(200, 10000, rng)
    tl = np.asarray(t, dtype=np.longdouble)
    ssq = np.minimum(((tl[i] - tl[j]) ** 2).sum(axis=1), ((tl[i] + tl[j]) ** 2).sum(axis=1)).astype(np.float64)
    return [Pairs(X[i], X[j], ssq)]


CHAINS = ["chain-3", "chain-13", "chain-20", "chain-30", "chain-40"]
KINDS = ["full-rank", "planar", "mirrored-tops", "two-atoms"] + CHAINS
_SETS = {}


def _pairs_of(kind, scale):
    if (kind, scale) not in _SETS:
        _SETS[kind, scale] = _set(kind, scale)
    return _SETS[kind, scale]


@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("kind", KINDS)
def test_no_pair_within_the_bound_is_ruled_out(kind, scale):
    """both rules at their knife-edge -- tau^2 = the pair's own msd, best = the pair's own sum -- rule a pair out exactly
    when the eigenvalue form exceeds the exact sum by more than the margin: that must not happen, with a factor of 4 to
    spare for the arithmetic this restatement does not model"""
    for h, p in enumerate(_pairs_of(kind, scale)):
        print(f"{kind} x{scale:g} h={h}: GG ~{np.median(p.gg):.3g}, settled {p.settled.mean():.3f}, eigenvalue form above the "
              f"exact sum by at most {p.used.max():.3g} (bare: {p.bare.max():.3g} = {(p.bare / p.gg).max():.3g} GG), "
              f"margins {p.tile_margin.min():.3g} / {p.best_margin:.3g}")
        assert np.all(np.isfinite(p.used))
        assert not np.any(4.0 * p.used > p.tile_margin), "k_knn_tile's rule drops a pair whose explicit sum is at most A tau^2"
        assert not np.any(4.0 * p.used > p.best_margin), "the `best` rule drops a (pair, p, h) whose explicit sum is at most best"


def test_bare_newton_value_is_two_sided():
    """the bare Newton value (what the rules used before kabsch_lambda_upper): within the margins on short chains at
    1 x, above them on long ones and at 30 x, and far above them on symmetric tops against their images"""
    over = {}
    for kind in CHAINS + ["two-atoms", "mirrored-tops"]:
        for scale in (1.0, 30.0):
            over[kind, scale] = sum(int((p.bare > p.tile_margin).sum()) for p in _pairs_of(kind, scale))
    print(over)
    assert over["chain-3", 1.0] == 0 and over["chain-13", 1.0] == 0 and over["two-atoms", 1.0] == 0
    assert over["chain-30", 1.0] > 0 and over["chain-40", 1.0] > 0
    assert all(over[kind, 30.0] > 0 for kind in CHAINS + ["two-atoms", "mirrored-tops"])
    worst = max(float((p.bare / p.gg).max()) for kind in CHAINS for p in _pairs_of(kind, 1.0))
    assert 1e-9 < worst < 1e-7  # ~sqrt(u): 8.6e-9 (Gp + Gq) measured
    # every pair that is over the margin is one the settled test declines
    for key in over:
        for p in _pairs_of(*key):
            assert not (p.settled & (p.bare > 0.25 * p.tile_margin)).any()


def test_settled_test_leaves_simple_roots_alone():
    """the filter stays as sharp as it was where it matters: every full-rank and every planar pair, in either handedness,
    keeps its Newton value; no rank-one pair does"""
    for scale in (1.0, 30.0):
        for kind in ("full-rank", "planar"):
            for p in _pairs_of(kind, scale):
                assert p.settled.all()
                assert np.abs(p.bare).max() < 1e-13 * p.gg.max()  # (and that value is the oracle's sum to rounding)
        for kind in CHAINS + ["two-atoms"]:
            assert not any(p.settled.any() for p in _pairs_of(kind, scale))
        tops = _pairs_of("mirrored-tops", scale)
        assert 0.2 < np.concatenate([p.settled for p in tops]).mean() < 0.9  # (both outcomes are exercised there)


def test_one_atom_rules_nothing_out():
    """B = 0, G = 0: den == 0 at the start, no step, not settled -- and A msd = 0 either way"""
    lam, slope, step, n2 = lambda_newton(np.zeros((3, 3, 3)), np.zeros(3))
    assert np.all(lam == 0.0) and np.all(slope == 0.0) and np.all(np.isinf(step)) and not is_settled(lam, slope, step, n2).any()


# ---- a direct sweep over (nearly) double largest roots ---------------------------------------------------------------------
def _rotations(rng, n):
    """n random proper rotations from unit quaternions"""
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)


SWEEP_CHUNKS, SWEEP_CHUNK = 8, 500_000


def _double_root_sweep():
    """B = U diag(c1, c2, -c2 (1 + eps)) V^T: the four roots are c1 -+ c2 eps (the largest pair, double at eps = 0),
    2 c2 - c1 + c2 eps and -(c1 + 2 c2 + c2 eps).  eps = 0 for a third of the draws, log-uniform in 1e-16 ... 1e-2 with either
    sign for the rest; the start c1 + c2 (2 + |eps|) (a structure against its own image) for half, up to twice that for
    the rest -> per chunk (lambda, slope, step, n2, the largest root)"""
    for chunk in range(SWEEP_CHUNKS):
        rng = np.random.default_rng(1000 + chunk)
        n = SWEEP_CHUNK
        c1 = rng.uniform(1.0, 10.0, size=n)
        c2 = c1 * rng.uniform(0.05, 0.999, size=n)
        eps = np.where(rng.random(n) < 1.0 / 3.0, 0.0, rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-16.0, -2.0, size=n))
        s3 = -c2 * (1.0 + eps)
        U, V = _rotations(rng, n), _rotations(rng, n)
        B = np.einsum("nik,nk,njk->nij", U, np.stack([c1, c2, s3], axis=1), V)
        half = (c1 + c2 + np.abs(s3)) * np.where(rng.random(n) < 0.5, 1.0, rng.uniform(1.0, 2.0, size=n))
        largest = np.maximum(c1 + c2 + s3, c1 - c2 - s3)
        yield lambda_newton(B, 2.0 * half) + (largest,)


def test_no_accepted_value_lies_below_a_double_largest_root():
    """4e6 covariances with an exact or nearly double largest root on full rank: whatever kabsch_lambda_is_settled accepts
    is the LARGEST root to 2e-11 of it.  A test that only asks for a small step on a simple root accepts the third or the
    fourth root a few times in 1e6 (the iterate is thrown below the critical points of P and converges there cleanly):
    counted here, so that the sweep is known to reach the case"""
    accepted = stray = 0
    worst = 0.0
    for lam, slope, step, n2, largest in _double_root_sweep():
        ok = is_settled(lam, slope, step, n2)
        accepted += int(ok.sum())
        short = (largest - lam) / largest
        worst = max(worst, float(short[ok].max(initial=0.0)))
        assert not np.any(short[ok] > 2e-11), "an accepted eigenvalue lies below the largest root"
        weak = settled_on_some_simple_root(lam, slope, step)
        stray += int((weak & (short > 1e-6)).sum())
    print(f"{accepted} of {SWEEP_CHUNKS * SWEEP_CHUNK} accepted, the lowest {worst:.3g} of the root below it; the weaker test would "
          f"accept {stray} values on another root")
    assert accepted > 0.05 * SWEEP_CHUNKS * SWEEP_CHUNK  # (eps well away from 0: a simple largest root, and it is found)
    assert stray > 0
