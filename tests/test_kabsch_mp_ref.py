"""The arbitrary-precision reference of tests/kabsch_mp_ref.py checked against what is known another way -- the closed forms
of tests/degenerate_ref.py, its own identities, the float64 oracle on well-conditioned pairs -- and then the oracle and
the tolerance the GPU suite applies (oracle.rotation_error_bound_batch) checked against the reference on the whole ladder:
the constant (2 A + 8) of that bound had never been compared with anything more precise than float64.  No GPU."""

import mpmath as mp
import numpy as np
import pytest

import degenerate_ref as dg
import kabsch_mp_ref as kr
from oracle import cpu_ref as o

mpf = mp.mpf


@pytest.fixture(scope="module")
def ladder():
    L = kr.kabsch_ladder()
    kr.check_ladder_claims(L)
    return L


@pytest.mark.parametrize("base_name", ["full", "planar", "line"])
def test_reference_reproduces_the_closed_forms_of_the_scaled_family(base_name):
    """conformer i = a_i b under a rigid motion: rmsd(i, j) = |a_i - a_j| rms(b), max deviation |a_i - a_j| max_a |b_a|,
    whatever the rank of b (the rigid motions are rounded to float64: 1e-15 A on coordinates of a few A)"""
    base = dg.scaled_base(base_name)
    X, a = dg.scaled_family(base, np.array([1e-8, 3e-5, 1e-3, 0.05, 0.25, 0.6]), seed=3)
    want_r, want_m = dg.scaled_rmsd(base, a), dg.scaled_maxdev(base, a)
    for i, j in [(0, 6), (1, 6), (2, 5), (3, 4), (4, 6), (5, 0), (2, 2)]:
        r = kr.reference(X[i], X[j], center=True)
        assert abs(float(r.rmsd) - want_r[i, j]) <= 1e-13, (i, j, float(r.rmsd), want_r[i, j])
        assert abs(float(r.maxdev) - want_m[i, j]) <= 1e-13, (i, j, float(r.maxdev), want_m[i, j])


def test_reference_is_consistent_with_itself(ladder):
    """the eigenvalues are the roots of the polynomial the header uses, they sum to zero, R is a rotation that reaches
    tr(R^T B) = lambda1, the explicit sum over the atoms equals (Gp + Gq) - 2 lambda1, and -B has the negated spectrum"""
    for e in ladder[::37]:
        r = e.ref
        S = r.S if r.S > 0 else mpf(1)
        assert abs(mp.fsum(r.lam)) <= mpf(10) ** -50 * S
        for lam in r.lam:
            assert abs(r.poly(lam)[0]) <= mpf(10) ** -45 * S ** 4
            assert abs(r.poly(-lam, mirror=True)[0]) <= mpf(10) ** -45 * S ** 4
        assert r.gap_product >= 0 and abs(r.poly(r.lam[0])[1] - r.gap_product) <= mpf(10) ** -45 * S ** 3
        R = r.R
        for x in range(3):
            for y in range(3):
                assert abs(mp.fsum(R[x][k] * R[y][k] for k in range(3)) - (1 if x == y else 0)) <= mpf(10) ** -50
        assert abs(mp.fsum(R[x][y] * r.B[x][y] for x in range(3) for y in range(3)) - r.lam[0]) <= mpf(10) ** -45 * S
        p = np.asarray(e.p, dtype=np.float64)
        q = np.asarray(e.q, dtype=np.float64)
        pr, qr = kr._mpf_rows(p), kr._mpf_rows(q)
        if e.center:
            pr, qr = kr._centred(pr), kr._centred(qr)
        ssq = mp.fsum((a[x] - mp.fsum(R[x][k] * b[k] for k in range(3))) ** 2 for a, b in zip(pr, qr) for x in range(3))
        assert abs(ssq - (r.G - 2 * r.lam[0])) <= mpf(10) ** -45 * S
        assert r.lam_m[0] == -r.lam[3] and r.msd_m >= 0


def test_reference_agrees_with_the_oracle_on_well_conditioned_pairs(ladder):
    n = 0
    for e in ladder:
        if e.family not in ("noisy", "unrelated", "half-turn", "knife") or e.A < 4 or not e.ref.gap > 1e-2 * e.ref.S:
            continue
        n += 1
        rmsd, maxdev = o.rmsd_and_max(e.p, e.q, center=e.center)
        assert abs(rmsd - float(e.ref.rmsd)) < 1e-13 and abs(maxdev - float(e.ref.maxdev)) < 1e-13, (e.family, e.claim)
    assert n > 300


# ---- the oracle and its bound on the whole ladder ---------------------------------------------------------------------------
def _oracle_figures(ladder, family):
    """-> per pair of the family: (rmsd error / scale, max-deviation error, bound, the reference's gap / S)"""
    rows = []
    for e in ladder:
        if e.family != family:
            continue
        rmsd, maxdev = o.rmsd_and_max(e.p, e.q, center=e.center)
        bound = float(o.rotation_error_bound_batch(e.p[None], e.q[None], center=e.center)[0])
        scale = e.claim["scale"] if family == "scale" else 300.0 if family == "offset" else 1.0
        gap_rel = float(e.ref.gap / e.ref.S) if e.ref.S > 0 else 0.0
        rows.append((abs(rmsd - float(e.ref.rmsd)) / scale, abs(maxdev - float(e.ref.maxdev)), bound, gap_rel))
    return np.array(rows)


@pytest.mark.parametrize("family", kr.FAMILIES)
def test_oracle_and_its_bound_against_the_reference(ladder, family):
    """oracle.rmsd_and_max within 1e-13 (x the coordinate scale) of the reference; its max deviation within
    rotation_error_bound_batch wherever that is finite; the bound infinite exactly where the reference's gap is below
    1e-12 S.  Printed: the worst ratio error / bound, which says how loose the GPU suite's tolerance is on the family
    ("What the math-header tests pin down")."""
    f = _oracle_figures(ladder, family)
    assert len(f) > 0
    rmsd_err, dev_err, bound, gap_rel = f.T
    finite = np.isfinite(bound)
    ratio = dev_err[finite] / bound[finite]
    print(f"{family}: {len(f)} pairs, rmsd error <= {rmsd_err.max():.3g}, bound finite on {int(finite.sum())}, worst max-deviation "
          f"error / bound {ratio.max(initial=0.0):.3g}, median {np.median(ratio) if ratio.size else 0.0:.3g}")
    assert rmsd_err.max() <= 1e-13
    assert np.array_equal(~finite, ~(gap_rel >= 1e-12)), "the bound is infinite exactly where the rotation is not unique"
    assert np.all(dev_err[finite] <= bound[finite])
