"""The bars fc_kabsch_math.h is held to, against tests/kabsch_mp_ref.py, on the outputs of the probe of
csrc/fc_kabsch_math_probe.h -- whichever compilation of the header wrote them: tools/kabsch_math_host.cpp on the host
(tests/test_kabsch_math_cpu.py) or fc_debug_kabsch_math on the device (tests/test_gpu_kabsch_math.py).  Test
infrastructure: the product never imports it.

Every bar function asserts, and returns the worst figure it measured next to its bar ("What the math-header
tests pin down", quotes them)."""

import functools
import os
import re

import mpmath as mp
import numpy as np

import kabsch_mp_ref as kr
from oracle import cpu_ref as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = kr.EPS
mpf = mp.mpf


@functools.lru_cache(maxsize=None)
def slots():
    """name -> index: the enum KabschProbeSlot of csrc/fc_kabsch_math_probe.h, read from the header itself"""
    text = open(os.path.join(ROOT, "firecode_amd", "csrc", "fc_kabsch_math_probe.h")).read()
    body = text[text.index("enum KabschProbeSlot"):]
    body = body[:body.index("};")]
    body = re.sub(r"//[^\n]*", "", body)
    return {name: int(value) for name, value in re.findall(r"\b(k\w+)\s*=\s*(\d+)", body)}


def coordinate_scale(e):
    """the size of the coordinates in units of an ordinary molecule in Angstrom: what the absolute figures of the header
    and of tests/test_complete_eig_bound.py scale with"""
    if e.family == "scale":
        return e.claim["scale"]
    return 300.0 if e.family == "offset" else 1.0


class Records:
    """the ladder as records of the probe: every pair at its thresholds.  A knife-edge pair has its own; every other pair
    is screened at 0.25 A and just above / well below its own msd in each handedness, so that both verdicts are forced
    on every geometry.  pair[i]: index into the ladder; A_thr2[i]: the float64 the routine is given"""

    def __init__(self, ladder):
        self.ladder = ladder
        rows, pair = [], []
        for k, e in enumerate(ladder):
            B, gg = e.inputs
            r = e.ref
            if e.thr is not None:
                thr2 = [e.thr * e.thr]
            else:
                lo = float(min(r.msd, r.msd_m))
                thr2 = [0.0625, lo * (1 + 1e-9), lo / 1.5 * (1 - 1e-9), float(r.msd) * (1 + 1e-9), float(r.msd) / 1.5 * (1 - 1e-9)]
            for t2 in thr2:
                rows.append(np.concatenate([B.ravel(), [gg, float(e.A), e.A * t2]]))
                pair.append(k)
        self.data = np.ascontiguousarray(np.array(rows, dtype=np.float64))
        self.pair = np.array(pair)
        self.A_thr2 = self.data[:, 11].copy()
        self.first = np.array([int(np.flatnonzero(self.pair == k)[0]) for k in range(len(ladder))])  # one record per pair


@functools.lru_cache(maxsize=None)
def records():
    ladder = kr.kabsch_ladder()
    kr.check_ladder_claims(ladder)  # the families lie where they claim, before anything under test runs
    return Records(ladder)


# ---- small helpers in mpmath ----------------------------------------------------------------------------------------------
def _R_metrics(R9, ref):
    """R9: nine float64 (row-major) -> (det - 1, |R R^T - I|_max, deficit lambda1 - tr(R^T B), |R - R_true|_F) as floats"""
    R = [[mpf(float(R9[3 * x + y])) for y in range(3)] for x in range(3)]
    det = (R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) - R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0])
           + R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]))
    orth = max(abs(mp.fsum(R[x][k] * R[y][k] for k in range(3)) - (1 if x == y else 0)) for x in range(3) for y in range(3))
    tr = mp.fsum(R[x][y] * ref.B[x][y] for x in range(3) for y in range(3))
    diff = mp.sqrt(mp.fsum((R[x][y] - ref.R[x][y]) ** 2 for x in range(3) for y in range(3)))
    return float(det - 1), float(orth), float(ref.lam[0] - tr), float(diff)


def _rotation_of_q(Q):
    q = np.asarray(Q, dtype=np.float64)
    q = q / np.sqrt((q * q).sum())
    return np.array(kr.rotation_of(q), dtype=np.float64).ravel()


# ---- c1, c2: what the float64 LAPACK route of the oracle reaches on the same family -------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_rotation_ratios():
    """-> {family: (r1, r2)}: the worst optimality deficit / (eps S) and the worst |R - R_true|_F gap / (eps S) (pairs with
    gap > 1e-12 S) of oracle.get_alignment_matrix on each family of the ladder"""
    worst = {}
    for e in kr.kabsch_ladder():
        p, q = (e.p - e.p.mean(axis=0), e.q - e.q.mean(axis=0)) if e.center else (e.p, e.q)
        R = o.get_alignment_matrix(p, q)
        r = e.ref
        _, _, deficit, diff = _R_metrics(R.ravel(), r)
        S = float(r.S)
        r1 = deficit / (EPS * S) if S > 0 else 0.0
        r2 = diff * float(r.gap) / (EPS * S) if r.gap > 1e-12 * r.S else 0.0
        w = worst.setdefault(e.family, [0.0, 0.0])
        w[0], w[1] = max(w[0], r1), max(w[1], r2)
    return {f: tuple(w) for f, w in worst.items()}


def rotation_constants():
    """-> {family: (c1, c2)}: ten times the oracle's worst ratios, at least 16"""
    return {f: (max(16.0, 10.0 * r1), max(16.0, 10.0 * r2)) for f, (r1, r2) in oracle_rotation_ratios().items()}


# ---- the bars --------------------------------------------------------------------------------------------------------------
def bar_one_sided_eigenvalue(out, rec):
    """kabsch_lambda_upper and both outputs of kabsch_lambda_max_both<true> (and the plain form's) are never below the
    largest root (of B, respectively -B) by more than 1.1e-11 x the value; the bare Newton value likewise wherever
    kabsch_lambda_is_settled holds for it"""
    s = slots()
    worst, settled = 0.0, 0
    for k, e in enumerate(rec.ladder):
        row, r = out[rec.first[k]], e.ref
        checks = [("upper", row[s["kPrUpper"]], r.lam[0]), ("both+", row[s["kPrBothPlus"]], r.lam[0]),
                  ("both-", row[s["kPrBothMinus"]], r.lam_m[0]), ("plain", row[s["kPrBothPlain"]], r.lam[0])]
        if row[s["kPrSettled"]] != 0.0:
            settled += 1
            checks.append(("bare, settled", row[s["kPrLam"]], r.lam[0]))
        for name, value, truth in checks:
            assert np.isfinite(value), (e.family, name, value)
            short = float(truth - mpf(float(value)))
            if value > 0:
                worst = max(worst, short / value)
            assert short <= 1.1e-11 * value, (e.family, e.claim, name, value, float(truth), short)
    return {"worst (root - value) / value": worst, "bar": 1.1e-11, "settled": settled, "pairs": len(rec.ladder)}


def bar_sharp(out, rec):
    """kabsch_lambda_is_sharp true: |sqrt((Gp + Gq - 2 lambda) / A) - rmsd| <= 1e-11 scale + eps (Gp + Gq) / (A rmsd)"""
    s = slots()
    worst, n = 0.0, 0
    for k, e in enumerate(rec.ladder):
        row, r = out[rec.first[k]], e.ref
        if row[s["kPrSharp"]] == 0.0:
            continue
        n += 1
        gg = rec.data[rec.first[k], 9]
        got = np.sqrt(max(gg - 2.0 * row[s["kPrLam"]], 0.0) / e.A)
        err = abs(float(mpf(float(got)) - r.rmsd))
        bar = 1e-11 * coordinate_scale(e) + (EPS * gg / (e.A * float(r.rmsd)) if r.rmsd > 0 else np.inf)
        worst = max(worst, err / bar)
        assert err <= bar, (e.family, e.claim, err, bar)
    assert n > 0.4 * len(rec.ladder), n  # (the bar is not passed by declining: the degenerate families are half the ladder)
    return {"worst error / bar": worst, "certified": n, "pairs": len(rec.ladder)}


def bar_lean_eigenvalue(out, rec):
    """the lean form: rmsd from its eigenvalue within 5e-11 x the coordinate scale where A msd > 2e-10 (Gp + Gq)^2 / A;
    qcp_lean_converged wherever lambda1 - lambda2 > 1e-6 lambda1"""
    s = slots()
    worst, n = 0.0, 0
    for k, e in enumerate(rec.ladder):
        row, r = out[rec.first[k]], e.ref
        gg = rec.data[rec.first[k], 9]
        if r.lam[0] - r.lam[1] > 1e-6 * r.lam[0]:
            assert row[s["kPrLeanConverged"]] == 1.0, (e.family, e.claim, "not converged")
        if row[s["kPrRawOk"]] == 1.0:  # the four pairs of a lane (four copies here): the same flags, the same eigenvalue
            assert row[s["kPrLean4Ok"]] == 4.0 and row[s["kPrLean4Spread"]] <= 1e-12 * abs(row[s["kPrLeanLam"]]), (e.family, e.claim)
        # (the kernel takes the eigenvalue of the pairs its certificate accepts: k_simbits_screen_mfma<., 2, ., EIG> clears
        # ok4 below the threshold and stores nothing of a declined pair -- on a (nearly) double root, which the certificate
        # declines, the iteration's value is off by up to 1e-7)
        if row[s["kPrRawOk"]] == 1.0 and e.A * r.msd > mpf(2e-10) * r.G * r.G / e.A:
            n += 1
            got = np.sqrt(max(gg - 2.0 * row[s["kPrLeanLam"]], 0.0) / e.A)
            err = abs(float(mpf(float(got)) - r.rmsd)) / coordinate_scale(e)
            worst = max(worst, err)
            assert err <= 5e-11, (e.family, e.claim, err)
    return {"worst |rmsd error| / scale": worst, "bar": 5e-11, "pairs above the kernel's threshold": n}


def bar_fp64_screen(out, rec):
    """kabsch_may_be_below, plain and ENANT: never false for a true msd below thr^2 (the smaller msd of the two
    handednesses under ENANT); always false for msd >= 1.5 thr^2 where the pair is not tiny and A thr^2 >= 1e-3 s"""
    s = slots()
    counts = {"must keep": 0, "must drop": 0, "free": 0}
    for i in range(len(rec.data)):
        e = rec.ladder[rec.pair[i]]
        r = e.ref
        A_thr2, sg = rec.A_thr2[i], 0.5 * rec.data[i, 9]
        tiny = not (A_thr2 < 0.5 * sg)
        for slot, msd in (("kPrBelow", r.msd), ("kPrBelowEnant", min(r.msd, r.msd_m))):
            verdict = out[i, s[slot]]
            assert verdict in (0.0, 1.0)
            if e.A * msd < mpf(float(A_thr2)):
                counts["must keep"] += 1
                assert verdict == 1.0, (e.family, e.claim, slot, "a similar pair is dropped", float(msd), A_thr2 / e.A)
            elif e.A * msd >= 1.5 * mpf(float(A_thr2)) and not tiny and A_thr2 >= 1e-3 * sg:
                counts["must drop"] += 1
                assert verdict == 0.0, (e.family, e.claim, slot, "a clearly dissimilar pair is kept", float(msd), A_thr2 / e.A)
            else:
                counts["free"] += 1
    assert counts["must keep"] > 1000 and counts["must drop"] > 200, counts
    return counts


# which outputs hold a rotation, and the certificate each is used under (None: always)
def _rotations_of(row, s):
    yield "kabsch_rotation", None, row[s["kPrJacobiR"]:s["kPrJacobiR"] + 9]
    if row[s["kPrQcpOk"]] != 0.0:
        yield "kabsch_rotation_qcp", "kPrQcpOk", row[s["kPrQcpR"]:s["kPrQcpR"] + 9]
    if row[s["kPrQuatOk"]] != 0.0:
        yield "kabsch_quaternion_qcp", "kPrQuatOk", _rotation_of_q(row[s["kPrQuatQ"]:s["kPrQuatQ"] + 4])
    if row[s["kPrLeanOk"]] != 0.0:
        yield "kabsch_quaternion_qcp_lean + rotation_from_quaternion", "kPrLeanOk", row[s["kPrRotOfQ"]:s["kPrRotOfQ"] + 9]
        yield "neg_rotation_from_quaternion", "kPrLeanOk", -row[s["kPrNegRotOfQ"]:s["kPrNegRotOfQ"] + 9]
    if row[s["kPrRawOk"]] != 0.0:
        yield "qcp_lean_quaternion_raw + neg_rotation_from_raw_quaternion", "kPrRawOk", -row[s["kPrNegRotRaw"]:s["kPrNegRotRaw"] + 9]
    if row[s["kPrCol0Ok"]] != 0.0:
        yield "qcp_lean_quaternion_col0", "kPrCol0Ok", _rotation_of_q(row[s["kPrCol0Q"]:s["kPrCol0Q"] + 4])


def bar_rotations(out, rec):
    """det R = 1 and |R R^T - I| <= 1e-14; optimality deficit lambda1 - tr(R^T B) <= c1 eps S on every pair;
    |R - R_true|_F <= c2 eps S / gap where gap > 1e-12 S -- c1, c2 per family from the oracle's own ratios"""
    s, consts = slots(), rotation_constants()
    worst = {}
    for k, e in enumerate(rec.ladder):
        row, r = out[rec.first[k]], e.ref
        c1, c2 = consts[e.family]
        S = float(r.S)
        for name, _, R9 in _rotations_of(row, s):
            assert np.all(np.isfinite(R9)), (e.family, e.claim, name)
            det1, orth, deficit, diff = _R_metrics(R9, r)
            w = worst.setdefault((name, e.family), [0.0, 0.0, 0.0, 0])
            w[3] += 1
            w[0] = max(w[0], orth, abs(det1))
            assert abs(det1) <= 1e-14 and orth <= 1e-14, (e.family, e.claim, name, det1, orth)
            if S > 0:
                w[1] = max(w[1], deficit / (EPS * S))
                assert deficit <= c1 * EPS * S, (e.family, e.claim, name, "deficit / (eps S)", deficit / (EPS * S), c1)
            if r.gap > 1e-12 * r.S:
                ratio = diff * float(r.gap) / (EPS * S)
                w[2] = max(w[2], ratio)
                assert ratio <= c2, (e.family, e.claim, name, "|R - R_true| gap / (eps S)", ratio, c2)
    return {key: {"orthogonality": w[0], "deficit / (eps S)": w[1], "|dR| gap / (eps S)": w[2], "rotations": w[3]}
            for key, w in worst.items()}


def bar_certificates(out, rec):
    """nothing passes by declining: the QCP forms certify every pair whose gap product is ten times their threshold (as
    the header states it, on the reference's numbers); column 0 certifies every such pair with q0^2 >= 0.7 and never one
    with q0^2 <= 0.5"""
    s = slots()
    n = {"kabsch_rotation_qcp": 0, "kabsch_quaternion_qcp": 0, "qcp_lean_quaternion_raw": 0, "col0 >= 0.7": 0, "col0 <= 0.5": 0}
    for k, e in enumerate(rec.ladder):
        row, r = out[rec.first[k]], e.ref
        B = r.B
        # scale of kabsch_rotation_qcp: |lambda| + |Sxx| + |Syy| + |Szz| + the six off-diagonal entries of K
        offd = [B[1][2] - B[2][1], B[2][0] - B[0][2], B[0][1] - B[1][0], B[0][1] + B[1][0], B[2][0] + B[0][2], B[1][2] + B[2][1]]
        scale = abs(r.lam[0]) + abs(B[0][0]) + abs(B[1][1]) + abs(B[2][2]) + mp.fsum(abs(v) for v in offd)
        if r.gap_product >= 10 * mpf(2e-3) * scale ** 3 and scale > 0:
            for name, slot in (("kabsch_rotation_qcp", "kPrQcpOk"), ("kabsch_quaternion_qcp", "kPrQuatOk")):
                n[name] += 1
                assert row[s[slot]] == 1.0, (e.family, e.claim, name, "declines a clearly simple eigenvalue")
        simple = r.n2 > 0 and r.gap_product >= 10 * mpf(2e-3) * 27 * r.n2 * mp.sqrt(r.n2)
        if simple:
            n["qcp_lean_quaternion_raw"] += 1
            assert row[s["kPrRawOk"]] == 1.0 and row[s["kPrLeanOk"]] == 1.0, (e.family, e.claim, "the lean form declines")
        q0sq = r.q[0] ** 2
        if simple and q0sq >= mpf("0.7"):
            n["col0 >= 0.7"] += 1
            assert row[s["kPrCol0Ok"]] == 1.0, (e.family, e.claim, "column 0 declines at q0^2 =", float(q0sq))
        if q0sq <= mpf("0.5"):
            n["col0 <= 0.5"] += 1
            assert row[s["kPrCol0Ok"]] == 0.0, (e.family, e.claim, "column 0 certifies at q0^2 =", float(q0sq))
        if row[s["kPrCol0Ok"]] == 1.0:  # and where it certifies, it is the general form's own bits
            assert row[s["kPrRawOk"]] == 1.0 and row[s["kPrCol0Nq"]] == row[s["kPrRawNq"]]
            assert np.array_equal(row[s["kPrCol0Q"]:s["kPrCol0Q"] + 4], row[s["kPrRawQ"]:s["kPrRawQ"] + 4])
    assert all(v >= 50 for v in n.values()), n
    return n


def all_bars(out, rec):
    """every bar -> {bar: figures}"""
    return {"one-sided eigenvalue": bar_one_sided_eigenvalue(out, rec), "sharp": bar_sharp(out, rec),
            "lean eigenvalue": bar_lean_eigenvalue(out, rec), "fp64 screen": bar_fp64_screen(out, rec),
            "rotations": bar_rotations(out, rec), "certificates": bar_certificates(out, rec)}
