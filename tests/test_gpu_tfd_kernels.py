"""The TFD first-match kernels of firecode_amd/csrc/fc_prune.hip (k_tfd_simbits, k_tfd_first_match, k_tfd_window_bounds,
k_tfd_first_match_rest, k_tfd_first_match_merge, k_tfd_pack_u16, k_tfd_window_bounds_f64, k_tfd_first_match_dense_u16,
k_tfd_first_match_walk_u16) against the literal NumPy formula (tests/tfd_ref.py) at the edges where a skip decision can
be wrong by one column or one window: the +-180 seam in every box angle, windows that straddle it, the boundaries of
phases, windows and chunks, the zero padding behind column N, every compile-time class of Q and NumPy's summation
order to the last bit, the launcher's own choice of form, the 16-bit path's angle range, and extreme thresholds.

Every comparison is exact (integers and bits).  Every case first asserts, from the reference alone, that it exercises
what its name says, and then, through fc_tfd_last_form, that the device form it names is the one that ran."""

import functools

import numpy as np
import pytest

import tfd_ref as R
from oracle import cpu_ref as o

pytestmark = pytest.mark.gpu

# "all forms": (FC_TFD_LOOKAHEAD, FC_TFD_U16)
FORMS = {"one_phase": ("0", None), "f32_look64": ("64", "0"), "u16_look64": ("64", None), "u16_look32": ("32", None)}


def _knobs(monkeypatch, look, u16):
    for name, v in (("FC_TFD_LOOKAHEAD", look), ("FC_TFD_U16", u16)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)


def _first_match(tf, thresh):
    from firecode_amd import _lib as L

    tf = np.ascontiguousarray(tf, dtype=np.float64)
    fm = np.full(len(tf), -7, dtype=np.int64)
    L.call("fc_tfd_first_match", L.pf(tf), tf.shape[0], tf.shape[1], float(thresh), L.pi(fm))
    form, n_open = L.tfd_last_form()
    return fm, form, n_open


def _check_form(name, n, form, n_open):
    """the form a set of knobs must take at n rows (two phases need n > 8 x look-ahead)"""
    look, u16 = FORMS[name]
    if int(look) == 0 or n <= 8 * int(look):
        assert (form, n_open) == (R.FORM_ONE_PHASE, 0), (name, form, n_open)
    elif u16 == "0":
        assert form == R.FORM_F32_REST, (name, form)
    else:
        assert form == R.FORM_U16_DENSE | (R.FORM_U16_WALK if n_open > 0 else 0), (name, form, n_open)


def _all_forms(monkeypatch, tf, thresh, ref, want_open=False):
    """fc_tfd_first_match under every form == ref"""
    for name in FORMS:
        _knobs(monkeypatch, *FORMS[name])
        fm, form, n_open = _first_match(tf, thresh)
        _check_form(name, len(tf), form, n_open)
        if want_open and form != R.FORM_ONE_PHASE:
            assert n_open > 0, name
        bad = np.flatnonzero(fm != ref)
        assert len(bad) == 0, (name, bad[:10], fm[bad[:10]], ref[bad[:10]])


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


# ---- the arrays and their references, computed once and shared (read-only) --------------------------------------
@functools.lru_cache(maxsize=None)
def _case_a(Q):
    tf, pos, neg = R.wrap_case(Q)
    (ref,) = _frozen(R.first_match(tf, 10.0))
    _frozen(tf)
    return tf, pos, neg, ref


@functools.lru_cache(maxsize=None)
def _case_b(Q):
    tf, planted = R.seam_windows_case(Q)
    (ref,) = _frozen(R.first_match(tf, 10.0))
    _frozen(tf)
    return tf, planted, ref


@functools.lru_cache(maxsize=None)
def _case_c():
    tf, plants, sweep = R.boundary_case()
    (ref,) = _frozen(R.first_match(tf, 10.0))
    _frozen(tf)
    return tf, plants, sweep, ref


@functools.lru_cache(maxsize=None)
def _case_f():
    tf, planted, check = R.launcher_case()
    ref = R.first_match(tf, 1.0, rows=check)
    _frozen(tf, check, ref)
    return tf, planted, check, ref


QS_AB = [1, 2, 4, 5, 8, 9, 12]


# ---- a ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", QS_AB)
def test_wrap_in_every_box_angle(fc, monkeypatch, Q):
    """a. One pair per angle q < min(Q, 9) whose whole offset (4.0) sits in angle q across the seam, 179.x against
    -179.x, the partner 3 000 - 5 000 rows later (many windows and boxes on); one pair spread over all angles; one
    negative control per q (10.5).  For Q >= 9 angle 8 is in no box and in no 16-bit sum.  Grid background (dense
    for Q <= 2, where no 6 000 rows are 10 degrees apart)."""
    tf, pos, neg, ref = _case_a(Q)
    assert tf.shape == (6000, Q)
    for i, j, ang, s in pos:
        assert ref[i] == j and s < 10.0 and R.opposite_sides(tf, i, j, ang) and np.abs(tf[i, ang]).min() > 176.0
    for i, j, ang, s in neg:
        assert ref[i] != j and s > 10.0 and R.opposite_sides(tf, i, j, ang) and (Q < 2 or ref[i] == -1)
    assert sorted(p[2][0] for p in pos if len(p[2]) == 1) == sorted(p[2][0] for p in neg) == list(range(min(Q, 9)))
    _all_forms(monkeypatch, tf, 10.0, ref, want_open=True)


# ---- b ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", QS_AB)
def test_windows_that_straddle_the_seam(fc, monkeypatch, Q):
    """b. Three windows of 256 columns whose first angle alternates between +179.5 and -179.5 (box 359 wide: counted as
    the whole circle) and one of +-179.25 (358.5 wide: just under the cut, a box still); early rows are near copies of
    columns inside those windows and right beside them, some across the seam from their column."""
    tf, planted, ref = _case_b(Q)
    for w, v in R.SEAM_WINDOWS:
        a0 = tf[w * 256:(w + 1) * 256, 0]
        assert a0.max() - a0.min() == 2 * v and (2 * v >= 359.0) == (v == 179.5)
    inside = lambda c: any(w * 256 <= c < (w + 1) * 256 for w, _ in R.SEAM_WINDOWS)  # noqa: E731
    hits = [int(ref[i]) for i, j, w, total in planted if total < 10.0]
    assert all(h >= 0 for h in hits) and sum(inside(h) for h in hits) >= (12 if Q >= 4 else 1)
    if Q >= 4:  # (match-free background: the planted column is the only partner)
        assert sum(ref[i] == j for i, j, w, total in planted if total < 10.0) >= 15  # (of 20: window rows can resemble each other)
        assert all(ref[i] == -1 for i, j, w, total in planted if total > 10.0)
        edges = [{int(ref[i]) - w * 256 for i, j, ww, total in planted if ww == w} & {-1, 0, 255, 256} for w, _ in R.SEAM_WINDOWS]
        # first matches on the first and last column of the windows and on the columns right beside them
        assert all(len(e) >= 3 for e in edges) and set().union(*edges) == {-1, 0, 255, 256}
        across = [(i, j) for i, j, w, total in planted if ref[i] == j and inside(j) and tf[i, 0] * tf[j, 0] < 0]
        assert len(across) >= 3
    _all_forms(monkeypatch, tf, 10.0, ref, want_open=True)


# ---- c ---------------------------------------------------------------------------------------------------------
def test_partners_on_phase_window_and_chunk_boundaries(fc, monkeypatch):
    """c. N = 9 000, Q = 3, look-ahead 64: the dense phase of block i0 ends at column i0 + 128.  Rows at lanes 0, 1, 62,
    63 with their ONLY partner at i0 + 127 / 128 / 129, at multiples of 256 and of 1 024 -1 / +0 / +1, at N - 1; and
    1 300 rows whose only partner is exactly 1 ... 1 300 columns later, so that whatever `from` column the look-ahead
    kernel hands over, some row has its partner on it."""
    tf, plants, sweep, ref = _case_c()
    assert tf.shape == (9000, 3)
    assert all(ref[i] == j for i, j, _, _ in plants) and all(ref[i] == j for i, j in sweep)
    assert {(k, d) for _, _, k, d in plants} >= {("dense", -1), ("dense", 0), ("dense", 1), ("win0", -1), ("win0", 0),
                                                 ("win0", 1), ("box0", -1), ("box0", 0), ("box0", 1), ("last", 0)}
    assert 8999 in [j for _, j, _, _ in plants]
    assert (ref >= 0).sum() < 1400  # (everything else is open to the end: the leftover lists are long)
    _all_forms(monkeypatch, tf, 10.0, ref, want_open=True)


# ---- d ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [1, 8])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 257, 1023, 1025, 2049])
def test_zero_rows_next_to_the_zero_padding(fc, monkeypatch, n, Q):
    """d. The last one, two or three rows are all-zero fingerprints -- equal to the padding behind column N -- and so is
    an earlier row: it must find the first of them, the last row nothing, and nobody a column >= N."""
    rng = np.random.default_rng(1000 * Q + n)
    t = min(1 + n % 3, n)
    tf = rng.choice([-1.0, 1.0], size=(n, Q)) * rng.uniform(20.0, 180.0, size=(n, Q))
    tf[n - t:] = 0.0
    early = (n - t) // 2 if n - t >= 1 else None
    if early is not None:
        tf[early] = 0.0
    ref = R.first_match(tf, 10.0)
    assert ref[n - 1] == -1 and (early is None or ref[early] == n - t) and (ref < n).all()
    assert [int(r) for r in ref[n - t:]] == [n - t + k + 1 for k in range(t - 1)] + [-1]
    forms = ["one_phase"] + (["u16_look32", "f32_look32"] if n > 8 * 32 else [])
    for name in forms:
        _knobs(monkeypatch, "0" if name == "one_phase" else "32", "0" if name == "f32_look32" else None)
        fm, form, n_open = _first_match(tf, 10.0)
        assert form == {"one_phase": 1, "f32_look32": 2}.get(name, 4 | (8 if n_open else 0)), (name, form)
        assert (fm < n).all() and fm[n - 1] == -1 and np.array_equal(fm, ref), name


def test_empty_fingerprints(fc, monkeypatch):
    """d. Q = 0: NumPy's empty sum is 0, so every row matches its successor for thresh > 0 and none for thresh <= 0"""
    from firecode_amd import _lib as L

    tf = np.zeros((5, 0))
    for thresh, want in ((10.0, [1, 2, 3, 4, -1]), (5e-324, [1, 2, 3, 4, -1]), (0.0, [-1] * 5), (-1.0, [-1] * 5)):
        assert R.first_match(tf, thresh).tolist() == want
        for name in FORMS:
            _knobs(monkeypatch, *FORMS[name])
            fm = np.full(5, -7, dtype=np.int64)
            L.call("fc_tfd_first_match", None, 5, 0, float(thresh), L.pi(fm))
            assert fm.tolist() == want, (thresh, name)


# ---- e ---------------------------------------------------------------------------------------------------------
QS_E = [1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 33, 64, 127, 128]


def _case_e(Q):
    """600 rows of a match-free grid with 40 pairs planted at ONE total: their sums, as NumPy adds them, differ in the
    last bits only.  Near partners (dense phase / look-ahead) and far ones (walk / chunks), some across the seam."""
    rng = np.random.default_rng(300 + Q)
    total = 0.2 if Q == 1 else 4.0
    tf = (R.lattice(600, 1, 0.55, 21, dims=1) if Q == 1 else R.lattice(25, Q, 13.0, 21)[:600]).copy()
    rows = rng.permutation(250)[:40]
    pairs = []
    seen0 = set()
    for k, i in enumerate(rows):
        j = 300 + int(i) if k % 2 else 599 - int(np.searchsorted(np.sort(rows), i))  # (distinct columns: 300 ... 549 / 560 ... 599)
        if k % 4 == 0 and Q >= 2 and tf[i, 0] not in seen0 and len(seen0) < 8:
            seen0.add(tf[i, 0])  # (rows moved to the seam in the last angle stay apart in the first)
            tf[i, Q - 1] = rng.choice([-1.0, 1.0]) * (180.0 - 1e-3)
        pairs.append((int(i), j, R.plant(tf, int(i), j, total, rng)))
    for k in range(0, 40, 5):  # near partners: within the dense phase / the look-ahead
        i, _, _ = pairs[k]
        j = i + 1 + k % 3
        while j in {p[0] for p in pairs} | {p[1] for p in pairs}:
            j += 1
        pairs[k] = (i, j, R.plant(tf, i, j, total, rng))
    return tf, pairs


@pytest.mark.parametrize("Q", QS_E)
def test_q_classes_and_numpys_order_to_the_last_bit(fc, monkeypatch, Q):
    """e. Every compile-time class of Q (QT = 1 ... 8 of the 16-bit kernels with their dword counts, 1 ... 16 of the fp32
    ones, the generic QT = 0 up to the limit of 128): 40 pairs whose sums sit within a few ulp of each other, thresh =
    the sum s of one of them (that pair is strictly not similar) and thresh = nextafter(s) (it is).  A kernel that adds
    in another order than np.sum flips about half of them."""
    fcm = fc.torsion_module
    tf, pairs = _case_e(Q)
    sums = sorted(p[2] for p in pairs)
    s = sums[len(sums) // 2]
    assert sums[-1] - sums[0] < 1e-12 and (Q < 2 or any(tf[i, Q - 1] * tf[j, Q - 1] < 0 for i, j, _ in pairs))
    assert {j - i for i, j, _ in pairs} & {1, 2, 3} and max(j - i for i, j, _ in pairs) > 300
    for thresh in (s, float(np.nextafter(s, np.inf))):
        ref = R.first_match(tf, thresh)
        for i, j, sk in pairs:
            assert (ref[i] == j) == (sk < thresh)
        assert any(ref[i] == j for i, j, sk in pairs if sk == s) == (thresh > s)
        if Q > 2:
            n_sim = sum(ref[i] == j for i, j, _ in pairs)
            assert 0 < n_sim < 40 or thresh > s, n_sim
        _all_forms(monkeypatch, tf, thresh, ref, want_open=True)
        S = R.simbits(tf, thresh)
        bits = R.bits_to_bool(fcm.tfd_simbits(tf, thresh), len(tf))
        assert np.array_equal(bits[:, :len(tf)], S) and not bits[:, len(tf):].any()


def test_more_than_128_angles_are_refused(fc):
    """e. np.sum recurses pairwise beyond 128 elements and the kernels' order no longer is NumPy's: refused"""
    from firecode_amd import _lib as L

    tf = np.zeros((3, 129))
    fm = np.zeros(3, dtype=np.int64)
    for fn in (lambda: L.call("fc_tfd_first_match", L.pf(tf), 3, 129, 10.0, L.pi(fm)),
               lambda: fc.torsion_module.tfd_simbits(tf, 10.0),
               lambda: fc.torsion_module.tfd_similarity(tf[0], tf[1]),
               lambda: fc.torsion_module.prune_tfd_from_tf_mat(tf)):
        with pytest.raises(fc.FirecodeHipInputError) as e:
            fn()
        assert e.value.code == L.FC_E_LIMIT and "128" in str(e.value)


# ---- f ---------------------------------------------------------------------------------------------------------
def test_the_launchers_own_choice(fc, monkeypatch):
    """f. No knob: 66 049 rows (the 257 x 257 grid of step 1.4, Q = 2, thresh 1.0) take the 16-bit dense phase of 128
    columns and the walk; FC_TFD_U16=0 the fp32 look-ahead of 4 096 and chunks of 65 536 columns, the second holding
    513.  Pairs at 1.0 + e for e = 0 ... +-0.5 at gaps 3 ... 40 000, across column 65 536, across the seam.  Reference:
    the rewritten rows, every row similar to one of them, 400 sampled rows; every other row is -1 by the grid argument."""
    tf, planted, check, ref = _case_f()
    n = len(tf)
    assert n == 66049 >= R.TWO_PHASE_N and n - R.CHUNK == 513
    at = {int(r): k for k, r in enumerate(check)}
    matched = [ref[at[i]] == j for i, j in planted]
    assert 30 < sum(matched) < len(planted) - 30  # both outcomes
    assert sum(m for m, (i, j) in zip(matched, planted) if i < R.CHUNK <= j) >= 3
    assert sum(m for m, (i, j) in zip(matched, planted) if np.any(tf[i] * tf[j] < -170.0 ** 2)) >= 3  # across the seam
    assert {j - i for (i, j), m in zip(planted, matched) if m} >= set(R.F_GAPS)
    sample = np.setdiff1d(np.random.default_rng(4).permutation(n)[:400], check)
    assert (R.first_match(tf, 1.0, rows=sample) == -1).all()
    want = np.full(n, -1, dtype=np.int64)
    want[check] = ref
    for u16, form_want in ((None, R.FORM_U16_DENSE | R.FORM_U16_WALK), ("0", R.FORM_F32_REST)):
        _knobs(monkeypatch, None, u16)
        fm, form, n_open = _first_match(tf, 1.0)
        assert form == form_want and n_open > 60000, (u16, form, n_open)
        bad = np.flatnonzero(fm != want)
        assert len(bad) == 0, (u16, bad[:10], fm[bad[:10]], want[bad[:10]])


# ---- g ---------------------------------------------------------------------------------------------------------
def test_angle_range_of_the_16_bit_path(fc, monkeypatch):
    """g. Angles in (180, 270] and exactly +-270 are accepted by the 16-bit kernels (no refusal in the form); the next
    double beyond 270, +-inf and NaN are refused and the fp32 kernels redo the array; +180 against -180 and -0.0 against
    +0.0 are the same angle; 300 against -100 and +260 as the reference has it."""
    _knobs(monkeypatch, "64", None)

    def pair(tf, i, j, a, b, off):
        tf[i, 1:3] += off  # (half a grid step off the grid in two angles: further than the threshold from every other row)
        tf[j] = tf[i]
        tf[i, 0], tf[j, 0] = a, b
        tf[j, 1] += 1.5

    tf = R.background(1500, 3).copy()  # (grid of step 25)
    pair(tf, 10, 900, 180.0, -180.0, 12.5)
    pair(tf, 20, 30, -0.0, 0.0, 12.5)
    pair(tf, 40, 1400, 269.0, -89.5, 12.5)    # |d| = 358.5 -> 1.5
    pair(tf, 50, 1300, 270.0, -270.0, 12.5)   # |d| = 540 -> 180: not similar
    pair(tf, 60, 1200, -270.0, 91.0, 12.5)    # |d| = 361 -> 1
    pair(tf, 70, 1100, 200.0, -165.0, 12.5)   # |d| = 365 -> 5
    pair(tf, 80, 1000, 181.0, 186.0, 12.5)
    assert np.abs(tf).max() == R.U16_MAX_ANGLE
    ref = R.first_match(tf, 10.0)
    assert [int(ref[i]) for i in (10, 20, 40, 50, 60, 70, 80)] == [900, 30, 1400, -1, 1200, 1100, 1000]
    fm, form, n_open = _first_match(tf, 10.0)
    assert form == (R.FORM_U16_DENSE | R.FORM_U16_WALK) and n_open > 0
    assert np.array_equal(fm, ref)
    beyond = float(np.nextafter(R.U16_MAX_ANGLE, np.inf))
    for bad in (beyond, -beyond, np.inf, -np.inf, np.nan):
        for where in ((700, 0), (1499, 2)):
            tf2 = tf.copy()
            tf2[where] = bad
            ref2 = R.first_match(tf2, 10.0)
            fm, form, n_open = _first_match(tf2, 10.0)
            assert form == (R.FORM_U16_REFUSED | R.FORM_F32_REST), (bad, form)
            assert np.array_equal(fm, ref2), bad
    # 300 against -100 and +260: deltas 40 and 40 (|a - b| = 400 and 40); against -250: |d| = 550 -> 190, where the
    # circular distance is 170 -- the reference as it is
    tf3 = R.lattice(5, 4, 60.0, 5, dims=4)[:600].copy()
    pair(tf3, 5, 500, 300.0, -100.0, 30.0)
    pair(tf3, 6, 501, 300.0, 260.0, 30.0)
    pair(tf3, 7, 502, 300.0, -250.0, 30.0)
    for thresh, want in ((10.0, [-1, -1, -1]), (45.0, [500, 501, -1])):
        ref3 = R.first_match(tf3, thresh)
        assert [int(ref3[i]) for i in (5, 6, 7)] == want
        fm, form, _ = _first_match(tf3, thresh)
        assert form == (R.FORM_U16_REFUSED | R.FORM_F32_REST) and np.array_equal(fm, ref3), thresh
    tf4 = tf3[[7, 502]].copy()  # the pair alone, one phase: similar below 191.5, not below 175
    for thresh, want in ((175.0, [-1, -1]), (192.0, [1, -1])):
        assert R.first_match(tf4, thresh).tolist() == want
        assert _first_match(tf4, thresh)[0].tolist() == want


# ---- h ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thresh", [0.0, -1.0, 5e-324, 1439.9, 1441.0, 2000.0, 1e300])
def test_extreme_thresholds(fc, monkeypatch, thresh):
    """h. Nothing is below 0; only exact copies are below 5e-324; 8 angles sum to at most 1 440, so an antipodal pair is
    not below 1 439.9 and everything is below 1 441 (first match = the next row); at 2 000 the 16-bit threshold is
    capped at 300 000 units; 1e300 is inf in fp32."""
    rng = np.random.default_rng(77)
    n = 1500
    tf = rng.uniform(-180, 180, size=(n, 8))
    tf[903] = tf[900]          # exact copies: sum 0, near
    tf[1400] = tf[200]         # ... and far
    tf[n - 1] = np.where(tf[n - 2] < 0, tf[n - 2] + 180.0, tf[n - 2] - 180.0)  # antipodal: every delta is 180
    ref = R.first_match(tf, thresh)
    assert R.pair_sum(tf[n - 2], tf[n - 1]) == 1440.0
    if thresh <= 0:
        assert (ref == -1).all()
    elif thresh < 1:
        assert ref[900] == 903 and ref[200] == 1400 and (ref >= 0).sum() == 2
    elif thresh < 1440:
        assert ref[n - 2] == -1 and (ref[:n - 2] >= 0).all()
    else:
        assert np.array_equal(ref[:n - 1], np.arange(1, n))
    _all_forms(monkeypatch, tf, thresh, ref)


# ---- i ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [1, 7, 8, 9, 128])
@pytest.mark.parametrize("n", [1, 2, 64, 65, 130, 1000])
def test_simbits_row_ranges_tail_word_and_first_match(fc, monkeypatch, n, Q):
    """i. k_tfd_simbits on row ranges other than all rows: the bits of rows [row_begin, row_end) of the full matrix, zero
    in the tail word behind column N, zero on the diagonal, symmetric; and per row the lowest set bit above the diagonal
    is fc_tfd_first_match in every form."""
    fcm = fc.torsion_module
    rng = np.random.default_rng(10 * n + Q)
    c = rng.uniform(-180, 180, size=(max(n // 8, 1), Q))
    tf = R.wrap(c[rng.integers(0, len(c), n)] + rng.uniform(-1, 1, size=(n, Q)) * 15.0 / Q)
    S = R.simbits(tf, 10.0)
    if n >= 64:
        assert S.any() and not S[np.triu_indices(n, 1)].all()
    W = (n + 63) // 64
    for rb, re in ((0, n), (0, 1), (n - 1, n), (37, 101), (n // 2, n // 2), (0, 0), (n, n)):
        if re > n:
            continue
        bits = fcm.tfd_simbits(tf, 10.0, rb, re)
        assert bits.shape == (re - rb, W)
        b = R.bits_to_bool(bits, n) if re > rb else np.zeros((0, W * 64), dtype=bool)
        assert np.array_equal(b[:, :n], S[rb:re]) and not b[:, n:].any(), (rb, re)
    full = R.bits_to_bool(fcm.tfd_simbits(tf, 10.0), n)[:, :n]
    assert np.array_equal(full, full.T) and not full.diagonal().any()
    upper = np.triu(full, 1)
    low = np.where(upper.any(axis=1), upper.argmax(axis=1), -1)
    assert np.array_equal(low, R.first_match(tf, 10.0))
    _all_forms(monkeypatch, tf, 10.0, low)


# ---- j ---------------------------------------------------------------------------------------------------------
def _masks_agree(fc, monkeypatch, tf, thresh, forms):
    masks = []
    for look, u16 in forms:
        _knobs(monkeypatch, look, u16)
        masks.append(fc.torsion_module.prune_tfd_from_tf_mat(tf, thresh))
    for m in masks[1:]:
        assert np.array_equal(m, masks[0])
    return masks[0]


@pytest.mark.parametrize("Q", QS_AB)
def test_end_to_end_mask_wrap_case(fc, monkeypatch, Q):
    """j. prune_tfd_from_tf_mat gives the same mask under every form on the arrays of case a, and the oracle's literal
    loop on a slice"""
    tf, pos, neg, ref = _case_a(Q)
    mask = _masks_agree(fc, monkeypatch, tf, 10.0, FORMS.values())
    assert mask.dtype == bool and mask.shape == (len(tf),)
    part = np.ascontiguousarray(tf[:500])
    assert np.array_equal(_masks_agree(fc, monkeypatch, part, 10.0, FORMS.values()), o.prune_tfd_from_tf_mat(part, 10.0))


def test_end_to_end_mask_boundary_case(fc, monkeypatch):
    tf, plants, sweep, ref = _case_c()
    mask = _masks_agree(fc, monkeypatch, tf, 10.0, FORMS.values())
    assert mask.shape == (9000,)
    part = np.ascontiguousarray(tf[:700])  # (sweep rows with their partners 1 ... 130 columns on, dense-phase plants)
    assert (R.first_match(part, 10.0) >= 0).sum() > 100
    assert np.array_equal(_masks_agree(fc, monkeypatch, part, 10.0, FORMS.values()), o.prune_tfd_from_tf_mat(part, 10.0))


def test_end_to_end_mask_launchers_choice(fc, monkeypatch):
    tf, planted, check, ref = _case_f()
    mask = _masks_agree(fc, monkeypatch, tf, 1.0, ((None, None), (None, "0"), ("0", None)))
    assert mask.shape == (len(tf),)
