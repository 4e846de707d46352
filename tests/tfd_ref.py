"""Reference and case builders for the TFD first-match kernels (test infrastructure; the product never imports it).

The contract is the literal formula of firecode/torsion_module.py:1056-1067,

    d = |a - b|;  d = |d - (d > 180) * 360|;  np.sum(d) < thresh

with ``np.sum`` over the contiguous last axis: the product promises NumPy's bits, not a better sum, so nothing
here adds in higher precision.
"""

import numpy as np

# ---- the constants of firecode_amd/csrc/fc_prune.hip that the cases are built around ---------------------------
ROWS = 64              # rows of a workgroup: `i0 = blockIdx.x * 64` in k_tfd_first_match / k_tfd_first_match_dense_u16
WALK_WIN = 256         # columns per window of the 16-bit walk: `WIN = 256` in k_tfd_first_match_walk_u16
REST_WIN = 1024        # columns per box of the fp32 chunks: `j0 = w * 1024` in k_tfd_window_bounds
CHUNK = 65536          # columns per chunk of k_tfd_first_match_rest: `const int64_t chunk = 65536` in the launcher
DENSE_DEFAULT = 128    # dense phase without a knob: `ahead = forced ? lookahead_env : 128` in the launcher
TWO_PHASE_N = 65536    # two phases without a knob: `forced ? N > 8 * lookahead_env : N >= 65536` in the launcher
LOOKAHEAD_DEFAULT = 4096  # fp32 look-ahead without a knob: `int64_t lookahead_env = 4096` in the launcher
U16_BAND = 10          # undecided band in 16-bit units: `t_hi = ceil(ts) + 10`, `t_lo = floor(ts) - 10` in the launcher
U16_MAX_ANGLE = 270.0  # angles the 16-bit path accepts: `if (!(fabs(a) <= 270.0)) bad = true` in k_tfd_pack_u16
Q_MAX = 128            # `if (Q > 128) return set_error(FC_E_LIMIT, ...` in fc_tfd_first_match / fc_tfd_simbits

# bits of fc_tfd_last_form
FORM_ONE_PHASE, FORM_F32_REST, FORM_U16_DENSE, FORM_U16_WALK, FORM_U16_REFUSED = 1, 2, 4, 8, 16


def wrap(a):
    """angles into [-180, 180)"""
    return (np.asarray(a, dtype=np.float64) + 180.0) % 360.0 - 180.0


def deltas(a, b):
    d = np.abs(a - b)
    return np.abs(d - (d > 180) * 360)


def pair_sum(a, b):
    """np.sum of the reference's deltas of one pair, as NumPy computes it"""
    return float(np.sum(deltas(np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64))))


def first_match(tf, thresh, rows=None):
    """first_match[i] = min{j > i : similar(i, j)} or -1, row against all later rows.  rows: the reference for those
    rows only (an array of len(rows) entries, in their order)."""
    tf = np.ascontiguousarray(tf, dtype=np.float64)
    n = len(tf)
    todo = range(n) if rows is None else [int(r) for r in rows]
    out = np.full(len(todo), -1, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for k, i in enumerate(todo):
            if i + 1 >= n:
                continue
            d = np.ascontiguousarray(deltas(tf[i + 1:], tf[i]))
            hit = np.flatnonzero(np.sum(d, axis=-1) < thresh)
            if len(hit):
                out[k] = i + 1 + hit[0]
    return out


def simbits(tf, thresh):
    """(N, N) bool: similar(i, j), diagonal False"""
    tf = np.ascontiguousarray(tf, dtype=np.float64)
    n = len(tf)
    out = np.zeros((n, n), dtype=bool)
    with np.errstate(invalid="ignore"):
        for i in range(n):
            out[i] = np.sum(np.ascontiguousarray(deltas(tf, tf[i])), axis=-1) < thresh
            out[i, i] = False
    return out


def bits_to_bool(bits, n):
    """rows of uint64 words (bit j of word j // 64) -> (rows, n_words * 64) bool"""
    b = np.ascontiguousarray(bits, dtype="<u8")
    return np.unpackbits(b.view(np.uint8).reshape(b.shape[0], -1), axis=1, bitorder="little").astype(bool)


def lattice(n_side, Q, spacing, seed, dims=2):
    """n_side ** dims rows in which no two are similar for any thresh <= spacing, by construction: distinct points of a
    grid of step `spacing`, centred on 0, in the first `dims` angles (two points differ by >= spacing in one of them,
    and every other delta only adds); the other angles hold one value per row.  The rows are shuffled.  The circular
    distance across the seam is 360 - (n_side - 1) * spacing: choose `spacing` so that it exceeds the threshold too.
    With Q < dims the grid loses coordinates and rows repeat (no such guarantee then)."""
    rng = np.random.default_rng(seed)
    g = (np.arange(n_side, dtype=np.float64) - (n_side - 1) / 2.0) * spacing
    assert (n_side - 1) * spacing < 360.0 and np.abs(g).max() < 180.0
    grid = np.stack(np.meshgrid(*[g] * dims, indexing="ij"), axis=-1).reshape(-1, dims)
    tf = np.empty((len(grid), Q), dtype=np.float64)
    tf[:, :min(Q, dims)] = grid[:, :min(Q, dims)]
    if Q > dims:
        tf[:, dims:] = rng.uniform(-150.0, 150.0, size=len(grid))[:, None]
    return np.ascontiguousarray(tf[rng.permutation(len(grid))])


def seam_gap(n_side, spacing):
    return 360.0 - (n_side - 1) * spacing


def plant(tf, i, j, total, rng, angles=None, across_wrap=False):
    """Overwrite row j with row i plus signed offsets whose absolute values sum to `total`, in the fingerprint angles
    `angles` (default: all).  across_wrap: row i's chosen angles are first moved to within the offset of +180 or -180,
    so that i and j end on opposite sides of the seam.  Returns the pair's np.sum."""
    Q = tf.shape[1]
    angles = np.arange(Q) if angles is None else np.asarray(angles, dtype=np.int64)
    w = rng.dirichlet(np.ones(len(angles))) * total if len(angles) > 1 else np.array([float(total)])
    sign = rng.choice([-1.0, 1.0], size=len(angles))
    if across_wrap:
        x = rng.uniform(0.1, 0.9, size=len(angles)) * w  # row i sits x inside the seam, row j  w - x  beyond it
        tf[i, angles] = sign * (180.0 - x)
    tf[j] = tf[i]
    v = tf[i, angles] + sign * w
    tf[j, angles] = np.where(np.abs(v) > 180.0, wrap(v), v)  # (the angles that stay inside keep their bits)
    return pair_sum(tf[i], tf[j])


def opposite_sides(tf, i, j, angles):
    """the pair sits on opposite sides of +-180 in every one of `angles`"""
    a, b = tf[i, angles], tf[j, angles]
    return bool(np.all(a * b < 0) and np.all(np.abs(a - b) > 180.0))


def eight_lane_sum(v):
    """The order tfd_sum (fc_prune.hip) adds in: left to right below 8 elements, otherwise eight running lanes combined
    as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) and the n % 8 tail one by one -- NumPy's order up to 128 elements."""
    v = [float(x) for x in v]
    n = len(v)
    if n < 8:
        res = 0.0
        for x in v:
            res += x
        return res
    r = v[:8]
    i = 8
    while i < n - n % 8:
        for k in range(8):
            r[k] += v[i + k]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    while i < n:
        res += v[i]
        i += 1
    return res


# ---- case builders (shared by tests/test_tfd_ref.py, which checks them on the CPU, and tests/test_gpu_tfd_kernels.py) ----
def background(n, Q, thresh=10.0):
    """n rows for the planted cases at thresh 10: match-free by construction where that many rows exist (Q >= 3: a grid of
    step > thresh in three or four angles); for Q = 1, 2 no 6 000 rows are pairwise 10 degrees apart, so the grid is
    dense there (rows have partners; the planted rows sit at the seam, 25 degrees and more from all of it)."""
    if Q == 1:
        tf = lattice(n, 1, 300.0 / n, 7, dims=1)
    elif Q == 2:
        side = int(np.ceil(np.sqrt(n)))
        tf = lattice(side, 2, 4.0, 7, dims=2)
    elif Q == 3:
        side = int(np.ceil(n ** (1.0 / 3.0) - 1e-9))
        tf = lattice(side, 3, 300.0 / side, 7, dims=3)
    else:
        side = int(np.ceil(n ** 0.25 - 1e-9))
        tf = lattice(side, Q, 300.0 / side, 7, dims=4)
    assert len(tf) >= n
    return np.ascontiguousarray(tf[:n])


def wrap_case(Q, n=6000, thresh=10.0, seed=0):
    """Case a: per angle q < min(Q, 9) one pair whose whole offset sits in angle q across the seam (total 4.0) and one
    negative control of the same geometry (total 10.5), one pair spread over all angles (Q > 1); partners 3 000 - 5 000 rows
    later.  The rows are redrawn until the reference, on the planted rows alone, says that every positive matched its
    partner and no negative did (for Q >= 2: that the negative matched nothing)."""
    base = background(n, Q, thresh)
    nq = min(Q, 9)
    for attempt in range(400):
        rng = np.random.default_rng([seed, Q, attempt])
        tf = base.copy()
        k = 2 * nq + (1 if Q > 1 else 0)  # (Q = 1: the spread pair would be the pair of angle 0 again)
        ii = rng.permutation(1000)[:k]  # (in any order: at Q = 1 all planted rows lie within 11 degrees of the seam)
        used = set(ii.tolist())
        pos, neg = [], []
        ok = True
        for m, i in enumerate(ii):
            j = int(i + rng.integers(3000, 5001))
            while j in used:
                j += 1
            if j >= n:
                ok = False
                break
            used.add(j)
            if m < nq:
                s = plant(tf, i, j, 4.0, rng, angles=[m], across_wrap=True)
                pos.append((int(i), j, [m], s))
            elif m < 2 * nq:
                s = plant(tf, i, j, 10.5, rng, angles=[m - nq], across_wrap=True)
                neg.append((int(i), j, [m - nq], s))
            else:
                s = plant(tf, i, j, 4.0, rng, across_wrap=True)
                pos.append((int(i), j, list(range(Q)), s))
        if not ok:
            continue
        ref = first_match(tf, thresh, rows=[p[0] for p in pos + neg])
        rp, rn = ref[:len(pos)], ref[len(pos):]
        if all(r == p[1] for r, p in zip(rp, pos)) and all(r != p[1] and (Q < 2 or r == -1) for r, p in zip(rn, neg)):
            return tf, pos, neg
    raise AssertionError("no placement of the planted pairs found")


SEAM_WINDOWS = ((5, 179.5), (11, 179.5), (20, 179.5), (15, 179.25))  # (window of 256 columns, +-value of angle 0)


def seam_windows_case(Q, n=6000, thresh=10.0, seed=0):
    """Case b: three windows of 256 columns whose first angle alternates between +179.5 and -179.5 (a box 359 wide: the
    whole circle) and one with +-179.25 (358.5 wide: a box still); early rows are copies (total 4.0, and 10.5 as the
    negative control) of columns at the first, a middle and the last column of each window and of the columns right
    before and behind it.  Returns tf and the planted (row, column, window, total)."""
    rng = np.random.default_rng([seed, Q, 77])
    tf = background(n, Q, thresh).copy()
    for w, v in SEAM_WINDOWS:
        cols = np.arange(w * WALK_WIN, (w + 1) * WALK_WIN)
        tf[cols, 0] = np.where(cols % 2 == 0, v, -v)
    early = iter(np.sort(rng.permutation(1000)[:6 * len(SEAM_WINDOWS)]).tolist())
    planted = []
    for w, _ in SEAM_WINDOWS:
        c0 = w * WALK_WIN
        for j, total in ((c0 - 1, 4.0), (c0, 4.0), (c0 + 101, 4.0), (c0 + 64, 10.5), (c0 + WALK_WIN - 1, 4.0), (c0 + WALK_WIN, 4.0)):
            i = next(early)
            # (row i becomes a copy of column j: the window keeps its box; the copies of the window's first and last
            # column differ in angle 0 alone, the first one redrawn until it lies across the seam from its column)
            while True:
                plant(tf, j, i, total, rng, angles=[0] if j in (c0, c0 + WALK_WIN - 1) else None)
                if j != c0 or tf[i, 0] * tf[j, 0] < 0:
                    break
            planted.append((i, j, w, total))
    return tf, planted


def boundary_case(n=9000, look=64, seed=0):
    """Case c (Q = 3, thresh 10, match-free grid of step 300 / 21 > 14): rows at lanes 0, 1, 62, 63 of every fourth block
    of 64 with their only partner at the end of the dense phase (i0 + 64 + look: -1, +0, +1), at the next two multiples
    of 256 and the next of 1 024 (-1, +0, +1; a multiple already taken: the one after) and at n - 1; and a gap sweep: row k of 1 300 has its only partner k + 1 columns
    later.  Returns tf, the boundary plants (row, column, kind) and the sweep (row, column)."""
    rng = np.random.default_rng([seed, 3, 99])
    tf = background(n, 3, 10.0).copy()
    used = set()
    kinds = []
    for unit, name in ((REST_WIN, "box"), (WALK_WIN, "win")):
        for nth in ((0,) if unit == REST_WIN else (1, 0)):
            kinds += [((name, nth, unit), d) for d in (-1, 0, 1)]
    kinds += [("dense", d) for d in (-1, 0, 1)]
    kinds.append(("last", 0))
    plants = []
    lanes = (0, 1, 62, 63)
    # plant p: kind p % len(kinds) at lane p % 4 (13 and 4 are coprime: every combination once), four plants to a block,
    # the blocks 1, 5, 9 ...: the multiples of 256 -1, +0, +1 lie in blocks 3 and 0 (mod 4), never on a planted row
    assert len(kinds) % 2 == 1
    for p in range(4 * len(kinds)):
        if True:
            (kind, d), lane = kinds[p % len(kinds)], lanes[p % 4]
            i0 = (4 * (p // 4) + 1) * ROWS
            i = i0 + lane
            end = i0 + ROWS + look
            bump = 0
            while True:  # (a column already taken: the multiple after it, the column before it)
                if kind == "dense":
                    j = end + d
                elif kind == "last":
                    j = n - 1 - bump
                else:
                    name, nth, unit = kind
                    j = ((end + 1) // unit + 1 + nth + bump) * unit + d
                if j not in used:
                    break
                bump += 1
                assert kind != "dense"
            assert i not in used and i < j < n
            used.update((i, j))
            plant(tf, i, j, 4.0, rng)
            plants.append((i, j, kind if isinstance(kind, str) else "%s%d" % (kind[0], kind[1]), d))
    sweep = []
    i = 0
    for k in range(1300):
        while i in used or i + k + 1 in used:
            i += 1
        j = i + k + 1
        assert j < n
        used.update((i, j))
        plant(tf, i, j, 4.0, rng)
        sweep.append((i, j))
        i += 4
    return tf, plants, sweep


F_EPS = (0.0, 1e-9, -1e-9, 3e-3, -3e-3, 0.02, -0.02, 0.05, -0.05, 0.07, -0.07, 0.5, -0.5)
F_GAPS = (3, 100, 127, 128, 129, 700, 40000)


def launcher_case(seed=0):
    """Case f: the 257 x 257 grid of step 1.4 (66 049 rows, Q = 2, thresh 1.0, seam gap 1.6) with pairs planted at totals
    1.0 + e for every e of F_EPS at every gap of F_GAPS, across column 65 536, and across the seam.  Returns tf, the
    planted (row, column) and `check`: every row whose first match the grid argument does not already give as -1,
    i.e. the rewritten rows and every row similar to one of them."""
    thresh = 1.0
    rng = np.random.default_rng([seed, 2, 257])
    tf = lattice(257, 2, 1.4, 11)
    n = len(tf)
    assert n == 66049 and seam_gap(257, 1.4) > thresh
    used, planted = set(), []

    def put(i, j, total, across):
        assert i not in used and j not in used and i < j < n
        used.update((i, j))
        if across:
            # row i goes to within 0.45 of the seam in angle 0 and half a grid step off the grid in angle 1: further than
            # thresh from every grid row (whose edge is 0.8 from the seam); the offsets are redrawn until row j is beyond
            tf[i] = (rng.choice([-1.0, 1.0]) * (180.0 - rng.uniform(0.1, 0.45)), tf[i, 1] + 0.7)
        while True:
            plant(tf, i, j, total, rng)
            if not across or tf[i, 0] * tf[j, 0] < 0:
                break
        planted.append((i, j))

    starts = iter(range(50, 25000, 251))
    for g in F_GAPS:
        for e in F_EPS:
            i = next(starts)
            while i in used or i + g in used:
                i += 1
            put(i, i + g, 1.0 + e, False)
    for k, e in enumerate(F_EPS):  # across the chunk boundary of the fp32 form, its second chunk holding 513 columns
        put(CHUNK - 1 - 40 * k, CHUNK + (k * 41) % 513, 1.0 + e, k % 2 == 1)
    for k, e in enumerate(F_EPS):  # across the seam, partners 30 000 columns later
        put(30000 + 97 * k, 60000 + 89 * k, 1.0 + e, True)
    changed = sorted(used)
    check = set(changed)
    for r in changed:
        near = np.flatnonzero(np.sum(np.ascontiguousarray(deltas(tf, tf[r])), axis=-1) < thresh)
        check.update(near.tolist())
    return tf, planted, np.array(sorted(check), dtype=np.int64)
