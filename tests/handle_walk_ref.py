"""One ensemble handle through every order of its operations (test infrastructure; the product never imports it).

``fc_ensemble`` carries state that some twenty features read and write ("State on the ensemble handle"): the
lazily made operand copies, the cached item table, the refine / ladder form hints, the sharding, ``bits_valid`` /
``lean`` / ``enant``, the counters and the pair queues the complete alignments borrow, the energies, the twin chain --
and behind it the process-wide context (stream, side streams, event pools, pinned slots, the caching pool).  This module
holds what the walk tests share:

* ``STEPS``: the operations, grouped in families; ``run(fc, ens, ctx)`` returns a tuple of NumPy arrays that is a pure
  function of the coordinates and the step's fixed parameters -- timings are dropped, pair lists are sorted, the stats a
  call returns go to ``ctx.log``;
* ``MODIFIERS``: what happens between two steps, in a fixed rotation;
* ``sequence(families)``: an Eulerian circuit of the complete directed graph with loops over the families, so that every
  ordered pair of families -- a family followed by itself included -- occurs adjacently;
* ``plan()``: the sequence with steps (rotating within a family) and modifiers filled in;
* ``walk()``: runs a plan on one long-lived handle and compares every step with ``Reference``: the same step on a FRESH
  handle under the same ``screen_select``, computed once per (step, screen) and kept;
* ``build(shape)``: the three ensembles, the smallest that still cross the launchers' branches.
"""

import ctypes as C
import os
from collections import namedtuple

import numpy as np

from firecode_amd import synthetic as syn

# ---- thresholds: (max_rmsd, max_dev).  SPARSE: below 5 % of the pairs similar; DENSE: above 50 % (test_handle_walk_cpu
# measures both with the oracle on each ensemble)
SPARSE = (0.5, 1.0)
DENSE = (1.52, 3.5)  # in the middle of the steep rise of the pair RMSDs: three quarters similar, and not transitively so
MAX_DE = 1.0  # energy window of the steps with energies (standard normal energies: about half of the pairs inside)

SHAPES = {
    "n300_a30": (300, 30),    # three row blocks of 128 with a tail, W = 5, 64-column tiles
    "n257_a120": (257, 120),  # 32-column tiles: the item table holds 32-column items afterwards
    "n150_a230": (150, 230),  # 16-column tiles
}
DUP_SOURCE = 3
N_OTHER = 97  # conformers of the second, different ensemble of the cross-ensemble steps


def dup_targets(n):
    return (11, n // 2 + 1, n - 1)


def degenerate_indices(n):
    """One planar conformer, then collinear ones.  A collinear structure has no unique optimal rotation with any partner:
    every pair with one goes to the fix-up queue of the complete alignments, like the exact duplicates.  As many as it
    takes to push that queue beyond 1 000 entries (the short-queue walk) while the similar pairs stay sparse."""
    count = -(-1001 // (n - 1)) + 2
    return [20 + q * ((n - 40) // count) for q in range(count)]


def fix_up_pairs(n):
    """pairs with a collinear partner: what the complete alignments queue for the fix-up at the least"""
    c = len(degenerate_indices(n)) - 1
    return c * (n - 1) - c * (c - 1) // 2


class Case:
    """An ensemble and everything the steps need beside the handle"""

    def __init__(self, shape):
        self.shape = shape
        n, a = SHAPES[shape]
        self.N, self.A = n, a
        X, atoms, _ = syn.synthetic_ensemble(n, a, seed=1000 + n)  # (every conformer has its own rigid motion)
        rng = np.random.default_rng(7 * n + a)
        for t in dup_targets(n):
            X[t] = X[DUP_SOURCE]  # exact duplicates
        for q, p in enumerate(degenerate_indices(n)):
            flat = np.zeros((a, 3))
            flat[:, :2 if q == 0 else 1] = rng.normal(scale=3.0, size=(a, 2 if q == 0 else 1))
            X[p] = flat @ syn.random_rotation(rng).T + rng.normal(scale=5.0, size=(1, 3))
        self.X, self.atoms = np.ascontiguousarray(X), atoms
        self.energies = rng.normal(size=n)
        self.energies2 = rng.normal(size=n)
        self.table = np.stack([np.arange(a), np.arange(a)[::-1]])  # a chain read from either end
        self.X_other = syn.synthetic_ensemble(N_OTHER, a, seed=2000 + n)[0]
        self.labels = (np.arange(n) % 4).astype(np.int64)
        self.labels[::17] = -1
        self.subset_idx = np.arange(0, n, 2, dtype=np.int64)[::-1].copy()
        iu, ju = np.triu_indices(n, 1)
        pick = np.random.default_rng(n).choice(len(iu), size=500, replace=False)
        self.pair_i, self.pair_j = iu[pick].astype(np.int64), ju[pick].astype(np.int64)
        self.other = None  # DeviceEnsemble of X_other (open())
        self.log = []      # (step name, what, stats) of the calls that return stats

    def open(self, fc):
        if self.other is None:
            self.other = fc.DeviceEnsemble(self.X_other, center=True)
        return self

    def close(self):
        if self.other is not None:
            self.other.close()
            self.other = None


_cases = {}


def build(shape):
    if shape not in _cases:
        _cases[shape] = Case(shape)
    return _cases[shape]


# ---- steps -----------------------------------------------------------------------------------------------------------
Step = namedtuple("Step", "name family params run")
REFUSED = "refused"


def _stats(a, keep=(0, 2, 5)):
    """pairs looked at, similar pairs, survivors / clusters: what does not depend on which correct screen ran"""
    return np.asarray(a, dtype=np.int64)[list(keep)].copy()


def _prune(thr, **kw):
    def run(fc, ens, ctx, name):
        e = {"E1": ctx.energies, "E2": ctx.energies2, None: None}[kw.get("energies")]
        extra = {k: v for k, v in kw.items() if k not in ("energies", "symmetry")}
        if kw.get("symmetry"):
            extra["symmetry"] = ctx.table
        mask, stats = ens.prune(thr[0], thr[1], energies=e, max_dE=MAX_DE if e is not None else 0.0, **extra)
        ctx.log.append((name, "prune", stats.copy()))
        return mask, _stats(stats)
    return run


def _simbits(thr, energies=None):
    def run(fc, ens, ctx, name):
        e = {"E1": ctx.energies, "E2": ctx.energies2, None: None}[energies]
        bits, _grey = ens.simbits(thr[0], thr[1], energies=e, max_dE=MAX_DE if e is not None else 0.0)
        return (bits,)
    return run


def _labelling(kind, thr, **kw):
    def run(fc, ens, ctx, name):
        out = getattr(ens, kind)(thr[0], thr[1], **kw)
        ctx.log.append((name, kind, out[-1].copy()))
        return tuple(out[:-1]) + (_stats(out[-1]),)
    return run


def host_ladder(ens, min_per_group, ranks=None):
    """the k-ladder on the host over ``prune_level`` (firecode_amd.dist.run_ladder); ``ranks``: the handles of all logical
    ranks, merged by the minimum as the all-gather would"""
    from firecode_amd import dist as fdist

    ranks = [ens] if ranks is None else ranks
    return fdist.run_ladder(ens.N, lambda k, m: np.stack([r.prune_level(k, m) for r in ranks]).min(axis=0),
                            lambda m: m[None], min_per_group=min_per_group)


def _begin(thr, rank, world, row_block, min_per_group=20, energies=None):
    def run(fc, ens, ctx, name):
        e = {"E1": ctx.energies, "E2": ctx.energies2, None: None}[energies]
        stats = ens.prune_begin(thr[0], thr[1], rank, world, row_block=row_block, energies=e,
                                max_dE=MAX_DE if e is not None else 0.0)
        ctx.log.append((name, "prune_begin", stats.copy()))
        level_mask = host_ladder(ens, min_per_group)
        try:
            pairs = np.sort(ens.similar_pairs())
        except fc.FirecodeHipInputError:  # the candidate queue overflowed: no list, the levels are the way
            return level_mask, _stats(stats, (0, 2)), np.array([REFUSED])
        again = np.sort(ens.similar_pairs(int(stats[2])))
        pair_mask = ens.prune_from_pairs(pairs, min_per_group)
        return level_mask, _stats(stats, (0, 2)), pairs, again, pair_mask
    return run


def _sharded(thr, min_per_group, row_block):
    def run(fc, ens, ctx, name):
        mask, stats = ens.prune_sharded(thr[0], thr[1], min_per_group=min_per_group, row_block=row_block)
        ctx.log.append((name, "prune_sharded", stats.copy()))
        return mask, _stats(stats, (0, 2))
    return run


def _bench_prune(thr):
    def run(fc, ens, ctx, name):
        _, _, mask, stats = ens.bench_prune(thr[0], thr[1], reps=4)
        ctx.log.append((name, "bench_prune", stats.copy()))
        return (mask,)
    return run


def _prune_many(thr, min_per_group, first):
    def run(fc, ens, ctx, name):
        order = [ens, ctx.other] if first else [ctx.other, ens]
        masks, survivors = fc._lib.prune_many(order, thr[0], thr[1], min_per_group=min_per_group)
        return masks[0], masks[1], survivors.copy()
    return run


def _all_pairs(kind):
    def run(fc, ens, ctx, name):
        if kind == "rmsd_and_max_all":
            r, d, _ms = ens.rmsd_and_max_all()
            return r, d
        if kind == "rmsd_values":
            return (ens.rmsd_values()[0],)
        return tuple(ens.rmsd_matrix())
    return run


def _knn(fc, ens, ctx, name):
    return tuple(ens.knn(8))


def _knn_against(fc, ens, ctx, name):
    return tuple(ens.knn_against(ctx.other, 5, max_rmsd=2.0))


def _diverse(fc, ens, ctx, name):
    return tuple(ens.select_diverse(12))


def _medoids(fc, ens, ctx, name):
    return tuple(ens.medoids(ctx.labels))


def _kmedoids(fc, ens, ctx, name):
    med, lab, dist, cost, n_iter = ens.kmedoids(6)
    return med, lab, dist, np.array([cost, n_iter], dtype=np.uint64)


def _silhouette(fc, ens, ctx, name):
    out = ens.silhouette(ctx.labels)
    return tuple(out[:-1]) + (np.array([out[-1]]),)


def _subset_view(fc, ens, ctx, name):
    sub = ens.subset(ctx.subset_idx)
    try:
        lab = ctx.labels[ctx.subset_idx]
        sil = sub.silhouette(lab)
        return tuple(sub.medoids(lab)) + tuple(sil[:-1]) + (np.array([sil[-1]]),)
    finally:
        sub.close()


def _rmsd_pairs(**kw):
    def run(fc, ens, ctx, name):
        extra = dict(kw)
        if extra.pop("symmetry", False):
            extra["symmetry"] = ctx.table
        return tuple(ens.rmsd_pairs(ctx.pair_i, ctx.pair_j, **extra))
    return run


def _steps():
    S = []

    def add(family, name, params, run):
        S.append(Step(name, family, params, lambda fc, ens, ctx, _run=run, _name=name: _run(fc, ens, ctx, _name)))

    add("a", "prune_sparse_mpg20", "SPARSE, min_per_group=20", _prune(SPARSE, min_per_group=20))
    add("a", "prune_dense_energies_mpg1", "DENSE, energies E1, min_per_group=1", _prune(DENSE, energies="E1", min_per_group=1))
    add("a", "prune_dense_mpg20", "DENSE, min_per_group=20", _prune(DENSE, min_per_group=20))
    add("b", "simbits_sparse", "SPARSE", _simbits(SPARSE))
    add("b", "simbits_dense_energies", "DENSE, energies E2", _simbits(DENSE, "E2"))
    add("c", "prune_enant_sparse", "SPARSE, prune_enantiomers", _prune(SPARSE, prune_enantiomers=True))
    add("c", "prune_enant_dense_mpg1", "DENSE, prune_enantiomers, min_per_group=1",
        _prune(DENSE, prune_enantiomers=True, min_per_group=1))
    add("d", "prune_symmetry_sparse", "SPARSE, reversal table", _prune(SPARSE, symmetry=True))
    add("d", "prune_symmetry_dense_energies", "DENSE, reversal table, energies E1",
        _prune(DENSE, symmetry=True, energies="E1"))
    add("e", "clusters_sparse", "SPARSE", _labelling("clusters", SPARSE))
    add("e", "dbscan_sparse_3", "SPARSE, min_samples=3", _labelling("dbscan", SPARSE, min_samples=3))
    add("e", "butina_dense", "DENSE", _labelling("butina", DENSE))
    add("f", "begin_0_1_128_sparse", "SPARSE, rank 0 of 1, row_block 128", _begin(SPARSE, 0, 1, 128))
    add("f", "begin_1_3_128_dense_energies", "DENSE, rank 1 of 3, row_block 128, energies E2, min_per_group=1",
        _begin(DENSE, 1, 3, 128, min_per_group=1, energies="E2"))
    add("f", "begin_0_2_256_sparse", "SPARSE, rank 0 of 2, row_block 256", _begin(SPARSE, 0, 2, 256))
    add("g", "sharded_sparse", "SPARSE, world of one", _sharded(SPARSE, 20, 0))
    add("g", "sharded_dense_mpg1_rb256", "DENSE, min_per_group=1, row_block 256", _sharded(DENSE, 1, 256))
    add("h", "bench_prune_sparse", "SPARSE, reps=4", _bench_prune(SPARSE))
    add("h", "bench_prune_dense", "DENSE, reps=4", _bench_prune(DENSE))
    add("i", "prune_many_first", "SPARSE, [ens, other]", _prune_many(SPARSE, 20, True))
    add("i", "prune_many_second_dense_mpg1", "DENSE, [other, ens], min_per_group=1", _prune_many(DENSE, 1, False))
    add("j", "rmsd_and_max_all", "", _all_pairs("rmsd_and_max_all"))
    add("j", "rmsd_values", "", _all_pairs("rmsd_values"))
    add("j", "rmsd_matrix", "", _all_pairs("rmsd_matrix"))
    add("k", "knn_8", "k=8", _knn)
    add("k", "knn_against_other_5", "k=5, max_rmsd=2.0", _knn_against)
    add("k", "select_diverse_12", "n_max=12", _diverse)
    add("l", "medoids", "labels i % 4, every 17th in no group", _medoids)
    add("l", "kmedoids_6", "n=6", _kmedoids)
    add("l", "silhouette", "labels i % 4, every 17th in no group", _silhouette)
    add("l", "subset_view", "every second conformer, reversed: medoids and silhouette", _subset_view)
    add("m", "rmsd_pairs", "500 sampled pairs", _rmsd_pairs())
    add("m", "rmsd_pairs_inverted", "500 sampled pairs, inverted", _rmsd_pairs(inverted=True))
    add("m", "rmsd_pairs_symmetry", "500 sampled pairs, reversal table", _rmsd_pairs(symmetry=True))
    return tuple(S)


STEPS = _steps()
FAMILIES = tuple(sorted({s.family for s in STEPS}))
PRUNE_STEPS = tuple(s.name for s in STEPS if s.family in "acdg")  # (their log entries are prune stats)

# ---- modifiers -------------------------------------------------------------------------------------------------------
MODIFIERS = ("screen_select(32)", "memory_trim", "stream_second", "screen_select(64)", "stream_own", "memory_trim",
             "screen_select(0)", "none")
TWIN = "twin"  # applied once per walk, at ``twin_at``


def sequence(families=FAMILIES):
    """Every ordered pair of families adjacent at least once: an Eulerian circuit of the complete directed graph with
    loops (Hierholzer, arcs taken in the order of ``families``) -> len(families)^2 + 1 entries"""
    families = list(families)
    unused = {f: list(families) for f in families}  # arcs f -> g not walked yet
    stack, circuit = [families[0]], []
    while stack:
        f = stack[-1]
        if unused[f]:
            stack.append(unused[f].pop(0))
        else:
            circuit.append(stack.pop())
    return circuit[::-1]


Visit = namedtuple("Visit", "index step modifier previous")


def plan(families=FAMILIES, twin_at=2, start=0, rounds=1):
    """the sequence with steps and modifiers filled in: within a family the steps rotate (``start`` shifts the
    rotation), the modifier in front of step i is ``MODIFIERS[i % 8]``, in front of step ``twin_at`` the twin is made too.
    ``rounds``: the circuit that many times on end, the rotation of family number q shifted by q more in every round, so
    that an ordered pair of families meets with other steps each time"""
    by_family = {f: [s for s in STEPS if s.family == f] for f in families}
    seen = {f: start for f in families}
    circuit = sequence(families)
    out, previous = [], None
    for i, f in enumerate(circuit + circuit[1:] * (rounds - 1)):
        if i >= len(circuit) and (i - len(circuit)) % (len(circuit) - 1) == 0:
            for q, g in enumerate(families):
                seen[g] += q
        step = by_family[f][seen[f] % len(by_family[f])]
        seen[f] += 1
        mod = MODIFIERS[i % len(MODIFIERS)]
        out.append(Visit(i, step, mod + "+" + TWIN if i == twin_at else mod, previous))
        previous = step.name
    return out


# ---- running ---------------------------------------------------------------------------------------------------------
class SecondStream:
    """a HIP stream of the caller's, made with the runtime the library itself is bound to"""

    def __init__(self, fc):
        self._hip = C.CDLL(fc._lib._mapped_hip_runtimes()[0])
        self.handle = C.c_void_p()
        rc = self._hip.hipStreamCreate(C.byref(self.handle))
        assert rc == 0 and self.handle.value, f"hipStreamCreate: {rc}"

    def destroy(self):
        if self.handle.value:
            self._hip.hipStreamDestroy(self.handle)
            self.handle = C.c_void_p()


def run_step(fc, step, ens, ctx):
    """the step's arrays, or the refusal it met on the host (an argument check made before any launch)"""
    try:
        return tuple(np.asarray(a) for a in step.run(fc, ens, ctx))
    except fc.FirecodeHipInputError as exc:
        return (np.array([REFUSED, str(exc.code), str(exc)]),)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def differences(got, ref):
    """indices of the outputs that are not bit-equal (NaN == NaN, -0.0 != 0.0: the same kernels saw the same data)"""
    if len(got) != len(ref):
        return list(range(max(len(got), len(ref))))
    return [k for k, (a, b) in enumerate(zip(got, ref)) if not same_bits(a, b)]


class Reference:
    """the same step on a fresh handle under the screen selection in force, once per (case, step, screen)"""

    def __init__(self, fc):
        self.fc, self.memo = fc, {}

    def get(self, ctx, step, screen):
        key = (ctx.shape, step.name, screen, os.environ.get("FC_PAIRQ_CAP", ""))  # (the queue length is read per call)
        if key not in self.memo:
            log, ctx.log = ctx.log, []  # (the stats of a reference run are not the walk's)
            try:
                with self.fc.DeviceEnsemble(ctx.X, center=True) as fresh:
                    self.memo[key] = run_step(self.fc, step, fresh, ctx)
            finally:
                ctx.log = log
        return self.memo[key]


class Walker:
    """applies modifiers and runs steps on long-lived handles; ``finish()`` restores the library's own stream and the
    automatic screen whatever happened"""

    def __init__(self, fc, reference=None):
        self.fc, self.reference, self.screen = fc, reference, 0
        self.stream = SecondStream(fc)
        self.twins = {}  # id(head) -> its twin workspace, once made

    def modify(self, modifier, ens):
        L = self.fc._lib
        for m in modifier.split("+"):
            if m.startswith("screen_select"):
                self.screen = int(m[m.index("(") + 1:-1])
                L.screen_select(self.screen)
            elif m == "memory_trim":
                L.memory_trim()
            elif m == "stream_second":
                L.stream_set(self.stream.handle.value)
            elif m == "stream_own":
                L.stream_set(None)
            elif m == TWIN:
                self.twins[id(ens)] = ens.twin()
            else:
                assert m == "none", m

    def step(self, visit, ens, ctx):
        got = self._compare(visit, ens, ctx, "")
        # the plain prunes also on the twin workspace, once it exists: it shares the head's coordinates and hints
        if visit.step.family == "a" and id(ens) in self.twins:
            self._compare(visit, self.twins[id(ens)], ctx, " on the twin workspace")
        return got

    def _compare(self, visit, ens, ctx, where):
        got = run_step(self.fc, visit.step, ens, ctx)
        if self.reference is not None:
            ref = self.reference.get(ctx, visit.step, self.screen)
            bad = differences(got, ref)
            if bad:
                raise AssertionError(
                    f"{ctx.shape}: step {visit.index} {visit.step.name} ({visit.step.params}){where} behind modifier "
                    f"{visit.modifier!r}, previous step {visit.previous}, screen_select({self.screen}): outputs {bad} "
                    f"differ from the same step on a fresh handle" + _describe(got, ref, bad))
        return got

    def finish(self):
        L = self.fc._lib
        try:
            L.screen_select(0)
        finally:
            try:
                L.stream_set(None)
            finally:
                self.stream.destroy()


def _describe(got, ref, bad):
    k = bad[0]
    if k >= len(got) or k >= len(ref):
        return f": {len(got)} outputs against {len(ref)}"
    a, b = got[k], ref[k]
    if a.shape != b.shape or a.dtype != b.dtype:
        return f": output {k} is {a.dtype}{a.shape}, fresh {b.dtype}{b.shape}; walk {a.ravel()[:4]}, fresh {b.ravel()[:4]}"
    if a.dtype.kind in "US":
        return f": walk {a}, fresh {b}"
    raw = [np.ascontiguousarray(x).reshape(-1).view(np.uint8).reshape(x.size, x.dtype.itemsize) for x in (a, b)]
    ne = np.flatnonzero((raw[0] != raw[1]).any(axis=1))
    at = ne[:4]
    return f": output {k} differs in {len(ne)} of {a.size} entries, first at {at}: walk {a.ravel()[at]}, fresh {b.ravel()[at]}"


def walk(fc, ctx, ens, visits, reference=None):
    """the whole plan on one handle -> the last result of every step name"""
    walker = Walker(fc, reference)
    last = {}
    try:
        ctx.open(fc)
        for v in visits:
            walker.modify(v.modifier, ens)
            last[v.step.name] = walker.step(v, ens, ctx)
    finally:
        walker.finish()
    return last
