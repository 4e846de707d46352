"""One ensemble handle through every order of its operations (tests/handle_walk_ref.py; DESIGN.md, "State on the ensemble
handle").  Nearly every other GPU test builds a fresh ``DeviceEnsemble``, runs one family of operations and closes it;
here one long-lived handle runs 170 steps in which every ordered pair of the 13 families occurs adjacently, with the
screen selection, the caching pool, the stream and the twin changing in between, and every step must give what the
same step gives on a fresh handle: masks, labels, indices, bit words and pair lists equal, floating-point outputs
bit-equal -- the same kernels see the same coordinates.

State-dependent form choices met: the refine's bucket form and the ladder's launch-per-level form (``last_candidates`` /
``last_similar``), the clusters' short-list hook and the context's hints for a fresh ensemble all pick between kernels
that produce the same integers; no floating-point output of any step depends on them, so no output is compared with a
tolerance against the fresh handle.  The final state is compared with the oracle at the suite's tolerance so that the
history-laden handle and the fresh one cannot be wrong together.
"""

import functools

import numpy as np
import pytest

import handle_walk_ref as hw
from firecode_amd import dist as fdist
from oracle import cpu_ref as o

pytestmark = pytest.mark.gpu

TOL = 1e-10
SHAPE_IDS = sorted(hw.SHAPES)
SMALL = "n300_a30"  # the directed cases
# FC_E_LIMIT by shape alone, before any launch: the value kernel keeps a 64-column tile in LDS (up to 104 atoms), a tile
# of the symmetry-aware screen both coordinate tiles and the table
EXPECTED_REFUSALS = {
    "n300_a30": set(),
    "n257_a120": {"rmsd_values"},
    "n150_a230": {"rmsd_values", "prune_symmetry_sparse", "prune_symmetry_dense_energies"},
}


@pytest.fixture(scope="module")
def reference(fc):
    return hw.Reference(fc)


@pytest.fixture(scope="module", autouse=True)
def _close_cases():
    yield
    for shape in SHAPE_IDS:
        hw.build(shape).close()


@functools.lru_cache(maxsize=None)
def oracle_matrices(shape):
    case = hw.build(shape)
    _, R, D = o.rmsd_similarity_matrix(case.X, case.atoms, hw.SPARSE[0], hw.SPARSE[1])
    return R, D


def oracle_similar(shape, thr):
    R, D = oracle_matrices(shape)
    S = (R < thr[0]) & (D < thr[1])
    np.fill_diagonal(S, False)
    return S


def oracle_mask(shape, thr, energies=None, min_per_group=20):
    """the handle's prune: the energy window belongs to the predicate, the order is the handle's own (sorting by energy
    is the drivers' business, firecode_amd.pruner)"""
    S = oracle_similar(shape, thr)
    if energies is not None:
        S = S & (np.abs(energies[:, None] - energies[None, :]) < hw.MAX_DE)
    return o.greedy_prune_from_matrix(S, min_per_group=min_per_group)


def packed(S, rows=None):
    i, j = np.nonzero(np.triu(S, 1))
    if rows is not None:
        keep = rows[i]
        i, j = i[keep], j[keep]
    return np.sort((i.astype(np.uint64) << np.uint64(32)) | j.astype(np.uint64))


# ---- the walks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPE_IDS)
def test_walk(fc, reference, shape):
    """the circuit three times on end on one handle (508 steps, an ordered pair of families meeting with other steps each
    time), the twin made early; every step equals the same step on a fresh handle"""
    case = hw.build(shape)
    case.log = []
    with fc.DeviceEnsemble(case.X, center=True) as ens:
        hw.walk(fc, case, ens, hw.plan(twin_at=2, rounds=3), reference)
    # the steps a fresh handle refuses are the library's documented limits at this shape and nothing else
    refused = {k[1]: v[0] for k, v in reference.memo.items() if k[0] == shape and k[3] == "" and len(v) == 1
               and v[0].dtype.kind in "US" and v[0][0] == hw.REFUSED}
    print(f"{shape}: steps a fresh handle refuses: {sorted(refused)}")
    assert set(refused) == EXPECTED_REFUSALS[shape], refused
    assert all(int(v[1]) == fc._lib.FC_E_LIMIT for v in refused.values()), refused


@pytest.mark.parametrize("shape", SHAPE_IDS)
def test_walk_with_a_short_pair_queue(fc, reference, shape, monkeypatch):
    """the same walk with a candidate queue of 1 000 entries (FC_PAIRQ_CAP, read whenever the prune workspace is shaped):
    the dense steps overflow it and take the bit-matrix redo, the complete alignments overflow their fix-up queue and run
    again -- and the twin comes late"""
    case = hw.build(shape)
    case.log = []
    monkeypatch.setenv("FC_PAIRQ_CAP", "1000")
    with fc.DeviceEnsemble(case.X, center=True) as ens:
        last = hw.walk(fc, case, ens, hw.plan(twin_at=130), reference)
        # without an overflow this walk tests nothing new
        candidates = [int(s[1]) for name, what, s in case.log if what == "prune"]
        print(f"{shape}: largest candidate count of a prune step {max(candidates)}")
        assert max(candidates) > 1000
        # (the bench form of the complete alignments reports the overflow that the plain call answers by running again)
        with pytest.raises(fc.FirecodeHipInputError, match="fix-up queue") as overflow:
            ens.bench_rmsd_and_max_all(1)
        print(f"{shape}: {overflow.value}")
        assert overflow.value.code == fc._lib.FC_E_LIMIT
        r, d, _ = ens.rmsd_and_max_all()  # ... and the handle is as good as before
        assert hw.same_bits(r, last["rmsd_and_max_all"][0]) and hw.same_bits(d, last["rmsd_and_max_all"][1])
    # a begin whose candidates overflowed has no pair list to hand out (rank 1 of 3 owns 22 rows of the 150: no overflow there)
    for name in ("begin_0_1_128_sparse", "begin_1_3_128_dense_energies", "begin_0_2_256_sparse"):
        queued = [int(s[1]) for n, what, s in case.log if n == name][-1]
        assert (last[name][-1].dtype.kind in "US") == (queued > 1000), (name, queued)
    assert last["begin_1_3_128_dense_energies"][-1].dtype.kind in "US" or case.N < 257


def test_two_handles_alternately(fc, reference):
    """steps alternate between two handles of different shape: what lives in the context (pinned slots, event pools,
    side streams, the hints for a fresh ensemble, ``mark_after_screen``) belongs to neither"""
    a, b = hw.build("n300_a30"), hw.build("n150_a230")
    a.log, b.log = [], []
    walker = hw.Walker(fc, reference)
    try:
        a.open(fc), b.open(fc)
        with fc.DeviceEnsemble(a.X, center=True) as ea, fc.DeviceEnsemble(b.X, center=True) as eb:
            for va, vb in zip(hw.plan(twin_at=2), hw.plan(twin_at=100, start=1)):
                walker.modify(va.modifier, ea)
                walker.step(va, ea, a)
                if hw.TWIN in vb.modifier:
                    walker.modify(hw.TWIN, eb)
                walker.step(vb, eb, b)
    finally:
        walker.finish()


@pytest.mark.parametrize("shape", SHAPE_IDS)
def test_final_state_against_the_oracle(fc, shape):
    """after a walk (no fresh handles in between) the handle still computes what the oracle computes"""
    case = hw.build(shape)
    case.log = []
    R0, D0 = oracle_matrices(shape)
    with fc.DeviceEnsemble(case.X, center=True) as ens:
        hw.walk(fc, case, ens, hw.plan(twin_at=130))
        mask, stats = ens.prune(*hw.SPARSE)
        S = oracle_similar(shape, hw.SPARSE)
        assert np.array_equal(mask, o.greedy_prune_from_matrix(S)) and stats[2] == np.triu(S, 1).sum()
        R, D, _ = ens.rmsd_and_max_all()
        idx, dist = ens.knn(8)
    i, j = case.pair_i, case.pair_j
    Xc = case.X - case.X.mean(axis=1, keepdims=True)
    bound = o.rotation_error_bound_batch(Xc[i], Xc[j])
    fin = np.isfinite(bound)
    print(f"{shape}: rmsd off by {np.abs(R[i, j] - R0[i, j]).max():.2e}, max deviation by "
          f"{np.abs(D[i, j] - D0[i, j])[fin].max():.2e} ({int((~fin).sum())} sampled pairs without a unique rotation)")
    assert np.abs(R[i, j] - R0[i, j]).max() < TOL
    assert np.all(np.abs(D[i, j] - D0[i, j])[fin] <= TOL + bound[fin]) and 0.8 < fin.mean() < 1.0
    # k-NN: the distances are the 8 smallest of the oracle's row, and every listed index has the listed distance
    off = R0 + np.diag(np.full(case.N, np.inf))
    assert np.abs(dist - np.sort(off, axis=1)[:, :8]).max() < TOL
    assert np.abs(dist - np.take_along_axis(off, idx.astype(np.int64), axis=1)).max() < TOL
    assert all(len(set(row)) == 8 for row in idx)


# ---- directed cases --------------------------------------------------------------------------------------------------
def test_prune_level_after_other_operations_is_refused_never_stale(fc):
    """``prune_level`` needs the bit matrix of a ``prune_begin``.  A lean prune and the clusters leave ``lean`` set, the
    complete alignments reshape the workspace (``bits_valid`` cleared): each is refused on the host, none answers from
    the bits of the earlier, denser ``prune_begin``.  ``similar_pairs`` hands out the list of whatever graph was built
    last -- the prune's or the clusters' own, as rank 0 of 1 -- and is refused after the complete alignments, which use
    the queues for their fix-up."""
    case = hw.build(SMALL).open(fc)
    ones = np.ones(case.N, dtype=np.uint8)
    sparse_pairs = packed(oracle_similar(SMALL, hw.SPARSE))
    with fc.DeviceEnsemble(case.X, center=True) as ens:
        for what in ("prune", "clusters", "rmsd_and_max_all"):
            ens.prune_begin(*hw.DENSE, 0, 1, 128)  # the bits a stale answer would come from
            assert np.array_equal(hw.host_ladder(ens, 20), oracle_mask(SMALL, hw.DENSE)), what
            if what == "prune":
                mask, _ = ens.prune(*hw.SPARSE)
                assert np.array_equal(mask, oracle_mask(SMALL, hw.SPARSE))
            elif what == "clusters":
                labels = ens.clusters(*hw.SPARSE)[0]
                assert labels.max() + 1 == len(set(labels)) and labels[hw.DUP_SOURCE] == labels[case.N - 1]
            else:
                R, _, _ = ens.rmsd_and_max_all()
                assert np.abs(R - oracle_matrices(SMALL)[0]).max() < TOL
            with pytest.raises(fc.FirecodeHipInputError, match="fc_prune_rmsd_begin has not been called"):
                ens.prune_level(1, ones)
            if what == "rmsd_and_max_all":
                with pytest.raises(fc.FirecodeHipInputError, match="fc_prune_rmsd_begin has not been called"):
                    ens.similar_pairs()
            else:
                assert np.array_equal(np.sort(ens.similar_pairs()), sparse_pairs), what
        # ... and the handle is usable afterwards
        ens.prune_begin(*hw.SPARSE, 0, 1, 128)
        assert np.array_equal(hw.host_ladder(ens, 20), oracle_mask(SMALL, hw.SPARSE))


def test_similar_pairs_after_prune_from_pairs_is_the_ranks_own_list_again(fc):
    """``prune_from_pairs`` with a proper subset of the rank's own list, then ``similar_pairs``: the rank's own list
    again, whole.  (fc_prune_from_pairs used to write the length of the caller's list into counters[2], the length of
    the ensemble's own queue: the next fc_prune_similar_pairs returned the first third of the list.)"""
    case = hw.build(SMALL)
    S = oracle_similar(SMALL, hw.SPARSE)
    with fc.DeviceEnsemble(case.X, center=True) as ens:
        stats = ens.prune_begin(*hw.SPARSE, 1, 3, 128)
        own = np.sort(ens.similar_pairs())
        assert np.array_equal(own, packed(S, fdist.owner_of_rows(case.N, 3, 128) == 1)) and len(own) == stats[2] > 30
        part = own[::3].copy()
        S_part = np.zeros_like(S)
        S_part[(part >> np.uint64(32)).astype(np.int64), (part & np.uint64(0xFFFFFFFF)).astype(np.int64)] = True
        for mpg in (20, 1):
            assert np.array_equal(ens.prune_from_pairs(part, mpg), o.greedy_prune_from_matrix(S_part | S_part.T, min_per_group=mpg))
            assert np.array_equal(np.sort(ens.similar_pairs()), own)
            assert np.array_equal(np.sort(ens.similar_pairs(int(stats[2]))), own)
        assert np.array_equal(ens.prune_from_pairs(part[:0], 20), np.ones(case.N, dtype=bool))  # an empty list prunes nothing
        assert np.array_equal(np.sort(ens.similar_pairs()), own)
        # the levels of this rank are untouched too
        lone = hw.host_ladder(ens, 20)
        ens.prune_begin(*hw.SPARSE, 1, 3, 128)
        assert np.array_equal(hw.host_ladder(ens, 20), lone)


def test_twins_made_before_and_after_a_prune_give_the_heads_masks(fc):
    """the twin aliases the head's operand copies (fp32, row tiles, split halves) only if they existed when it was made:
    a twin from before any prune makes its own, a twin from after one shares -- the same masks either way, under each
    screen selection"""
    case = hw.build(SMALL)
    want = {thr: oracle_mask(SMALL, thr) for thr in (hw.SPARSE, hw.DENSE)}
    try:
        for kind in (0, 32, 64):
            fc._lib.screen_select(kind)
            with fc.DeviceEnsemble(case.X, center=True) as early, fc.DeviceEnsemble(case.X, center=True) as late:
                t_early = early.twin()
                assert np.array_equal(late.prune(*hw.SPARSE)[0], want[hw.SPARSE])
                t_late = late.twin()
                for name, h in (("twin made early", t_early), ("its head", early), ("twin made late", t_late), ("its head", late)):
                    for thr in (hw.SPARSE, hw.DENSE, hw.SPARSE):
                        mask, stats = h.prune(*thr)
                        assert np.array_equal(mask, want[thr]), (kind, name, thr)
                        assert stats[2] == np.triu(oracle_similar(SMALL, thr), 1).sum(), (kind, name, thr)
    finally:
        fc._lib.screen_select(0)


def test_min_per_group_20_then_1_then_20_on_one_handle(fc):
    """the ladder values that can run depend on min_per_group (and are cached with the handle)"""
    case = hw.build(SMALL)
    want = {m: oracle_mask(SMALL, hw.DENSE, case.energies, m) for m in (20, 1)}
    assert not np.array_equal(want[20], want[1])
    with fc.DeviceEnsemble(case.X, center=True) as ens:
        for m in (20, 1, 20, 1):
            mask, stats = ens.prune(*hw.DENSE, energies=case.energies, max_dE=hw.MAX_DE, min_per_group=m)
            assert np.array_equal(mask, want[m]), m
            assert stats[5] == want[m].sum()


def test_energies_given_then_none_then_other_energies(fc):
    """the energies stay on the handle's device buffer: a call without them must not see the last call's"""
    case = hw.build(SMALL)
    runs = [case.energies, None, case.energies2, None, case.energies]
    want = [oracle_mask(SMALL, hw.DENSE, e) for e in runs]
    assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[0], want[2]) and not np.array_equal(want[1], want[2])
    with fc.DeviceEnsemble(case.X, center=True) as ens:
        for e, ref in zip(runs, want):
            mask, _ = ens.prune(*hw.DENSE, energies=e, max_dE=hw.MAX_DE if e is not None else 0.0)
            assert np.array_equal(mask, ref)
            bits, _ = ens.simbits(*hw.DENSE, energies=e, max_dE=hw.MAX_DE if e is not None else 0.0)
            S = fc._lib.unpack_bits(bits, case.N)
            window = np.ones_like(S) if e is None else np.abs(e[:, None] - e[None, :]) < hw.MAX_DE
            assert np.array_equal(S, np.triu(oracle_similar(SMALL, hw.DENSE) & window, 1))


def test_sharding_changes_between_prunes_on_one_handle(fc):
    """rank 1 of 3 with row blocks of 128, a whole prune, then rank 0 of 2 with row blocks of 256: each rank's levels,
    merged over the logical ranks on the host, give the single-rank mask"""
    case = hw.build(SMALL)
    with fc.DeviceEnsemble(case.X, center=True) as ens, fc.DeviceEnsemble(case.X, center=True) as h1, \
            fc.DeviceEnsemble(case.X, center=True) as h2:
        single = {}
        for thr in (hw.DENSE, hw.SPARSE):
            h2.prune_begin(*thr, 0, 1, 128)
            single[thr] = hw.host_ladder(h2, 20)
            assert np.array_equal(single[thr], oracle_mask(SMALL, thr))
        pairs = int(ens.prune_begin(*hw.DENSE, 1, 3, 128)[0]) + int(h1.prune_begin(*hw.DENSE, 0, 3, 128)[0]) + \
            int(h2.prune_begin(*hw.DENSE, 2, 3, 128)[0])
        assert pairs == case.N * (case.N - 1) // 2
        assert np.array_equal(hw.host_ladder(ens, 20, ranks=[h1, ens, h2]), single[hw.DENSE])
        assert np.array_equal(ens.prune(*hw.SPARSE)[0], single[hw.SPARSE])
        pairs = int(ens.prune_begin(*hw.SPARSE, 0, 2, 256)[0]) + int(h1.prune_begin(*hw.SPARSE, 1, 2, 256)[0])
        assert pairs == case.N * (case.N - 1) // 2
        assert np.array_equal(hw.host_ladder(ens, 20, ranks=[ens, h1]), single[hw.SPARSE])
        assert np.array_equal(np.sort(np.concatenate([ens.similar_pairs(), h1.similar_pairs()])),
                              packed(oracle_similar(SMALL, hw.SPARSE)))
