"""The sparse ladder reference of the GPU ladder tests (tests/ladder_ref.py), on the CPU.

Two things are pinned here, so that tests/test_gpu_ladder.py can compare bit for bit and cannot weaken silently:
the reference equals the dense oracle and the literal sequential loop, and every input the GPU tests call an edge case
gives a DIFFERENT result under the mutant of the reference that gets that edge wrong."""

import numpy as np
import pytest

import ladder_ref as lr
from oracle import cpu_ref as o

SIZES = (2, 3, 63, 64, 65, 130, 300, 1000)


def _kinds(n):
    return [k for k in lr.KINDS if k != "complete" or n <= lr.COMPLETE_MAX_N]


def test_ladder_values_are_the_oracles():
    assert lr.LADDER == tuple(o.LADDER)


@pytest.mark.parametrize("n", SIZES)
def test_reference_equals_the_dense_oracle_and_the_sequential_loop(n):
    for kind in _kinds(n):
        i, j = lr.make_graph(kind, n, seed=1)
        assert ((i < j) & (j < n) & (i >= 0)).all()
        S = lr.dense_from_pairs(n, i, j)
        for mpg in (1, 2, 20):
            for drop in ("earlier", "later"):
                mask, levels = lr.ladder_from_pairs(n, i, j, mpg, drop)
                what = (kind, n, mpg, drop)
                assert np.array_equal(mask, o.greedy_prune_from_matrix(S, min_per_group=mpg, drop=drop)), what
                trace = []
                if n <= 300:
                    seq = o.greedy_prune(n, lambda a, b: S[a, b], min_per_group=mpg, drop=drop, trace=trace)
                    assert np.array_equal(mask, seq), what
                    assert levels == len(trace), what
                vm, vl = lr.ladder_variant(n, i, j, mpg, drop, mutant=None)
                assert np.array_equal(vm, mask) and vl == levels, what


def test_graph_kinds_have_the_advertised_shape():
    n = 4099
    i, j = lr.make_graph("random", n)
    assert 2.9 * n < i.shape[0] <= 3 * n
    i, j = lr.make_graph("band", n)
    assert (j - i).min() == 1 and (j - i).max() == 40 and i.shape[0] > 2.9 * n
    i, j = lr.make_graph("chain", n)
    assert np.array_equal(i, np.arange(n - 1)) and np.array_equal(j, i + 1)
    i, j = lr.make_graph("star", n)
    hubs, deg = np.unique(j, return_counts=True)
    assert np.array_equal(hubs, np.arange(96, n, 97)) and (deg == 96).all()
    i, j = lr.make_graph("cross", n)
    assert set(np.unique(j - i)) == {1, 2, 3, n // 200 + 1, n // 20 + 1, n // 2}
    assert lr.make_graph("empty", n)[0].shape[0] == 0
    assert lr.make_graph("complete", 130)[0].shape[0] == 130 * 129 // 2
    for kind in lr.KINDS:  # seeded: the CPU and the GPU tests see the same graph
        a, b = lr.make_graph(kind, 130, seed=3), lr.make_graph(kind, 130, seed=3)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("n", (65, 300, 4099))
def test_dirty_words_hold_the_same_graph(n):
    for kind in ("random", "cross", "star"):
        i, j = lr.make_graph(kind, n, seed=2)
        w = lr.dirty_words(n, i, j, seed=2)
        wi, wj = (w >> np.uint64(32)).astype(np.int64), (w & np.uint64(0xFFFFFFFF)).astype(np.int64)
        assert (w == lr.PAD).any() and (wj <= wi).any() and (wj >= n).any()
        assert w.shape[0] > np.unique(w).shape[0]  # duplicates
        ok = (wj > wi) & (wj < n)
        assert set(zip(wi[ok], wj[ok])) == set(zip(i, j))
        for drop in ("earlier", "later"):
            a, b = lr.ladder_from_pairs(n, wi, wj, 20, drop), lr.ladder_from_pairs(n, i, j, 20, drop)
            assert np.array_equal(a[0], b[0]) and a[1] == b[1]


# ---- each directed case of tests/test_gpu_ladder.py separates the mutant of the edge it claims ------------------------
def _differs(n, i, j, mpg, mutant, drop="earlier"):
    mask, levels = lr.ladder_from_pairs(n, i, j, mpg, drop)
    vm, vl = lr.ladder_variant(n, i, j, mpg, drop, mutant=mutant)
    return not np.array_equal(mask, vm), levels != vl


@pytest.mark.parametrize("n,mpg,kinds", lr.REMAINDER_CASES)
def test_remainder_cases_separate_the_clamp_and_the_last_chunk(n, mpg, kinds):
    """n % k large against n // k at a level that runs, and pairs inside the remainder: a ladder that does not clamp
    the chunk index, or that ends the last chunk at k * chunk, gives another mask"""
    for kind in kinds:
        i, j = lr.make_graph(kind, n)
        for mutant in ("no_clamp", "short_last"):
            assert _differs(n, i, j, mpg, mutant)[0], (kind, n, mpg, mutant)
    if n <= 4099:  # (the chain is run at these sizes; it separates the clamp)
        assert _differs(n, *lr.make_graph("chain", n), mpg, "no_clamp")[0]


def test_round_sizes_would_not_separate_them():
    """(why the GPU tests do not use n = 1000: no level has a remainder there)"""
    i, j = lr.make_graph("cross", 1000)
    for mutant in ("no_clamp", "short_last"):
        assert _differs(1000, i, j, 20, mutant) == (False, False)


def test_run_rule_case_separates_less_from_less_or_equal():
    n, i, j, mpg = lr.run_rule_case()
    mask, levels = lr.ladder_from_pairs(n, i, j, mpg)
    assert not mask[19] and not mask[21] and mask.sum() == n - 2
    vm, vl = lr.ladder_variant(n, i, j, mpg, mutant="run_le")
    assert vm[19] and not vm[21] and vl == levels + 1
    S = lr.dense_from_pairs(n, i, j)
    assert np.array_equal(mask, o.greedy_prune(n, lambda a, b: S[a, b], min_per_group=mpg))


@pytest.mark.parametrize("n,mpg", lr.STOP_CASES)
def test_stop_cases_count_another_level_under_less_or_equal(n, mpg):
    """the chain leaves few survivors early; the levels behind must stop exactly where the reference's do -- the count
    of levels run (which the GPU tests compare) differs under ``<=``"""
    i, j = lr.make_graph("chain", n)
    for drop in ("earlier", "later"):
        assert _differs(n, i, j, mpg, "run_le", drop)[1], (n, mpg, drop)


def test_empty_graph_counts_levels_and_the_run_rule_shows_in_the_count():
    for n in (2, 3, 63, 64, 65, 130, 300, 1003, 4099):
        for mpg in (1, 2, 20):
            mask, levels = lr.ladder_from_pairs(n, [], [], mpg)
            assert mask.all() and levels == sum(1 for k in lr.LADDER if k == 1 or mpg * k < n)
    assert lr.ladder_from_pairs(2, [], [], 1)[1] == 1 and lr.ladder_variant(2, [], [], 1, mutant="run_le")[1] == 2


@pytest.mark.parametrize("n", (63, 64, 65, 130, 300, 1003, 4099, 20011))
def test_chain_separates_feedback_inside_a_level(n):
    i, j = lr.make_graph("chain", n)
    for mpg in (1, 20):
        for drop in ("earlier", "later"):
            assert _differs(n, i, j, mpg, "feedback", drop)[0], (n, mpg, drop)


@pytest.mark.parametrize("n", (65, 300, 4099, 20011))
def test_drop_rule_changes_every_graph_with_an_edge(n):
    for kind in _kinds(n):
        i, j = lr.make_graph(kind, n)
        if i.shape[0] == 0:  # (empty; the star below its first hub)
            continue
        for mpg in (1, 20):
            assert _differs(n, i, j, mpg, "drop_swapped")[0], (kind, n, mpg)
