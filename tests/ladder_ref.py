"""A sparse NumPy reference of the greedy k-ladder, and the graphs the ladder tests feed it.

The ladder (oracle.cpu_ref.greedy_prune, whose docstring is the specification): for every ladder value k with
``k == 1 or min_per_group * k < n_active`` the array is cut into k contiguous chunks of ``n // k`` (the last chunk takes
the remainder); inside a chunk a structure active at the start of the level falls to an active similar one behind it
(``drop="earlier"``) or in front of it (``drop="later"``).  Kills are read from the level's input mask and written to its
output, so over a list of similar pairs (i < j) a level is

    act = in[i] & in[j] & (c(i) == c(j)),   c(x) = min(x // chunk, k - 1),   out[i or j][act] = False

which costs O(pairs) per level: the reference serves a quarter of a million structures, where the dense oracle's
(n, n) matrix does not exist.  tests/test_ladder_cpu.py pins it to the dense oracle and to the literal sequential loop.

``ladder_variant`` is the same loop with one rule bent (the MUTANTS): the CPU tests use it to prove that an input the
GPU tests call an edge case really separates the right ladder from a subtly wrong one.
"""

import numpy as np

LADDER = (500000, 200000, 100000, 50000, 20000, 10000, 5000, 2000, 1000, 500, 200, 100, 50, 20, 10, 5, 2, 1)
PAD = np.uint64(0xFFFFFFFFFFFFFFFF)
KINDS = ("random", "band", "chain", "star", "cross", "empty", "complete")
COMPLETE_MAX_N = 300  # n (n - 1) / 2 pairs: small n only


# Directed cases of tests/test_gpu_ladder.py; tests/test_ladder_cpu.py proves on the CPU that each separates the mutant
# of the edge it claims.
# (n, min_per_group, kinds): a level runs whose remainder n % k is large against its chunk n // k, and the graph has
# pairs inside the remainder -- 300 / 1: k = 200, chunks of 1, the last chunk is [199, 300); 4099: k = 2000 or 200,
# the last chunk holds 99 nodes more than the others; 245 760 / 20: k = 10 000, chunks of 24, 5 760 nodes more
# (star and complete graphs end in the same mask however the chunks are cut: every edge acts at k = 1 at the latest and
# its killer is still there; they claim no edge of this kind)
_CUT_SENSITIVE = ("random", "band", "cross")
REMAINDER_CASES = ((300, 1, _CUT_SENSITIVE), (4099, 1, _CUT_SENSITIVE), (4099, 2, _CUT_SENSITIVE),
                   (4099, 20, _CUT_SENSITIVE), (245760, 20, _CUT_SENSITIVE))
# (n, min_per_group): the chain leaves one survivor per chunk at the first level; the levels behind must stop where the
# reference's do -- at 4099 / 20 the 200 survivors meet k = 10 with 20 * 10 == 200
STOP_CASES = ((4099, 2), (4099, 20))


def _valid(n, i, j):
    i = np.asarray(i, dtype=np.int64).reshape(-1)
    j = np.asarray(j, dtype=np.int64).reshape(-1)
    ok = (i >= 0) & (j > i) & (j < n)  # every other entry never acts
    return i[ok], j[ok]


def ladder_from_pairs(n, i, j, min_per_group=20, drop="earlier"):
    """(mask, levels_run) of the ladder over the similar pairs (i[p], j[p]).  Entries with ``j <= i`` or ``j >= n``
    never act; duplicates are harmless."""
    if drop not in ("earlier", "later"):
        raise ValueError(drop)
    i, j = _valid(n, i, j)
    kill = i if drop == "earlier" else j
    mask = np.ones(n, dtype=bool)
    levels = 0
    for k in LADDER:
        if not (k == 1 or min_per_group * k < np.count_nonzero(mask)):
            continue
        levels += 1
        chunk = n // k
        act = mask[i] & mask[j] & (np.minimum(i // chunk, k - 1) == np.minimum(j // chunk, k - 1))
        out = mask.copy()
        out[kill[act]] = False
        mask = out
    return mask, levels


MUTANTS = ("no_clamp", "run_le", "feedback", "short_last", "drop_swapped")


def ladder_variant(n, i, j, min_per_group=20, drop="earlier", mutant=None):
    """``ladder_from_pairs`` with one rule bent:

    no_clamp      the chunk index is ``x // chunk``: the remainder is cut into chunks of its own;
    run_le        a level runs while ``min_per_group * k <= n_active``;
    feedback      kills are visible inside the level (the pairs are walked one by one on the live mask, in the order
                  in which a kill can reach the next pair: from the back for "earlier", from the front for "later");
    short_last    the last chunk ends at ``k * chunk``: the remainder belongs to no chunk;
    drop_swapped  the other member of a pair falls.
    ``mutant=None`` is the right ladder (the tests check that against ``ladder_from_pairs``)."""
    if mutant is not None and mutant not in MUTANTS:
        raise ValueError(mutant)
    if mutant == "drop_swapped":
        drop = "later" if drop == "earlier" else "earlier"
    i, j = _valid(n, i, j)
    kill = i if drop == "earlier" else j
    mask = np.ones(n, dtype=bool)
    levels = 0
    for k in LADDER:
        active = np.count_nonzero(mask)
        run = k == 1 or (min_per_group * k <= active if mutant == "run_le" else min_per_group * k < active)
        if not run:
            continue
        levels += 1
        chunk = n // k
        if chunk == 0:  # (run_le alone can get here: k == n)
            continue
        ci, cj = i // chunk, j // chunk
        if mutant != "no_clamp":
            ci, cj = np.minimum(ci, k - 1), np.minimum(cj, k - 1)
        same = ci == cj
        if mutant == "short_last":
            same &= j < k * chunk
        if mutant == "feedback":
            order = np.argsort(-i, kind="stable") if drop == "earlier" else np.argsort(j, kind="stable")
            live = mask.copy()
            for p in order[same[order]]:
                if live[i[p]] and live[j[p]]:
                    live[kill[p]] = False
            mask = live
            continue
        act = mask[i] & mask[j] & same
        out = mask.copy()
        out[kill[act]] = False
        mask = out
    return mask, levels


def make_graph(kind, n, seed=0):
    """Similar pairs (i, j), all with i < j < n, of one of KINDS on n nodes; the same (kind, n, seed) gives the same
    graph in the CPU and the GPU tests."""
    rng = np.random.default_rng([seed, n, KINDS.index(kind)])
    node = np.arange(n, dtype=np.int64)
    if kind == "empty" or n < 2:
        i = j = np.zeros(0, dtype=np.int64)
    elif kind == "random":  # about 3 n pairs anywhere
        a, b = rng.integers(0, n, size=3 * n), rng.integers(0, n, size=3 * n)
        i, j = np.minimum(a, b), np.maximum(a, b)
    elif kind == "band":  # three per node, at most 40 behind it
        i = np.repeat(node, 3)
        j = i + rng.integers(1, 41, size=i.shape[0])
    elif kind == "chain":  # i -> i + 1: a kill that feeds back inside a level changes every second node
        i, j = node[:-1], node[1:]
    elif kind == "star":  # a hub every 97 nodes, similar to the 96 nodes in front of it
        j = np.repeat(np.arange(96, n, 97, dtype=np.int64), 96)
        i = j - np.tile(np.arange(1, 97, dtype=np.int64), j.shape[0] // 96)
    elif kind == "cross":  # three per node at distances that straddle the chunk borders of every level
        steps = np.array([1, 2, 3, n // 200 + 1, n // 20 + 1, max(n // 2, 1)], dtype=np.int64)
        i = np.repeat(node, 3)
        j = i + steps[rng.integers(0, steps.shape[0], size=i.shape[0])]
    elif kind == "complete":
        if n > COMPLETE_MAX_N:
            raise ValueError(f"complete graph on {n} nodes")
        i, j = np.triu_indices(n, 1)
        i, j = i.astype(np.int64), j.astype(np.int64)
    else:
        raise ValueError(kind)
    ok = (j > i) & (j < n)
    return i[ok], j[ok]


def run_rule_case():
    """(n, i, j, min_per_group) on which the outcome depends on ``<`` against ``<=`` in the run rule: n = 400 and
    min_per_group = 20, so level k = 20 (chunks of 20) is reached with 20 * 20 == 400 active and must NOT run; the
    first level that runs is k = 10 (chunks of 40).  The path 19 - 21 - 22: 21 and 22 share a chunk at k = 20, 19 and
    21 only at k = 10.  Right: k = 10 sees all three alive, 19 and 21 fall.  With ``<=``: k = 20 drops 21 first, and
    19 survives."""
    return 400, np.array([19, 21], dtype=np.int64), np.array([21, 22], dtype=np.int64), 20


def pack_pairs(i, j):
    """the library's pair words: (i << 32) | j"""
    return (np.asarray(i, dtype=np.uint64) << np.uint64(32)) | np.asarray(j, dtype=np.uint64)


def dirty_words(n, i, j, seed=0):
    """The pair words of (i, j) as a careless caller sends them: every pair, a third of them twice, pad words,
    entries with j <= i (the pair reversed, and i == j) and with j >= n, all shuffled.  Same graph."""
    rng = np.random.default_rng([seed, n, 77])
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    dup = rng.random(i.shape[0]) < 1.0 / 3.0
    m = max(8, i.shape[0] // 8)
    lo = rng.integers(0, n, size=m)
    parts = [
        pack_pairs(i, j),
        pack_pairs(i[dup], j[dup]),
        np.full(m, PAD, dtype=np.uint64),
        pack_pairs(j[dup], i[dup]),                                 # j < i
        pack_pairs(lo, lo),                                         # j == i
        pack_pairs(lo, n + rng.integers(0, 3 * n + 64, size=m)),    # j >= n
        pack_pairs(np.zeros(1, dtype=np.int64), np.array([0xFFFFFFFF], dtype=np.int64)),
    ]
    words = np.concatenate(parts)
    return words[rng.permutation(words.shape[0])]


def dense_from_pairs(n, i, j):
    """the symmetric (n, n) similarity matrix of the dense oracle"""
    i, j = _valid(n, i, j)
    S = np.zeros((n, n), dtype=bool)
    S[i, j] = True
    return S | S.T


def bits_from_pairs(n, i, j):
    """the (n, ceil(n / 64)) uint64 rows of fc_greedy_prune_from_bits: bit j of row i"""
    W = (n + 63) // 64
    padded = np.zeros((n, W * 64), dtype=np.uint8)
    padded[:, :n] = dense_from_pairs(n, i, j)
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint64)
