"""The greedy k-ladder of the RMSD prunes, fed from chosen graphs, in each of its device forms.

The prunes reach the ladder behind the similarity kernels, so the rest of the suite shows it only the graphs that
synthetic ensembles make.  Here the graph is the input: fc_debug_ladder_from_pairs runs one chosen form (0 the
bit-matrix levels, 1 the one-workgroup pair ladder, 2 the launch-per-level pair ladder with a chosen grid) and the
production entry points (greedy_prune_from_bits, prune_from_pairs, the gathered and the deferred paths) run whatever
they pick.  Every comparison is bit for bit against tests/ladder_ref.py, the count of levels run included; there are no
tolerances.  tests/test_ladder_cpu.py pins that reference to the oracle and proves that the directed cases below
separate the wrong ladders they are meant to catch.

The device buffers of the gathered paths are made with the HIP runtime the library itself is bound to (ctypes), not
with torch: torch's wheel carries a HIP runtime of its own, and two runtimes in one process cannot both own the GPU
(tests/test_gpu_torch_interop.py runs in a child interpreter for that reason)."""

import ctypes as C
import time

import numpy as np
import pytest

import ladder_ref as lr

pytestmark = pytest.mark.gpu

FORMS = ((0, 0), (1, 0), (2, 1), (2, 2), (2, 16), (2, 64))  # (form, workgroups per level of form 2)
PAIR_FORMS = FORMS[1:]
SMALL = (2, 3, 63, 64, 65, 130, 300, 1003, 4099)
ENTRY_SIZES = (65, 300, 4099, 20011)
PAIRS_NONE = 0xFFFFFFFFFFFFFFFE


def _kinds(n):
    return [k for k in lr.KINDS if k != "complete" or n <= lr.COMPLETE_MAX_N]


def _run_form(words, n, mpg, form, grid):
    from firecode_amd import _lib as L

    words = np.ascontiguousarray(words, dtype=np.uint64)
    mask = np.zeros(n, dtype=np.uint8)
    levels = C.c_int64(-1)
    L.call("fc_debug_ladder_from_pairs", L.pw(words), int(words.shape[0]), int(n), int(mpg), int(form), int(grid),
           L.pb(mask), C.byref(levels))
    return mask.astype(bool), levels.value


def _check_forms(n, i, j, mpg, forms, drop="earlier", words=None, what=()):
    ref, ref_levels = lr.ladder_from_pairs(n, i, j, mpg, drop)
    words = lr.pack_pairs(i, j) if words is None else words
    for form, grid in forms:
        mask, levels = _run_form(words, n, mpg, form, grid)
        where = what + (n, mpg, drop, "form", form, "grid", grid)
        assert np.array_equal(mask, ref), where + ("differs at", np.flatnonzero(mask != ref)[:8])
        assert levels == ref_levels, where


def _entry_words(n, i, j, seed):
    """the list as a careless caller sends it (ladder_ref.dirty_words) where the ladder's cap on the list's length,
    min(2^20, max(1024, n (n - 1) / 2)) words, leaves room for the litter; the complete graph fills the cap by itself and
    goes shuffled only"""
    words = lr.dirty_words(n, i, j, seed=seed)
    if words.shape[0] > min(2 ** 20, max(1024, n * (n - 1) // 2)):
        words = lr.pack_pairs(i, j)[np.random.default_rng(seed).permutation(i.shape[0])]
    return words


def _limit(fn):
    from firecode_amd import _lib as L

    with pytest.raises(L.FirecodeHipInputError) as err:
        fn()
    assert err.value.code == L.FC_E_LIMIT, err.value
    return err.value


# ---- every form on every graph kind -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SMALL)
def test_every_form_on_every_graph_kind(fc, n):
    """n = 300 at min_per_group = 1: chunks of 1 to 3 nodes, the remainder chunk a third of the array.  Grid 1: workgroup
    0 is also the last one.  empty: every level runs with empty buckets, the mask stays all ones and the levels are
    still counted.  chain and star at 4099: few survivors early, the levels behind stop where the reference's do."""
    for kind in _kinds(n):
        i, j = lr.make_graph(kind, n)
        for mpg in (1, 2, 20):
            _check_forms(n, i, j, mpg, FORMS, what=(kind,))
            if kind == "empty":
                assert lr.ladder_from_pairs(n, i, j, mpg)[0].all()


@pytest.mark.parametrize("kind", [k for k in lr.KINDS if k != "complete"])
def test_every_form_at_twenty_thousand(fc, kind):
    i, j = lr.make_graph(kind, 20011)
    _check_forms(20011, i, j, 20, FORMS, what=(kind,))


def test_run_rule_is_strict(fc):
    """min_per_group * k == active when level k is reached: the level must not run (ladder_ref.run_rule_case)"""
    n, i, j, mpg = lr.run_rule_case()
    _check_forms(n, i, j, mpg, FORMS)


# ---- stride wrap and the LDS limit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("random", "band", "cross"))
@pytest.mark.parametrize("n", (70001, 245760))
def test_pair_ladders_beyond_one_stride_and_at_the_lds_limit(fc, n, kind):
    """70 001: 1 094 mask words, the 1 024-thread loops over the words wrap.  245 760: 3 840 words, the two masks fill
    exactly the 60 KB the pair ladders allow themselves."""
    i, j = lr.make_graph(kind, n)
    _check_forms(n, i, j, 20, PAIR_FORMS, what=(kind,))


def test_pair_ladders_refuse_what_they_cannot_hold(fc):
    from firecode_amd import _lib as L

    n = 245761
    words = lr.pack_pairs(*lr.make_graph("cross", n))
    for form, grid in PAIR_FORMS:  # one mask word too many for the LDS: never another form in its place
        _limit(lambda: _run_form(words, n, 20, form, grid))
    # a list longer than min(2^20, max(1024, n (n - 1) / 2)), made of duplicates: the pair forms decline, the bit matrix
    # does not care
    n = 65
    i, j = lr.make_graph("random", n)
    long_words = np.tile(lr.pack_pairs(i, j), 2080 // i.shape[0] + 2)
    assert long_words.shape[0] > max(1024, n * (n - 1) // 2)
    for form, grid in PAIR_FORMS:
        _limit(lambda: _run_form(long_words, n, 1, form, grid))
    _check_forms(n, i, j, 1, FORMS[:1], words=long_words)
    at_cap = long_words[: max(1024, n * (n - 1) // 2)]  # exactly the cap is taken
    _check_forms(n, i, j, 1, FORMS, words=at_cap)
    with pytest.raises(L.FirecodeHipInputError):
        _run_form(long_words, n, 1, 3, 16)
    with pytest.raises(L.FirecodeHipInputError):
        _run_form(long_words, n, 1, 2, 0)


def _free_device_bytes(fc):
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert _hip().hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_prune_from_pairs_dense_rebuild_beyond_the_lds_limit(fc):
    """n = 245 761 does not fit the pair ladders: fc_prune_from_pairs scatters the list into the whole bit matrix
    (about 7.6 GB) and runs the bit-matrix levels"""
    n = 245761
    if _free_device_bytes(fc) < 12 * 2 ** 30:
        pytest.skip("less than 12 GB of device memory free")
    i, j = lr.make_graph("cross", n)
    ref, _ = lr.ladder_from_pairs(n, i, j, 20)
    with fc.DeviceEnsemble(np.zeros((n, 1, 3))) as ens:
        t0 = time.perf_counter()
        mask = ens.prune_from_pairs(lr.pack_pairs(i, j), 20)
        print(f"dense rebuild at n = {n}: {time.perf_counter() - t0:.2f} s")
    from firecode_amd import _lib as L

    L.memory_trim()
    assert np.array_equal(mask, ref), np.flatnonzero(mask != ref)[:8]


# ---- the production entry points, from graphs -------------------------------------------------------------------------
@pytest.mark.parametrize("n", (65, 300, 4099))
def test_greedy_prune_from_bits_on_graphs(fc, n):
    for kind in _kinds(n):
        i, j = lr.make_graph(kind, n, seed=5)
        bits = lr.bits_from_pairs(n, i, j)
        for mpg in (1, 20):
            ref, _ = lr.ladder_from_pairs(n, i, j, mpg)
            assert np.array_equal(fc.pruner.greedy_prune_from_bits(bits, n, min_per_group=mpg), ref), (kind, n, mpg)


@pytest.mark.parametrize("n", ENTRY_SIZES)
def test_prune_from_pairs_on_graphs(fc, n):
    """an ensemble of one-atom structures (the coordinates play no part) and lists as a careless caller sends them: pad
    words, entries with j <= i and j >= n, duplicates, shuffled"""
    with fc.DeviceEnsemble(np.zeros((n, 1, 3))) as ens:
        for kind in _kinds(n):
            i, j = lr.make_graph(kind, n, seed=6)
            words = _entry_words(n, i, j, seed=6)
            for mpg in (1, 20):
                ref, _ = lr.ladder_from_pairs(n, i, j, mpg)
                assert np.array_equal(ens.prune_from_pairs(words, mpg), ref), (kind, n, mpg)


def test_prune_from_pairs_list_beyond_the_kernels_cap(fc):
    """more words than min(2^20, max(1024, n (n - 1) / 2)), made of duplicates at small n: the right mask or FC_E_LIMIT,
    never another mask -- today the refusal (the pair ladder declines and no bit matrix stands behind it)"""
    from firecode_amd import _lib as L

    n = 65
    i, j = lr.make_graph("cross", n, seed=7)
    ref, _ = lr.ladder_from_pairs(n, i, j, 1)
    words = np.tile(lr.dirty_words(n, i, j, seed=7), 12)
    assert max(1024, n * (n - 1) // 2) < words.shape[0] <= 2 ** 20
    with fc.DeviceEnsemble(np.zeros((n, 1, 3))) as ens:
        try:
            mask = ens.prune_from_pairs(words, 1)
        except L.FirecodeHipInputError as err:
            assert err.code == L.FC_E_LIMIT, err
            print("over-cap list of duplicates: FC_E_LIMIT")
        else:
            assert np.array_equal(mask, ref)
            print("over-cap list of duplicates: the right mask")
        assert np.array_equal(ens.prune_from_pairs(lr.dirty_words(n, i, j, seed=7), 1), ref)  # the ensemble still works


@pytest.mark.parametrize("n", ENTRY_SIZES)
def test_drop_later_convention_in_the_pair_forms(fc, n):
    from firecode_amd import _lib as L

    L.call("fc_prune_conventions", 1)
    try:
        for kind in _kinds(n):
            i, j = lr.make_graph(kind, n, seed=6)
            words = _entry_words(n, i, j, seed=6)
            for mpg in (1, 20):
                _check_forms(n, i, j, mpg, PAIR_FORMS, drop="later", words=words, what=(kind,))
        i, j = lr.make_graph("cross", n, seed=6)
        with pytest.raises(L.FirecodeHipInputError) as err:  # the bit-matrix levels implement the default rule only
            _run_form(lr.pack_pairs(i, j), n, 20, 0, 0)
        assert err.value.code == L.FC_E_INVALID
    finally:
        L.call("fc_prune_conventions", 0)
    _check_forms(n, i, j, 20, FORMS, what=("cross",))  # and the default is back


# ---- the gathered and the deferred paths ------------------------------------------------------------------------------
_HIP = None


def _hip():
    """the HIP runtime libfc_hip.so is bound to (already mapped: dlopen hands back the same copy)"""
    global _HIP
    if _HIP is None:
        from firecode_amd import _lib as L

        mapped = L._mapped_hip_runtimes()
        assert mapped, "libfc_hip.so is loaded, so a HIP runtime is mapped"
        hip = C.CDLL(mapped[0])
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipFree.argtypes = [C.c_void_p]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        _HIP = hip
    return _HIP


class _DeviceWords:
    """uint64 words in device memory; .ptr is what the library takes"""

    def __init__(self, host):
        host = np.ascontiguousarray(host, dtype=np.uint64)
        p = C.c_void_p()
        assert _hip().hipMalloc(C.byref(p), max(host.nbytes, 8)) == 0
        self.ptr = p.value
        assert _hip().hipMemcpy(self.ptr, host.ctypes.data, host.nbytes, 1) == 0  # (blocking, host to device)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        assert _hip().hipFree(self.ptr) == 0


def _messages(words, world, seed=0):
    """`words` dealt to `world` messages of cap + 1 words -- count, entries, padding -- of unequal lengths: message 0
    holds exactly cap entries, message 1 (world > 1) none"""
    rng = np.random.default_rng([seed, world])
    words = words[rng.permutation(words.shape[0])]
    total = words.shape[0]
    if world == 1:
        sizes = [total]
    else:
        cap = total // 2 + 1
        rest = total - cap
        cuts = np.sort(rng.integers(0, rest + 1, size=world - 3)) if world > 3 else np.zeros(0, dtype=np.int64)
        sizes = [cap, 0] + list(np.diff(np.concatenate([[0], cuts, [rest]])))
    cap = int(max(sizes))
    assert len(sizes) == world and sum(sizes) == total and sizes[0] == cap and (world == 1 or min(sizes) == 0)
    assert world < 3 or len(set(sizes)) > 2
    buf = np.full((world, cap + 1), lr.PAD, dtype=np.uint64)
    at = 0
    for r, c in enumerate(sizes):
        buf[r, 0] = c
        buf[r, 1: 1 + c] = words[at: at + c]
        at += c
    return buf, cap


@pytest.mark.parametrize("world", (1, 3, 8))
def test_prune_from_gathered_messages(fc, world):
    for n in (300, 4099):
        with fc.DeviceEnsemble(np.zeros((n, 1, 3))) as ens:
            for kind in ("random", "cross", "chain", "empty"):
                i, j = lr.make_graph(kind, n, seed=8)
                words = lr.dirty_words(n, i, j, seed=8)
                buf, cap = _messages(words, world, seed=8)
                with _DeviceWords(buf) as dev:
                    for mpg in (1, 20):
                        ref, _ = lr.ladder_from_pairs(n, i, j, mpg)
                        mask, stats = ens.prune_from_gathered_dev(dev.ptr, world, cap, min_per_group=mpg)
                        assert np.array_equal(mask, ref), (kind, n, world, mpg)
                        assert stats[5] == ref.sum()


def test_deferred_prunes_collected_out_of_order(fc):
    """four graphs into slots 0 .. 3 of one batch, collected as 2, 0, 3, 1"""
    n, mpg, world = 4099, 20, 3
    jobs = []
    for slot, kind in enumerate(("cross", "band", "chain", "random")):
        i, j = lr.make_graph(kind, n, seed=9 + slot)
        buf, cap = _messages(lr.dirty_words(n, i, j, seed=9), world, seed=slot)
        jobs.append((lr.ladder_from_pairs(n, i, j, mpg)[0], _DeviceWords(buf), cap))
    assert len({ref.tobytes() for ref, _, _ in jobs}) == 4
    try:
        with fc.DeviceEnsemble(np.zeros((n, 1, 3))) as ens:
            for slot, (_, dev, cap) in enumerate(jobs):
                ens.prune_from_gathered_enqueue(dev.ptr, world, cap, slot, 4, min_per_group=mpg)
            for slot in (2, 0, 3, 1):
                mask, stats = ens.prune_collect(slot, 4)
                assert np.array_equal(mask, jobs[slot][0]), slot
                assert stats[5] == jobs[slot][0].sum()
    finally:
        for _, dev, _ in jobs:
            dev.__exit__()


@pytest.mark.parametrize("bad", ("none", "too_long"))
def test_gathered_message_missing_or_too_long(fc, bad):
    """a message whose count word says "none", or more than cap: FC_E_LIMIT from the synchronous path and from
    fc_prune_collect, and the next correct prune on the same ensemble is right"""
    n, mpg, world = 300, 1, 3
    i, j = lr.make_graph("cross", n, seed=10)
    ref, _ = lr.ladder_from_pairs(n, i, j, mpg)
    good, cap = _messages(lr.dirty_words(n, i, j, seed=10), world, seed=10)
    broken = good.copy()
    broken[2, 0] = PAIRS_NONE if bad == "none" else cap + 1
    with fc.DeviceEnsemble(np.zeros((n, 1, 3))) as ens, _DeviceWords(good) as dev_good, _DeviceWords(broken) as dev_bad:
        _limit(lambda: ens.prune_from_gathered_dev(dev_bad.ptr, world, cap, min_per_group=mpg))
        mask, _ = ens.prune_from_gathered_dev(dev_good.ptr, world, cap, min_per_group=mpg)
        assert np.array_equal(mask, ref)
        ens.prune_from_gathered_enqueue(dev_bad.ptr, world, cap, 0, 2, min_per_group=mpg)
        ens.prune_from_gathered_enqueue(dev_good.ptr, world, cap, 1, 2, min_per_group=mpg)
        _limit(lambda: ens.prune_collect(0, 2))
        mask, _ = ens.prune_collect(1, 2)
        assert np.array_equal(mask, ref)
        mask, _ = ens.prune_from_gathered_dev(dev_good.ptr, world, cap, min_per_group=mpg)
        assert np.array_equal(mask, ref)
