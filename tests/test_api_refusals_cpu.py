"""The refusals of the neighbour, bench-hook and cluster entry points, pinned: return code AND error text.

Every check below happens on the host before any device is touched, so no GPU is needed: the handles are NULL, or the
call is refused (or is empty, N = 0) before it would need one.  For each entry point one argument at a time leaves a
baseline of valid values; what comes back -- (code, fc_last_error() text) -- also pins the ORDER in which bad arguments
are judged, because the baseline's NULL handle is itself a refusal that the varied argument has to come in front of.

tests/golden/api_refusals.json was written by this file's ``__main__`` from the library built at the commit BEFORE the C
API file was split by domain (FC_LIB_PATH=<that build's libfc_hip.so> python tests/test_api_refusals_cpu.py --write), and
is not to be regenerated from the tree under test: a refusal that changes is a change of the ABI's behaviour.
"""

import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from firecode_amd import _lib  # noqa: E402
from firecode_amd.symmetry import PERM_MAX  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "api_refusals.json")
KNN_MAX = _lib.KNN_MAX

# ---- the arguments of each entry point, in the order of include/fc_hip.h -------------------------------------------
_TABLE = ["perms", "K", "A_sel"]
_SYM = _TABLE + ["mirror"]
_LIST = ["indices32", "dist"]
_TIMES = ["reps", "ms_device", "ms_host"]
_THR = ["max_rmsd", "max_dev"]
_EN = ["energies", "max_dE"]
_CC = ["labels", "reps_out", "sizes", "n_clusters"]
_DB = ["labels", "reps_out", "sizes", "core", "degrees", "n_clusters"]
_BU = ["labels", "reps_out", "sizes", "degrees", "n_clusters"]

PARAMS = {
    "fc_ensemble_select_diverse": ["ens", "n_max", "start", "stop_rmsd", "indices64", "radii", "labels", "dist", "n_selected"],
    "fc_ensemble_select_diverse_perm": ["ens"] + _SYM + ["n_max", "start", "stop_rmsd", "indices64", "radii", "labels", "dist",
                                                         "n_selected"],
    "fc_ensemble_knn": ["ens", "k"] + _LIST,
    "fc_ensemble_knn_cross": ["queries", "refs", "k", "max_rmsd"] + _LIST,
    "fc_ensemble_knn_perm": ["ens"] + _SYM + ["k"] + _LIST,
    "fc_ensemble_knn_cross_perm": ["queries", "refs"] + _SYM + ["k", "max_rmsd"] + _LIST,
    "fc_bench_select_diverse": ["ens", "n_max", "start", "stop_rmsd"] + _TIMES + ["indices64", "n_selected", "lanes"],
    "fc_bench_select_diverse_perm": ["ens"] + _SYM + ["n_max", "start", "stop_rmsd"] + _TIMES + ["indices64", "n_selected",
                                                                                                 "sym_stats"],
    "fc_bench_knn": ["ens", "k"] + _TIMES + ["strips"],
    "fc_bench_knn_cross": ["queries", "refs", "k", "max_rmsd"] + _TIMES + ["strips"],
    "fc_bench_knn_perm": ["ens"] + _SYM + ["k"] + _TIMES + ["strips", "sym_stats"],
    "fc_bench_knn_cross_perm": ["queries", "refs"] + _SYM + ["k", "max_rmsd"] + _TIMES + ["strips", "sym_stats"],
    "fc_rmsd_clusters": ["ens"] + _THR + _EN + _CC + ["stats"],
    "fc_rmsd_clusters_enant": ["ens"] + _THR + _EN + _CC + ["stats"],
    "fc_rmsd_clusters_perm": ["ens"] + _TABLE + _THR + _EN + _CC + ["stats"],
    "fc_clusters_from_pairs": ["pairs", "n_pairs", "N"] + _CC,
    "fc_clusters_from_bits": ["bits", "N"] + _CC,
    "fc_rmsd_dbscan": ["ens"] + _THR + ["min_samples"] + _EN + _DB + ["stats"],
    "fc_rmsd_dbscan_enant": ["ens"] + _THR + ["min_samples"] + _EN + _DB + ["stats"],
    "fc_rmsd_dbscan_perm": ["ens"] + _TABLE + _THR + ["min_samples"] + _EN + _DB + ["stats"],
    "fc_dbscan_from_pairs": ["pairs", "n_pairs", "N", "min_samples"] + _DB,
    "fc_dbscan_from_bits": ["bits", "N", "min_samples"] + _DB,
    "fc_rmsd_butina": ["ens"] + _THR + _EN + _BU + ["stats"],
    "fc_rmsd_butina_enant": ["ens"] + _THR + _EN + _BU + ["stats"],
    "fc_rmsd_butina_perm": ["ens"] + _TABLE + _THR + _EN + _BU + ["stats"],
    "fc_butina_from_pairs": ["pairs", "n_pairs", "N"] + _BU,
    "fc_butina_from_bits": ["bits", "N"] + _BU,
}
NEIGHBOURS = [n for n in PARAMS if "knn" in n or "diverse" in n]
LABELS = [n for n in PARAMS if n not in NEIGHBOURS]
assert len(NEIGHBOURS) == 12 and len(LABELS) == 15

_OUTPUTS = ("indices32", "indices64", "dist", "radii", "labels", "reps_out", "sizes", "core", "degrees")


def _pair(i, j):
    return (i << 32) | j


def _baseline():
    """valid values for every argument name; the handles are NULL"""
    i32, i64, f64, u8, u64 = np.int32, np.int64, np.float64, np.uint8, np.uint64
    return {
        "ens": None, "queries": None, "refs": None,
        "perms": np.array([[0, 1, 2, 3], [1, 0, 2, 3]], dtype=i32), "K": 2, "A_sel": 4, "mirror": 0,
        "n_max": 4, "start": 0, "stop_rmsd": 0.0, "k": 2, "max_rmsd": 0.5, "max_dev": 1.0, "min_samples": 2,
        "energies": None, "max_dE": 0.0, "reps": 1,
        "ms_device": np.zeros(1, f64), "ms_host": np.zeros(1, f64), "strips": np.zeros(1, i64), "lanes": np.zeros(1, i64),
        "sym_stats": np.zeros(2, i64), "stats": np.zeros(8, i64), "n_selected": np.zeros(1, i64), "n_clusters": np.zeros(1, i64),
        "indices32": np.zeros(64, i32), "indices64": np.zeros(64, i64), "dist": np.zeros(64, f64), "radii": np.zeros(64, f64),
        "labels": np.zeros(64, i32), "reps_out": np.zeros(64, i64), "sizes": np.zeros(64, i64), "core": np.zeros(64, u8),
        "degrees": np.zeros(64, i32),
        "pairs": np.array([_pair(0, 1)], dtype=u64), "n_pairs": 1, "N": 4, "bits": np.zeros(4, u64),
    }


# name -> the arguments that leave the baseline.  A variation applies to an entry point that has all of its arguments.
VARIATIONS = {
    "baseline (NULL handles)": {},
    "k=0": {"k": 0},
    "k=-1": {"k": -1},
    "k=FC_KNN_MAX+1": {"k": KNN_MAX + 1},
    "reps=0": {"reps": 0},
    "reps=4097": {"reps": 4097},
    "ms pointers NULL": {"ms_device": None, "ms_host": None},
    "max_rmsd=0": {"max_rmsd": 0.0},
    "max_rmsd=nan": {"max_rmsd": float("nan")},
    "max_rmsd=0 and k=0": {"max_rmsd": 0.0, "k": 0},
    "max_dev=0": {"max_dev": 0.0},
    "perms NULL": {"perms": None},
    "K=0": {"K": 0},
    "K=FC_PERM_MAX+1": {"K": PERM_MAX + 1},
    "A_sel=0": {"A_sel": 0},
    "non-permutation row": {"perms": np.array([[0, 1, 2, 3], [1, 1, 2, 3]], dtype=np.int32)},
    "index outside the row": {"perms": np.array([[0, 1, 2, 3], [1, 0, 2, 4]], dtype=np.int32)},
    "non-identity first row": {"perms": np.array([[1, 0, 2, 3], [0, 1, 2, 3]], dtype=np.int32)},
    "not closed under inverse": {"perms": np.array([[0, 1, 2, 3], [1, 2, 0, 3]], dtype=np.int32)},
    "mirror=2": {"mirror": 2},
    "mirror=2 and k=0": {"mirror": 2, "k": 0},
    "K=0 and reps=0": {"K": 0, "reps": 0},
    "min_samples=0": {"min_samples": 0},
    "min_samples=0 and max_rmsd=0": {"min_samples": 0, "max_rmsd": 0.0},
    "n_max=0": {"n_max": 0},
    "stop_rmsd=nan": {"stop_rmsd": float("nan")},
    "n_clusters NULL": {"n_clusters": None},
    "n_selected NULL": {"n_selected": None},
    "lists NULL": {"indices32": None, "dist": None},
    "n_pairs=-1": {"n_pairs": -1},
    "N=-1": {"N": -1},
    "N=2^31, no pairs": {"N": 1 << 31, "n_pairs": 0},
    "N=2^31, NULL bits": {"N": 1 << 31, "bits": None},
    "self-pair": {"pairs": np.array([_pair(0, 1), _pair(2, 2)], dtype=np.uint64), "n_pairs": 2},
    "pair outside [0, N)": {"pairs": np.array([_pair(0, 4)], dtype=np.uint64)},
    "pairs NULL": {"pairs": None},
    "bits NULL": {"bits": None},
    "N=0, no pairs, NULL outputs": {"N": 0, "n_pairs": 0, "pairs": None, "@outputs": None},
    "N=0, NULL bits and outputs": {"N": 0, "bits": None, "@outputs": None},
    "N=0, no pairs, n_clusters NULL": {"N": 0, "n_pairs": 0, "n_clusters": None},
    "N=0, NULL bits, n_clusters NULL": {"N": 0, "bits": None, "n_clusters": None},
    "N=0, no pairs, min_samples=0": {"N": 0, "n_pairs": 0, "min_samples": 0},
    "N=0, NULL bits, min_samples=0": {"N": 0, "bits": None, "min_samples": 0},
}


def cases(entry):
    """(case name, {argument: value}) of one entry point: the variations all of whose arguments it has ("@outputs":
    every output array it has).  The entry points that take the caller's graph have no handle to refuse: their baseline
    would go on to the device, so it is left out."""
    names = PARAMS[entry]
    for label, change in VARIATIONS.items():
        if not set(change) - {"@outputs"} <= set(names) or ("N" in names and not change):
            continue
        change = dict(change)
        if "@outputs" in change:
            del change["@outputs"]
            change.update({o: None for o in _OUTPUTS if o in names})
        yield label, change


def run_case(lib, entry, change):
    names, argtypes = PARAMS[entry], _lib._SIGNATURES[entry]
    assert len(names) == len(argtypes), entry
    values = _baseline()
    values.update(change)
    args = []
    for name, ctype in zip(names, argtypes):
        v = values[name]
        args.append(v.ctypes.data_as(ctype) if isinstance(v, np.ndarray) else v)
    rc = getattr(lib, entry)(*args)
    return [int(rc), lib.fc_last_error().decode("utf-8", "replace") if rc != 0 else ""]


def collect(lib):
    return {f"{entry}::{label}": run_case(lib, entry, change) for entry in PARAMS for label, change in cases(entry)}


@pytest.fixture(scope="module")
def golden_refusals():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_every_case_is_in_the_golden_file_and_the_reverse(golden_refusals):
    mine = {f"{entry}::{label}" for entry in PARAMS for label, _ in cases(entry)}
    assert mine == set(golden_refusals)
    assert len(mine) >= 250


@pytest.mark.parametrize("entry", sorted(PARAMS))
def test_refusals_are_the_golden_ones(entry, golden_refusals):
    lib = _lib.load()
    wrong = []
    for label, change in cases(entry):
        got, want = run_case(lib, entry, change), golden_refusals[f"{entry}::{label}"]
        if got != want:
            wrong.append((label, got, want))
    assert not wrong, wrong


def test_the_cases_refuse_in_more_than_one_place(golden_refusals):
    """the table would pin little if every case ended at the NULL handle: most texts appear, and the empty calls pass"""
    texts = {text for _, text in golden_refusals.values()}
    assert len(texts) >= 25
    assert any(code == 0 for code, _ in golden_refusals.values())
    assert {code for code, _ in golden_refusals.values()} == {0, _lib.FC_E_INVALID, _lib.FC_E_LIMIT}


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: FC_LIB_PATH=<libfc_hip.so of the commit before the split> python tests/test_api_refusals_cpu.py --write")
    table = collect(_lib.load())
    with open(GOLDEN, "w") as fh:
        json.dump(table, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{len(table)} cases from {_lib.LIB_PATH} -> {GOLDEN}")
