"""NumPy restatement of the symmetry- and mirror-aware medoids, k-medoids and silhouettes (fc_ensemble_medoids_perm,
fc_ensemble_kmedoids_perm, fc_ensemble_silhouette_perm, include/fc_hip.h).  Thin glue: the rows of
d_sym from ``knn_sym_ref.self_rows`` go into the restatements of the plain contracts, which take rows as they come --
``medoid_ref.medoids_from_rows`` (one evaluation per unordered pair, row i < column j), ``medoid_ref.kmedoids_from_rows``
(its diverse start runs on the same rows) and ``silhouette_ref.silhouette_from_rows`` (the full square).  Test
infrastructure: the product never imports it."""

import knn_sym_ref as ks
import medoid_ref as mr
import silhouette_ref as sil
from knn_sym_ref import prepared  # noqa: F401  (re-exported for the tests)


def rows(X, atoms, table, mirror=False):
    """(N, N): d_sym of every ordered pair of the prepared ensemble; ``table`` over the selected atoms"""
    return ks.self_rows(prepared(X, atoms), table, mirror)


def medoids(D, labels=None, n_groups=None):
    return mr.medoids_from_rows(D, labels, n_groups)


def kmedoids(D, n, init=None, max_iter=50):
    return mr.kmedoids_from_rows(D, n, init=init, max_iter=max_iter)


def silhouette(D, labels=None, n_groups=None):
    return sil.silhouette_from_rows(D, labels, n_groups)
