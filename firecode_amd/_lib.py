"""ctypes binding of libfc_hip.so (include/fc_hip.h).

The library is the product: there is no Python/NumPy fallback.  If the shared
object is missing, or no gfx950 device is usable, the calls raise
``FirecodeHipError`` -- loudly, never silently.
"""

from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FC_LIB_PATH") or os.path.join(_HERE, "libfc_hip.so")  # FC_LIB_PATH: a tuning build

FC_OK = 0
FC_E_INVALID, FC_E_NODEVICE, FC_E_HIP, FC_E_NOMEM, FC_E_LIMIT, FC_E_INTERNAL = -1, -2, -3, -4, -5, -6


class FirecodeHipError(RuntimeError):
    """Any failure reported by libfc_hip.so (code in ``.code``)."""

    def __init__(self, code, message):
        super().__init__(f"libfc_hip error {code}: {message}")
        self.code = code


class FirecodeHipInputError(FirecodeHipError, ValueError):
    """FC_E_INVALID / FC_E_LIMIT: the arguments were rejected before any launch."""


class FirecodeHipDeviceError(FirecodeHipError):
    """FC_E_NODEVICE / FC_E_HIP / FC_E_NOMEM."""


_lib = None

_p_f64 = C.POINTER(C.c_double)
_p_i64 = C.POINTER(C.c_int64)
_p_u64 = C.POINTER(C.c_uint64)
_p_u8 = C.POINTER(C.c_uint8)
_i64 = C.c_int64
_f64 = C.c_double
_ens = C.c_void_p

# name -> argtypes  (restype is always int unless noted)
_SIGNATURES = {
    "fc_abi_version": [],
    "fc_device_count": [],
    "fc_init": [C.c_int],
    "fc_shutdown": [],
    "fc_warmup": [],
    "fc_device_info": [C.c_char_p, _i64, _p_i64, _p_i64],
    "fc_ensemble_create": [_p_f64, _i64, _i64, _p_u8, C.c_int, C.POINTER(_ens)],
    "fc_ensemble_destroy": [_ens],
    "fc_ensemble_shape": [_ens, _p_i64, _p_i64],
    "fc_kabsch_rmsd_pairs": [_p_f64, _i64, _i64, _p_u8, _p_i64, _p_i64, _i64, C.c_int, _p_f64, _p_f64],
    "fc_ensemble_rmsd_pairs": [_ens, _p_i64, _p_i64, _i64, _p_f64, _p_f64],
    "fc_kabsch_rmsd_pairs_inv": [_p_f64, _i64, _i64, _p_u8, _p_i64, _p_i64, _i64, C.c_int, _p_f64, _p_f64],
    "fc_ensemble_rmsd_pairs_inv": [_ens, _p_i64, _p_i64, _i64, _p_f64, _p_f64],
    "fc_ensemble_rmsd_matrix": [_ens, _p_f64, _p_f64],
    "fc_ensemble_rmsd_values": [_ens, _p_f64, _p_f64],
    "fc_ensemble_rmsd_and_max_all": [_ens, _p_f64, _p_f64, _p_f64],
    "fc_bench_rmsd_and_max_all": [_ens, _i64, _p_f64, _p_f64, _p_i64],
    "fc_bench_rmsd_and_max_all_sampled": [_ens, _i64, _p_i64, _p_i64, _i64, _p_f64, _p_f64, _p_f64, _p_f64, _p_i64],
    "fc_bench_refine": [_ens, _f64, _f64, _i64, _p_f64, _p_i64],
    "fc_screen_select": [C.c_int],
    "fc_prune_conventions": [C.c_int],
    "fc_prune_similarity": [_p_f64, _i64, _i64, _p_u8, _p_f64, C.c_int, _f64, C.c_int, _f64, _f64, _p_f64, _f64, _i64,
                            _p_u8, _p_u8, _p_i64],
    "fc_alignment_matrices": [_p_f64, _p_f64, _i64, _i64, _p_f64],
    "fc_rmsd_simbits": [_ens, _f64, _f64, _p_f64, _f64, _i64, _i64, _p_u64, _p_i64],
    "fc_prune_rmsd": [_ens, _f64, _f64, _p_f64, _f64, _i64, _p_u8, _p_i64],
    "fc_rmsd_simbits_enant": [_ens, _f64, _f64, _p_f64, _f64, _i64, _i64, _p_u64, _p_i64],
    "fc_prune_rmsd_enant": [_ens, _f64, _f64, _p_f64, _f64, _i64, _p_u8, _p_i64],
    "fc_prune_rmsd_host": [_p_f64, _i64, _i64, _p_u8, C.c_int, _f64, _f64, _p_f64, _f64, _i64, _p_u8, _p_i64],
    "fc_greedy_prune_from_bits": [_p_u64, _i64, _i64, _p_u8],
    "fc_rmsd_clusters": [_ens, _f64, _f64, _p_f64, _f64, C.POINTER(C.c_int32), _p_i64, _p_i64, _p_i64, _p_i64],
    "fc_rmsd_clusters_enant": [_ens, _f64, _f64, _p_f64, _f64, C.POINTER(C.c_int32), _p_i64, _p_i64, _p_i64, _p_i64],
    "fc_ensemble_rmsd_pairs_perm": [_ens, C.POINTER(C.c_int32), _i64, _i64, _p_i64, _p_i64, _i64, _p_f64, _p_f64],
    "fc_rmsd_simbits_perm": [_ens, C.POINTER(C.c_int32), _i64, _i64, _f64, _f64, _p_f64, _f64, _i64, _i64, _p_u64, _p_i64],
    "fc_prune_rmsd_perm": [_ens, C.POINTER(C.c_int32), _i64, _i64, _f64, _f64, _p_f64, _f64, _i64, _p_u8, _p_i64],
    "fc_rmsd_clusters_perm": [_ens, C.POINTER(C.c_int32), _i64, _i64, _f64, _f64, _p_f64, _f64, C.POINTER(C.c_int32), _p_i64,
                              _p_i64, _p_i64, _p_i64],
    "fc_clusters_from_pairs": [_p_u64, _i64, _i64, C.POINTER(C.c_int32), _p_i64, _p_i64, _p_i64],
    "fc_clusters_from_bits": [_p_u64, _i64, C.POINTER(C.c_int32), _p_i64, _p_i64, _p_i64],
    "fc_rmsd_dbscan": [_ens, _f64, _f64, _i64, _p_f64, _f64, C.POINTER(C.c_int32), _p_i64, _p_i64, _p_u8, C.POINTER(C.c_int32),
                       _p_i64, _p_i64],
    "fc_rmsd_dbscan_enant": [_ens, _f64, _f64, _i64, _p_f64, _f64, C.POINTER(C.c_int32), _p_i64, _p_i64, _p_u8,
                             C.POINTER(C.c_int32), _p_i64, _p_i64],
    "fc_rmsd_dbscan_perm": [_ens, C.POINTER(C.c_int32), _i64, _i64, _f64, _f64, _i64, _p_f64, _f64, C.POINTER(C.c_int32), _p_i64,
                            _p_i64, _p_u8, C.POINTER(C.c_int32), _p_i64, _p_i64],
    "fc_dbscan_from_pairs": [_p_u64, _i64, _i64, _i64, C.POINTER(C.c_int32), _p_i64, _p_i64, _p_u8, C.POINTER(C.c_int32), _p_i64],
    "fc_dbscan_from_bits": [_p_u64, _i64, _i64, C.POINTER(C.c_int32), _p_i64, _p_i64, _p_u8, C.POINTER(C.c_int32), _p_i64],
    "fc_rmsd_butina": [_ens, _f64, _f64, _p_f64, _f64, C.POINTER(C.c_int32), _p_i64, _p_i64, C.POINTER(C.c_int32), _p_i64,
                       _p_i64],
    "fc_rmsd_butina_enant": [_ens, _f64, _f64, _p_f64, _f64, C.POINTER(C.c_int32), _p_i64, _p_i64, C.POINTER(C.c_int32),
                             _p_i64, _p_i64],
    "fc_rmsd_butina_perm": [_ens, C.POINTER(C.c_int32), _i64, _i64, _f64, _f64, _p_f64, _f64, C.POINTER(C.c_int32), _p_i64,
                            _p_i64, C.POINTER(C.c_int32), _p_i64, _p_i64],
    "fc_butina_from_pairs": [_p_u64, _i64, _i64, C.POINTER(C.c_int32), _p_i64, _p_i64, C.POINTER(C.c_int32), _p_i64],
    "fc_butina_from_bits": [_p_u64, _i64, C.POINTER(C.c_int32), _p_i64, _p_i64, C.POINTER(C.c_int32), _p_i64],
    "fc_prune_rmsd_begin": [_ens, _f64, _f64, _p_f64, _f64, _i64, _i64, _i64, _p_i64],
    "fc_prune_level": [_ens, _i64, _p_u8, _p_u8],
    "fc_prune_similar_pairs": [_ens, _p_u64, _i64, _p_i64],
    "fc_prune_from_pairs": [_ens, _p_u64, _i64, _i64, _p_u8],
    "fc_prune_rmsd_begin_async": [_ens, _f64, _f64, _i64, _i64, _i64],
    "fc_prune_export_pairs_dev": [_ens, C.c_void_p, _i64],
    "fc_prune_from_gathered_dev": [_ens, C.c_void_p, _i64, _i64, _i64, _p_u8, _p_i64],
    "fc_prune_from_gathered_dev_enqueue": [_ens, C.c_void_p, _i64, _i64, _i64, _i64, _i64],
    "fc_prune_collect": [_ens, _i64, _i64, _p_u8, _p_i64],
    "fc_stream_set": [C.c_void_p],
    "fc_memory_trim": [],
    "fc_host_alloc_pinned": [C.c_int64, C.POINTER(C.c_void_p)],
    "fc_host_free_pinned": [C.c_void_p],
    "fc_inertia_moments": [_p_f64, _i64, _i64, _p_f64, _p_f64],
    "fc_prune_rmsd_rot_corr": [_p_f64, _i64, _i64, _p_u8, _p_i64, _i64, _p_u8, _p_f64, C.POINTER(C.c_int32), _i64,
                               _f64, _f64, _p_f64, _f64, _i64, _p_u8, _p_u64],
    "fc_align_by_moi": [_p_f64, _i64, _i64, _p_f64, _p_f64],
    "fc_prune_moi": [_p_f64, _i64, _i64, _p_f64, _f64, _p_f64, _f64, _i64, _p_u8],
    "fc_moi_simbits": [_p_f64, _i64, _i64, _p_f64, _f64, _p_f64, _f64, _p_u64],
    "fc_align_to_first": [_p_f64, _i64, _i64, _p_i64, _i64, _p_f64],
    "fc_rototranslate": [_p_f64, _i64, _i64, _p_f64, _p_f64, _p_f64],
    "fc_clash_self": [_p_f64, _i64, _i64, _f64, _f64, _p_i64],
    "fc_clash_fragments": [_p_f64, _i64, _i64, _p_i64, _i64, _f64, _i64, _p_i64, _p_u8],
    "fc_clash_graph": [_p_f64, _i64, _i64, _p_u8, _f64, _p_i64],
    "fc_fitness_check": [_p_f64, _i64, _i64, _p_i64, _p_f64, _i64, _f64, _p_f64, _p_u8],
    "fc_bond_changes": [_p_f64, _i64, _i64, C.POINTER(C.c_int32), _i64, _p_f64, _p_f64, _i64, _p_u64, _p_i64, _p_i64,
                        _i64, _i64, _p_i64, _p_u8],
    "fc_bond_changes_list": [_p_f64, _i64, _i64, C.POINTER(C.c_int32), _i64, _p_f64, _p_f64, _i64, _p_u64, _p_i64,
                             _p_i64, _i64, _p_i64, _p_i64],
    "fc_embed_poses_clash": [_p_f64, _i64, _i64, _p_f64, _i64, _i64, _p_i64, _p_i64, _p_f64, _p_f64,
                             _p_f64, _p_f64, _i64, _f64, _i64, _p_i64, _p_u8, _p_f64],
    "fc_embed_mol_transforms": [_p_f64, _i64, _i64, _p_i64, _i64, _p_f64, _p_f64, _i64, _p_f64, _i64, _p_f64, _p_f64],
    "fc_embed_trimolecular": [C.POINTER(_p_f64), _p_i64, _p_i64, C.POINTER(_p_i64), _p_i64, _i64, _p_i64, _p_f64,
                              _p_f64, _p_f64, _p_f64, _p_u8, _p_i64, _p_f64, _p_f64, _i64, C.POINTER(C.c_int32),
                              _i64, _f64, _i64, _f64, _p_f64, _p_f64, _p_u8, _p_u8],
    "fc_embed_grid_clash": [_p_f64, _i64, _i64, _p_i64, _i64, _p_f64, _p_f64, _p_f64, _i64, _i64, _p_i64, _i64,
                            _p_f64, _p_f64, _p_f64, _i64, _p_f64, _i64, _f64, _i64, _p_u8,
                            C.POINTER(C.c_int32), _p_f64],
    "fc_embed_grid_dedupe": [_p_f64, _i64, _i64, _p_i64, _i64, _p_f64, _p_f64, _p_f64, _i64, _i64, _p_i64, _i64,
                             _p_f64, _p_f64, _p_f64, _i64, _p_f64, _i64, _f64, _i64, _f64, _p_u8, _p_u8],
    "fc_string_embed": [_p_f64, _i64, _i64, _p_f64, _p_f64, _i64, _p_f64, _i64, _i64, _p_f64, _p_f64, _i64, _p_f64, _i64,
                        _p_i64, _i64, _f64, _i64, _f64, _p_u8, _p_u8, _p_f64, _p_f64],
    "fc_torsion_scan": [_p_f64, _i64, _p_i64, _i64, _p_u8, _p_i64, _i64, _f64, _i64, _p_f64, _p_i64],
    "fc_torsion_scan_fingerprints": [_p_f64, _i64, _p_i64, _i64, _p_u8, _p_i64, _i64, _f64, _i64, _p_i64, _i64,
                                     _p_f64, _p_i64, _p_f64],
    "fc_torsion_scan_tfd": [_p_f64, _i64, _p_i64, _i64, _p_u8, _p_i64, _i64, _f64, _i64, _p_i64, _i64, _f64, _p_i64, _p_u8],
    "fc_torsion_scan_tfd_grid": [_p_f64, _i64, _p_i64, _i64, _p_u8, _p_i64, _p_i64, _f64, _i64, _p_i64, _i64, _f64, _p_i64, _p_u8],
    "fc_torsion_fingerprint": [_p_f64, _i64, _i64, _p_i64, _i64, _p_f64],
    "fc_tfd_simbits": [_p_f64, _i64, _i64, _f64, _i64, _i64, _p_u64],
    "fc_tfd_first_match": [_p_f64, _i64, _i64, _f64, _p_i64],
    "fc_tfd_last_form": [_p_i64],
    "fc_tfd_ladder_from_first_match": [_p_i64, _i64, _p_u8],
    "fc_tfd_prune": [_p_f64, _i64, _i64, _f64, _p_u8],
    "fc_debug_pyset_order_ints": [_p_i64, _i64, _p_i64, _p_i64],
    "fc_debug_pyset_order_pairs": [_p_i64, _i64, _p_i64, _p_i64],
    "fc_debug_pyset_order_pairs_device": [_p_i64, _i64, _p_i64],
    "fc_debug_tfd_ladder_emulate": [_p_i64, _i64, _p_u8],
    "fc_debug_ladder_from_pairs": [_p_u64, _i64, _i64, _i64, C.c_int, _i64, _p_u8, _p_i64],
    "fc_xyz_write": [C.c_char_p, C.POINTER(C.c_char_p), _i64, _p_f64, _i64, C.c_char_p, C.c_int],
    "fc_xyz_scan": [C.c_char_p, _p_i64, _p_i64],
    "fc_cartesian_product_i64": [_p_i64, _p_i64, _i64, _p_i64],
    "fc_cartesian_product_f64": [_p_f64, _p_i64, _i64, _p_f64],
    "fc_xyz_read": [C.c_char_p, _i64, _i64, C.c_char_p, _p_f64],
    "fc_bench_prune_rmsd": [_ens, _f64, _f64, _i64, _p_f64, _p_f64, _p_u8, _p_i64],
    "fc_stream_use": [C.c_void_p],
    "fc_ensemble_twin": [_ens, C.POINTER(_ens)],
    "fc_prune_rmsd_begin_split_async": [_ens, _f64, _f64, _i64, _i64, _i64, C.c_void_p, C.c_int],
    "fc_screen_last_kind": [],
    "fc_debug_screen_plan": [_i64, _i64, _i64, _i64, _f64, _f64, _i64, _p_i64],
    "fc_debug_mfma_f16_model": [_i64, _p_i64, _p_f64],
    "fc_debug_h2_covariance": [_ens, _i64, _i64, C.POINTER(C.c_float), _p_f64, _p_f64],
    "fc_debug_kabsch_math": [C.c_int, _p_f64, _i64, _p_f64],
    "fc_comm_unique_id": [_p_u8],
    "fc_comm_init": [_i64, _i64, _p_u8],
    "fc_comm_destroy": [],
    "fc_comm_info": [_p_i64, _p_i64],
    "fc_allgather_mask": [_p_u8, _i64, _p_u8],
    "fc_allgather_u8_dev": [C.c_void_p, C.c_void_p, _i64],
    "fc_comm_barrier": [],
    "fc_debug_comm_loopback": [_i64, _i64],
    "fc_prune_rmsd_sharded": [_ens, _f64, _f64, _i64, _i64, _p_u8, _p_i64],
    "fc_bench_prune_rmsd_sharded": [_ens, _f64, _f64, _i64, C.c_int, _p_f64, _p_f64, _p_u8, _p_i64],
    "fc_ensemble_select_diverse": [_ens, _i64, _i64, _f64, _p_i64, _p_f64, C.POINTER(C.c_int32), _p_f64, _p_i64],
    "fc_bench_select_diverse": [_ens, _i64, _i64, _f64, _i64, _p_f64, _p_f64, _p_i64, _p_i64, _p_i64],
    "fc_ensemble_select_diverse_perm": [_ens, C.POINTER(C.c_int32), _i64, _i64, C.c_int, _i64, _i64, _f64, _p_i64, _p_f64,
                                        C.POINTER(C.c_int32), _p_f64, _p_i64],
    "fc_bench_select_diverse_perm": [_ens, C.POINTER(C.c_int32), _i64, _i64, C.c_int, _i64, _i64, _f64, _i64, _p_f64, _p_f64,
                                     _p_i64, _p_i64, _p_i64],
    "fc_prune_rmsd_many": [C.POINTER(_ens), _i64, _f64, _f64, _i64, C.POINTER(_p_u8), _p_i64],
    "fc_ensemble_knn": [_ens, _i64, C.POINTER(C.c_int32), _p_f64],
    "fc_bench_knn": [_ens, _i64, _i64, _p_f64, _p_f64, _p_i64],
    "fc_ensemble_knn_cross": [_ens, _ens, _i64, C.c_double, C.POINTER(C.c_int32), _p_f64],
    "fc_bench_knn_cross": [_ens, _ens, _i64, C.c_double, _i64, _p_f64, _p_f64, _p_i64],
    "fc_ensemble_knn_perm": [_ens, C.POINTER(C.c_int32), _i64, _i64, C.c_int, _i64, C.POINTER(C.c_int32), _p_f64],
    "fc_ensemble_knn_cross_perm": [_ens, _ens, C.POINTER(C.c_int32), _i64, _i64, C.c_int, _i64, C.c_double,
                                   C.POINTER(C.c_int32), _p_f64],
    "fc_bench_knn_perm": [_ens, C.POINTER(C.c_int32), _i64, _i64, C.c_int, _i64, _i64, _p_f64, _p_f64, _p_i64, _p_i64],
    "fc_bench_knn_cross_perm": [_ens, _ens, C.POINTER(C.c_int32), _i64, _i64, C.c_int, _i64, C.c_double, _i64, _p_f64, _p_f64,
                                _p_i64, _p_i64],
    "fc_ensemble_subset": [_ens, _p_i64, _i64, C.POINTER(_ens)],
    "fc_ensemble_medoids": [_ens, C.POINTER(C.c_int32), _i64, _p_i64, _p_i64, _p_f64, _p_f64, _p_u64, _p_f64, _p_f64],
    "fc_ensemble_kmedoids": [_ens, _p_i64, _i64, _i64, _p_i64, C.POINTER(C.c_int32), _p_f64, _p_u64, _p_i64],
    "fc_ensemble_silhouette": [_ens, C.POINTER(C.c_int32), _i64, _p_f64, _p_f64, _p_f64, C.POINTER(C.c_int32), _p_f64, _p_i64,
                               _p_f64, _p_f64],
    "fc_ensemble_medoids_perm": [_ens, C.POINTER(C.c_int32), _i64, _i64, C.c_int, C.POINTER(C.c_int32), _i64, _p_i64, _p_i64,
                                 _p_f64, _p_f64, _p_u64, _p_f64, _p_f64, _p_i64],
    "fc_ensemble_kmedoids_perm": [_ens, C.POINTER(C.c_int32), _i64, _i64, C.c_int, _p_i64, _i64, _i64, _p_i64,
                                  C.POINTER(C.c_int32), _p_f64, _p_u64, _p_i64],
    "fc_ensemble_silhouette_perm": [_ens, C.POINTER(C.c_int32), _i64, _i64, C.c_int, C.POINTER(C.c_int32), _i64, _p_f64, _p_f64,
                                    _p_f64, C.POINTER(C.c_int32), _p_f64, _p_i64, _p_f64, _p_f64, _p_i64],
    "fc_ensemble_group_means": [_ens, C.POINTER(C.c_int32), _i64, _p_i64, _i64, C.c_double, _p_f64, _p_f64, _p_f64, _p_f64,
                                _p_i64, _p_i64, _p_i64, _p_f64],
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES) + ("fc_last_error",)


def _hip_runtime_mode():
    """Which HIP runtime libfc_hip.so binds to.  Default ``system``: the ROCm install the library was
    built against -- the product does not depend on PyTorch being installed.  ``FC_HIP_RUNTIME=torch``
    (explicit opt-in, for callers that hand the library torch streams / tensors: the legacy
    torch.distributed exchange in ``firecode_amd.dist``) maps the ``libamdhip64.so`` bundled with
    PyTorch's ROCm wheel first, so that both sides share ONE runtime and one device context; two HIP
    runtimes in one process cannot both own the GPU.  Importing torch BEFORE this module has the same
    effect (its copy is then already mapped under the same soname) and is reported as ``torch``."""
    want = os.environ.get("FC_HIP_RUNTIME", "system")
    if want not in ("system", "torch", "auto"):
        raise FirecodeHipInputError(FC_E_INVALID, f"FC_HIP_RUNTIME={want!r}: expected 'system' or 'torch'")
    return "system" if want == "auto" else want


def _mapped_hip_runtimes():
    """paths of every libamdhip64 already mapped into this process"""
    try:
        with open("/proc/self/maps") as fh:
            return sorted({ln.split()[-1] for ln in fh if "libamdhip64" in ln})
    except OSError:
        return []


HIP_RUNTIME = None  # "system" | "torch": set by load()


def _share_torch_hip_runtime():
    """FC_HIP_RUNTIME=torch: map torch's bundled HIP runtime ahead of libfc_hip.so (see
    ``_hip_runtime_mode``).  Refuses when another libamdhip64 is already mapped (a second copy
    would leave one side without a device) or when the bundled file does not carry the soname
    libfc_hip.so asks for."""
    import importlib.util
    import sys

    mapped = _mapped_hip_runtimes()
    if "torch" in sys.modules:
        return mapped[0] if mapped else None  # torch's copy is in: libfc_hip.so binds to it by soname
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        raise FirecodeHipDeviceError(FC_E_NODEVICE, "FC_HIP_RUNTIME=torch but PyTorch is not installed")
    path = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if mapped and os.path.realpath(mapped[0]) != os.path.realpath(path):
        raise FirecodeHipDeviceError(
            FC_E_NODEVICE, f"FC_HIP_RUNTIME=torch but {mapped[0]} is already mapped: a second HIP runtime "
            "in this process would see no GPU")
    if not os.path.exists(path):
        raise FirecodeHipDeviceError(FC_E_NODEVICE, f"FC_HIP_RUNTIME=torch but {path} does not exist")
    with open(path, "rb") as fh:  # the soname libfc_hip.so was linked against must be the one it carries
        if b"libamdhip64.so.7" not in fh.read():
            raise FirecodeHipDeviceError(
                FC_E_NODEVICE, f"{path} does not carry the soname libamdhip64.so.7 that libfc_hip.so binds to")
    C.CDLL(path, mode=C.RTLD_GLOBAL)
    return path


def load():
    """dlopen the library (no device is touched) and set the prototypes."""
    global _lib, HIP_RUNTIME
    if _lib is not None:
        return _lib
    import sys

    mode = _hip_runtime_mode()
    if mode == "torch":
        _share_torch_hip_runtime()
    HIP_RUNTIME = "torch" if (mode == "torch" or "torch" in sys.modules) else "system"
    if not os.path.exists(LIB_PATH):
        raise FirecodeHipDeviceError(
            FC_E_NODEVICE,
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C firecode_amd/csrc`; firecode_amd has no CPU fallback",
        )
    lib = C.CDLL(LIB_PATH)
    for name, argtypes in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = C.c_int
    lib.fc_last_error.argtypes = []
    lib.fc_last_error.restype = C.c_char_p
    _lib = lib
    return lib


def check(rc):
    if rc == FC_OK:
        return
    msg = load().fc_last_error().decode("utf-8", "replace")
    if rc in (FC_E_INVALID, FC_E_LIMIT):
        raise FirecodeHipInputError(rc, msg)
    raise FirecodeHipDeviceError(rc, msg)


def call(name, *args):
    check(getattr(load(), name)(*args))


# ---- array helpers ---------------------------------------------------------------
def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def ptr(a, ctype):
    if a is None:
        return None
    return a.ctypes.data_as(C.POINTER(ctype))


def pf(a):
    return ptr(a, C.c_double)


def pi(a):
    return ptr(a, C.c_int64)


def pb(a):
    return ptr(a, C.c_uint8)


def pw(a):
    return ptr(a, C.c_uint64)


def init(device=0):
    call("fc_init", int(device))


def shutdown():
    call("fc_shutdown")


def stream_set(hip_stream):
    """Enqueue on the caller's HIP stream (integer handle, e.g. ``torch.cuda.Stream().cuda_stream``);
    None / 0 switches back to the library's own stream."""
    call("fc_stream_set", C.c_void_p(int(hip_stream) if hip_stream else None))


def stream_use(hip_stream):
    """``stream_set`` without draining the previous stream (the caller orders streams with events)."""
    call("fc_stream_use", C.c_void_p(int(hip_stream) if hip_stream else None))


def screen_last_kind():
    """32 / 64 / 1: arithmetic of the all-pairs screen the last prune launched (fc_screen_last_kind)."""
    return int(load().fc_screen_last_kind())


def tfd_last_form():
    """(form, n_open) of the last TFD first match (fc_tfd_last_form): form bits 1 = one-phase fp32, 2 = fp32 look-ahead +
    chunks, 4 = 16-bit dense, 8 = 16-bit walk launched, 16 = 16-bit path refused and redone; n_open = rows left open
    after the first phase."""
    n_open = C.c_int64(0)
    return int(load().fc_tfd_last_form(C.byref(n_open))), int(n_open.value)


def screen_select(kind=0):
    """0 = automatic, 32 = single-precision screen, 64 = fp64 screen for the prunes that follow."""
    call("fc_screen_select", int(kind))


# ---- the exchange (RCCL behind the C ABI; firecode_amd/dist.py holds the bootstrap) ------------
def comm_unique_id():
    buf = np.zeros(128, dtype=np.uint8)
    call("fc_comm_unique_id", pb(buf))
    return buf.tobytes()


def comm_init(rank, world, unique_id):
    buf = np.frombuffer(bytes(unique_id), dtype=np.uint8).copy()
    if buf.shape[0] != 128:
        raise FirecodeHipInputError(FC_E_INVALID, "the RCCL unique id has 128 bytes")
    call("fc_comm_init", int(rank), int(world), pb(buf))


def comm_destroy():
    call("fc_comm_destroy")


def comm_info():
    r, w = C.c_int64(0), C.c_int64(1)
    call("fc_comm_info", C.byref(r), C.byref(w))
    return r.value, w.value


def comm_barrier():
    call("fc_comm_barrier")


def allgather_mask(mask_u8):
    """(n,) uint8 on every rank -> (world, n) uint8 (fc_allgather_mask; a group of one without comm_init)."""
    m = u8(mask_u8).reshape(-1)
    _, world = comm_info()
    out = np.zeros((world, m.shape[0]), dtype=np.uint8)
    call("fc_allgather_mask", pb(m), int(m.shape[0]), pb(out))
    return out


def warmup():
    """Load every translation unit's device code and prime the buffer pool now (fc_warmup)."""
    call("fc_warmup")


def memory_trim():
    """Return the device blocks kept by the library's caching pool to the HIP runtime."""
    call("fc_memory_trim")


def device_count():
    return int(load().fc_device_count())


def device_info():
    name = C.create_string_buffer(160)
    ncu, hbm = C.c_int64(0), C.c_int64(0)
    call("fc_device_info", name, 160, C.byref(ncu), C.byref(hbm))
    return {"name": name.value.decode(), "n_cu": ncu.value, "hbm_bytes": hbm.value}


def check_flag(name, value):
    """The boolean keywords of the enantiomer-aware forms (``inverted=``, ``prune_enantiomers=``): a real bool, checked
    before any device use -- ``1``, ``"yes"`` or an array would otherwise pick a kernel by truthiness."""
    if not isinstance(value, (bool, np.bool_)):
        raise FirecodeHipInputError(FC_E_INVALID, f"{name} must be a bool, got {value!r}")
    return bool(value)


def check_min_samples(value):
    """``min_samples`` of the density-based clusters: a real integer >= 1, checked before any device use -- ``True`` or
    ``2.5`` would otherwise be truncated into a different density."""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or int(value) < 1:
        raise FirecodeHipInputError(FC_E_INVALID, f"min_samples must be an integer >= 1, got {value!r}")
    if int(value) >= 2 ** 63:
        raise FirecodeHipInputError(FC_E_INVALID, f"min_samples={value!r} does not fit 64 bits")
    return int(value)


KNN_MAX = 64  # FC_KNN_MAX (include/fc_hip.h)


def check_knn_k(value, limit=True):
    """``k`` of the nearest-neighbour lists: a real integer >= 1, checked before any device use (``2.5`` or ``True``
    would otherwise be truncated into another list length); above FC_KNN_MAX the refusal is FC_E_LIMIT -- made here
    with ``limit``, left to the library (which makes it before any device use too) without."""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or int(value) < 1:
        raise FirecodeHipInputError(FC_E_INVALID, f"k must be an integer >= 1, got {value!r}")
    if int(value) >= 2 ** 63:
        raise FirecodeHipInputError(FC_E_INVALID, f"k={value!r} does not fit 64 bits")
    if limit and int(value) > KNN_MAX:
        raise FirecodeHipInputError(FC_E_LIMIT, f"k={value!r} neighbours: at most FC_KNN_MAX = {KNN_MAX}")
    return int(value)


def check_max_rmsd_cap(value):
    """``max_rmsd`` of the cross-ensemble lists: ``None`` (no cap: +inf) or a positive number, checked before any
    device use -- a NaN, zero or a negative radius is refused, not read as "no cap"."""
    if value is None:
        return float("inf")
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise FirecodeHipInputError(FC_E_INVALID, f"max_rmsd must be a positive number or None, got {value!r}")
    if not float(value) > 0.0:
        raise FirecodeHipInputError(FC_E_INVALID, f"max_rmsd={value!r} must be positive")
    return float(value)


def check_count(name, value, low=1, high=None):
    """An integer argument of the medoid calls (``n``, ``n_groups``, ``max_iter``): a real integer in [low, high], checked
    before any device use -- ``True`` or ``2.5`` would otherwise be truncated into another count."""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or int(value) < low:
        raise FirecodeHipInputError(FC_E_INVALID, f"{name} must be an integer >= {low}, got {value!r}")
    if int(value) >= 2 ** 63 or (high is not None and int(value) > high):
        raise FirecodeHipInputError(FC_E_INVALID, f"{name}={value!r} exceeds {2 ** 63 - 1 if high is None else high}")
    return int(value)


def check_indices(name, value, n_conformers, distinct=False, count=None):
    """Conformer indices (``indices``, ``init``): a 1-D integer array inside [0, N), ``count`` long and without repeats
    where asked, checked before any device use -> a contiguous int64 array"""
    idx = np.asarray(value)
    if idx.ndim != 1 or (idx.size and (idx.dtype == np.bool_ or not np.issubdtype(idx.dtype, np.integer))):
        raise FirecodeHipInputError(FC_E_INVALID, f"{name} must be a 1-D array of integers, got {idx.dtype} {idx.shape}")
    idx = i64(idx)
    if count is not None and idx.shape[0] != count:
        raise FirecodeHipInputError(FC_E_INVALID, f"{name} holds {idx.shape[0]} indices, expected {count}")
    if idx.size and (idx.min() < 0 or idx.max() >= n_conformers):
        raise FirecodeHipInputError(FC_E_INVALID, f"{name} has an entry outside [0, {n_conformers})")
    if distinct and np.unique(idx).shape[0] != idx.shape[0]:
        raise FirecodeHipInputError(FC_E_INVALID, f"{name} names a conformer more than once")
    return idx


def check_group_labels(labels, n_conformers, n_groups=None):
    """``labels`` / ``n_groups`` of the medoids: one integer per conformer (negative: in no group) below ``n_groups``
    (default: the largest label + 1, at least 1), checked before any device use -> (a contiguous int32 array or None,
    n_groups)"""
    if labels is None:
        return None, 1 if n_groups is None else check_count("n_groups", n_groups, high=2 ** 31 - 1)
    lab = np.asarray(labels)
    if lab.ndim != 1 or lab.shape[0] != n_conformers:
        raise FirecodeHipInputError(FC_E_INVALID, f"labels must hold one entry per conformer ({n_conformers}), got {lab.shape}")
    if lab.size and (lab.dtype == np.bool_ or not np.issubdtype(lab.dtype, np.integer)):
        raise FirecodeHipInputError(FC_E_INVALID, f"labels must be integers, got {lab.dtype}")
    top = int(lab.max()) if lab.size else -1
    n_groups = max(top + 1, 1) if n_groups is None else check_count("n_groups", n_groups, high=2 ** 31 - 1)
    if top >= n_groups:
        raise FirecodeHipInputError(FC_E_INVALID, f"labels holds {top}, which is not below n_groups={n_groups}")
    return np.ascontiguousarray(np.maximum(lab.astype(np.int64), -1), dtype=np.int32), n_groups


def check_group_refs(refs, labels, n_groups, n_conformers):
    """``refs`` of the group means: one conformer per group, a member of it (the entry of an empty group is not read),
    against ``labels`` / ``n_groups`` as ``check_group_labels`` returned them, checked before any device use -> a
    contiguous int64 array"""
    idx = np.asarray(refs)
    if idx.ndim != 1 or idx.shape[0] != n_groups or (idx.size and (idx.dtype == np.bool_ or not np.issubdtype(idx.dtype, np.integer))):
        raise FirecodeHipInputError(FC_E_INVALID, f"refs must hold one integer per group ({n_groups}), got {idx.dtype} {idx.shape}")
    idx = i64(idx)
    lab = np.zeros(n_conformers, dtype=np.int32) if labels is None else labels
    sizes = np.bincount(lab[lab >= 0], minlength=n_groups)
    for g in np.flatnonzero(sizes):
        r = int(idx[g])
        if not 0 <= r < n_conformers:
            raise FirecodeHipInputError(FC_E_INVALID, f"refs[{g}]={r} outside [0, {n_conformers})")
        if lab[r] != g:
            raise FirecodeHipInputError(FC_E_INVALID, f"refs[{g}]={r} is not a member of group {g}")
    return idx


def check_tol(name, value):
    """A convergence tolerance: a real number >= 0, checked before any device use -> float"""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise FirecodeHipInputError(FC_E_INVALID, f"{name} must be a real number, got {value!r}")
    if not float(value) >= 0.0:
        raise FirecodeHipInputError(FC_E_INVALID, f"{name}={value!r} is negative or NaN")
    return float(value)


class DeviceEnsemble:
    """HBM-resident prepared ensemble (fc_ensemble)."""

    def __init__(self, coords, atom_mask=None, center=True):
        coords = f64(coords)
        if coords.ndim != 3 or coords.shape[2] != 3:
            raise FirecodeHipInputError(FC_E_INVALID, f"coords must be (N, A, 3), got {coords.shape}")
        self.N, self.A_all = int(coords.shape[0]), int(coords.shape[1])
        m = None if atom_mask is None else u8(np.asarray(atom_mask, dtype=bool))
        if m is not None and m.shape != (self.A_all,):
            raise FirecodeHipInputError(FC_E_INVALID, "atom_mask must have one entry per atom")
        self._atom_mask = None if m is None else m.astype(bool)
        self._h = _ens()
        call("fc_ensemble_create", pf(coords), self.N, self.A_all, pb(m), int(bool(center)), C.byref(self._h))
        self.W = (max(self.N, 1) + 63) // 64

    def close(self):
        if getattr(self, "_h", None):
            load().fc_ensemble_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        if not self._h:
            raise FirecodeHipInputError(FC_E_INVALID, "ensemble already destroyed")
        return self._h

    def _perm_args(self, symmetry, flag_name=None, flag=False):
        """``symmetry=`` (a (K, A_all) table over all atoms; firecode_amd.symmetry) -> the leading arguments of the
        ``_perm`` entry points in selected-atom indices, every check of the contract made before the handle is used"""
        from firecode_amd import symmetry as S

        table = S.resolve(symmetry, None, n_atoms=self.A_all)
        if flag:
            raise FirecodeHipInputError(
                FC_E_INVALID, f"{flag_name}=True cannot be combined with symmetry=: the symmetry-aware forms have no such variant")
        t = S.selected_table(table, self._atom_mask)
        return t, (ptr(t, C.c_int32), int(t.shape[0]), int(t.shape[1]))

    def _form(self, name, perm, enant):
        """the entry point ``name`` in the form the keywords ask for -> (its name, its leading arguments): ``_perm`` with
        the table of ``_perm_args`` behind the handle, else ``_enant``, else plain"""
        if perm is not None:
            return name + "_perm", (self.handle, *perm[1])
        return (name + "_enant" if enant else name), (self.handle,)

    def rmsd_pairs(self, pair_i, pair_j, inverted=False, symmetry=None):
        """(rmsd, maxdev) of the pairs; ``inverted=True``: of (X_i, -X_j), the partner's mirror image
        (fc_ensemble_rmsd_pairs_inv).  ``symmetry=`` a (K, A_all) table: both (P, K), the values of
        (X_i, X_j[perms[k]]) for every k (fc_ensemble_rmsd_pairs_perm); choosing among them is the caller's."""
        inverted = check_flag("inverted", inverted)
        if symmetry is not None:
            keep, args = self._perm_args(symmetry, "inverted", inverted)
            pi_, pj_ = i64(pair_i), i64(pair_j)
            P = int(pi_.shape[0])
            r, m = np.empty((P, args[1])), np.empty((P, args[1]))
            call("fc_ensemble_rmsd_pairs_perm", self.handle, *args, pi(pi_), pi(pj_), P, pf(r), pf(m))
            return r, m
        pi_, pj_ = i64(pair_i), i64(pair_j)
        P = int(pi_.shape[0])
        r, m = np.empty(P), np.empty(P)
        call("fc_ensemble_rmsd_pairs_inv" if inverted else "fc_ensemble_rmsd_pairs", self.handle, pi(pi_), pi(pj_), P,
             pf(r), pf(m))
        return r, m

    def _diverse_perm_args(self, symmetry, prune_enantiomers):
        """``symmetry=`` (a (K, A_all) table) and the mirror flag of the diverse selection -> None when neither is set,
        else the leading arguments of the ``_perm`` entry points; every check made before the handle is used"""
        from firecode_amd import symmetry as S

        enant = check_flag("prune_enantiomers", prune_enantiomers)
        if symmetry is None and not enant:
            return None
        # (a twin workspace refuses here; the identity table stands for "mirror images only")
        keep, args = self._perm_args(np.arange(self.A_all, dtype=np.int64)[None] if symmetry is None else symmetry)
        S.diverse_lds_check(args[1], args[2])
        return keep, args + (int(enant),)

    def select_diverse(self, n_max, start=0, stop_rmsd=None, symmetry=None, prune_enantiomers=False):
        """Greedy max-min selection under this ensemble's RMSD (fc_ensemble_select_diverse; the contract is in
        include/fc_hip.h) -> ``(indices (K,) int64 in selection order, labels (N,) int32 = position in ``indices``
        of each conformer's representative, distances (N,) to it, radii (K,) nonincreasing, radii[0] = inf)``.
        ``symmetry=`` a (K, A_all) table of atom permutations and / or ``prune_enantiomers=True``: under the smallest
        RMSD over the permutations and, with the flag, over both handednesses (fc_ensemble_select_diverse_perm) --
        relabelled copies and mirror images of a representative are at distance 0 from it."""
        perm = self._diverse_perm_args(symmetry, prune_enantiomers)
        n_max, start = int(n_max), int(start)
        stop = -1.0 if stop_rmsd is None else float(stop_rmsd)
        if stop_rmsd is not None and not stop >= 0.0:
            raise FirecodeHipInputError(FC_E_INVALID, f"stop_rmsd={stop_rmsd!r} must be >= 0")
        cap = max(1, min(n_max, self.N))
        idx, rad = np.empty(cap, dtype=np.int64), np.empty(cap)
        lab, dist = np.empty(self.N, dtype=np.int32), np.empty(self.N)
        k = C.c_int64(0)
        if perm is not None:
            call("fc_ensemble_select_diverse_perm", self.handle, *perm[1], n_max, start, stop, pi(idx), pf(rad),
                 ptr(lab, C.c_int32), pf(dist), C.byref(k))
        else:
            call("fc_ensemble_select_diverse", self.handle, n_max, start, stop, pi(idx), pf(rad),
                 ptr(lab, C.c_int32), pf(dist), C.byref(k))
        return idx[:k.value], lab, dist, rad[:k.value]

    def bench_select_diverse(self, n_max, start=0, stop_rmsd=None, reps=3, symmetry=None, prune_enantiomers=False):
        """``reps`` selections -> (mean device ms, mean host ms, indices of the last, lanes per conformer used); with
        ``symmetry=`` / ``prune_enantiomers=True`` (fc_bench_select_diverse_perm) the last entry is instead
        ``(k_h_formed, k_h_explicit)``: the (permutation, handedness) combinations whose eigenvalue was formed and
        those that went on to the explicit pass, over one selection."""
        perm = self._diverse_perm_args(symmetry, prune_enantiomers)
        stop = -1.0 if stop_rmsd is None else float(stop_rmsd)
        idx = np.empty(max(1, min(int(n_max), self.N)), dtype=np.int64)
        dev, host, k, lanes = C.c_double(0), C.c_double(0), C.c_int64(0), C.c_int64(0)
        if perm is not None:
            stats = np.zeros(2, dtype=np.int64)
            call("fc_bench_select_diverse_perm", self.handle, *perm[1], int(n_max), int(start), stop, int(reps),
                 C.byref(dev), C.byref(host), pi(idx), C.byref(k), pi(stats))
            return dev.value, host.value, idx[:k.value], (int(stats[0]), int(stats[1]))
        call("fc_bench_select_diverse", self.handle, int(n_max), int(start), stop, int(reps), C.byref(dev),
             C.byref(host), pi(idx), C.byref(k), C.byref(lanes))
        return dev.value, host.value, idx[:k.value], lanes.value

    def _knn_perm_args(self, symmetry, prune_enantiomers):
        """``symmetry=`` (a (K, A_all) table) and the mirror flag of the nearest-neighbour lists -> None when neither is
        set, else the arguments of the ``_perm`` entry points behind the handles; every check made before a handle is used"""
        from firecode_amd import symmetry as S

        enant = check_flag("prune_enantiomers", prune_enantiomers)
        if symmetry is None and not enant:
            return None
        # (a twin workspace refuses here; the identity table stands for "mirror images only")
        keep, args = self._perm_args(np.arange(self.A_all, dtype=np.int64)[None] if symmetry is None else symmetry)
        S.knn_lds_check(args[1], args[2])
        return keep, args + (int(enant),)

    def knn(self, k, symmetry=None, prune_enantiomers=False):
        """The ``k`` nearest neighbours of every conformer under this ensemble's RMSD (fc_ensemble_knn; the contract is
        in include/fc_hip.h) -> ``(indices (N, k) int32, distances (N, k) float64)``, each row in ascending order of
        (distance, index), the conformer itself left out; rows longer than N - 1 end in -1 / +inf.  No N x N matrix.
        ``symmetry=`` a (K, A_all) table of atom permutations and / or ``prune_enantiomers=True``: under the smallest
        RMSD over the permutations and, with the flag, over both handednesses (fc_ensemble_knn_perm) -- a relabelled
        copy or a mirror image of a conformer is its first neighbour, at distance 0."""
        perm = self._knn_perm_args(symmetry, prune_enantiomers)
        k = check_knn_k(k, limit=False)
        shape = (self.N, k) if k <= KNN_MAX else (1, 1)  # (beyond the limit the library refuses before it writes)
        idx, dist = np.empty(shape, dtype=np.int32), np.empty(shape)
        if perm is not None:
            call("fc_ensemble_knn_perm", self.handle, *perm[1], k, ptr(idx, C.c_int32), pf(dist))
        else:
            call("fc_ensemble_knn", self.handle, k, ptr(idx, C.c_int32), pf(dist))
        return idx, dist

    def bench_knn(self, k, reps=3, symmetry=None, prune_enantiomers=False):
        """``reps`` calls of ``knn(k)`` -> (mean device ms, mean host ms, column strips of the launch); with
        ``symmetry=`` / ``prune_enantiomers=True`` (fc_bench_knn_perm) a fourth entry ``(formed, explicit)``: the
        (pair, permutation, handedness) combinations whose eigenvalue was formed and those taken through the explicit
        pass, over one call."""
        perm = self._knn_perm_args(symmetry, prune_enantiomers)
        dev, host, strips = C.c_double(0), C.c_double(0), C.c_int64(0)
        if perm is not None:
            stats = np.zeros(2, dtype=np.int64)
            call("fc_bench_knn_perm", self.handle, *perm[1], check_knn_k(k, limit=False), int(reps), C.byref(dev), C.byref(host),
                 C.byref(strips), pi(stats))
            return dev.value, host.value, strips.value, (int(stats[0]), int(stats[1]))
        call("fc_bench_knn", self.handle, check_knn_k(k, limit=False), int(reps), C.byref(dev), C.byref(host), C.byref(strips))
        return dev.value, host.value, strips.value

    def _other(self, other):
        """the reference ensemble of a cross-ensemble call: a live DeviceEnsemble with this one's atom selection"""
        if not isinstance(other, DeviceEnsemble):
            raise FirecodeHipInputError(FC_E_INVALID, f"the reference ensemble must be a DeviceEnsemble, got {type(other).__name__}")
        mine = np.ones(self.A_all, dtype=bool) if self._atom_mask is None else self._atom_mask
        theirs = np.ones(other.A_all, dtype=bool) if other._atom_mask is None else other._atom_mask
        if mine.shape != theirs.shape or not np.array_equal(mine, theirs):
            raise FirecodeHipInputError(FC_E_INVALID, "the two ensembles do not have the same atom selection")
        return other.handle

    def knn_against(self, other, k, max_rmsd=None, symmetry=None, prune_enantiomers=False):
        """For every conformer of this ensemble its ``k`` nearest conformers of ``other`` under the RMSD
        (fc_ensemble_knn_cross; the contract is in include/fc_hip.h) -> ``(indices (N, k) int32 into ``other``,
        distances (N, k) float64)``, each row in ascending order of (distance, index), nothing left out (``other`` may
        be this ensemble: a row then lists itself first).  ``max_rmsd``: only references with ``d < max_rmsd`` are
        listed; rows with fewer than ``k`` of them end in -1 / +inf.  Both ensembles: centred, the same atom selection.
        ``symmetry=`` / ``prune_enantiomers=True``: as in ``knn`` (fc_ensemble_knn_cross_perm); the one table serves
        both ensembles."""
        perm = self._knn_perm_args(symmetry, prune_enantiomers)
        k = check_knn_k(k, limit=False)
        cap = check_max_rmsd_cap(max_rmsd)
        ref = self._other(other)
        shape = (self.N, k) if k <= KNN_MAX else (1, 1)  # (beyond the limit the library refuses before it writes)
        idx, dist = np.empty(shape, dtype=np.int32), np.empty(shape)
        if perm is not None:
            call("fc_ensemble_knn_cross_perm", self.handle, ref, *perm[1], k, cap, ptr(idx, C.c_int32), pf(dist))
        else:
            call("fc_ensemble_knn_cross", self.handle, ref, k, cap, ptr(idx, C.c_int32), pf(dist))
        return idx, dist

    def bench_knn_against(self, other, k, max_rmsd=None, reps=3, symmetry=None, prune_enantiomers=False):
        """``reps`` calls of ``knn_against(other, k, max_rmsd)`` -> (mean device ms, mean host ms, column strips); with
        ``symmetry=`` / ``prune_enantiomers=True`` (fc_bench_knn_cross_perm) a fourth entry ``(formed, explicit)`` as
        ``bench_knn``"""
        perm = self._knn_perm_args(symmetry, prune_enantiomers)
        dev, host, strips = C.c_double(0), C.c_double(0), C.c_int64(0)
        if perm is not None:
            stats = np.zeros(2, dtype=np.int64)
            call("fc_bench_knn_cross_perm", self.handle, self._other(other), *perm[1], check_knn_k(k, limit=False),
                 check_max_rmsd_cap(max_rmsd), int(reps), C.byref(dev), C.byref(host), C.byref(strips), pi(stats))
            return dev.value, host.value, strips.value, (int(stats[0]), int(stats[1]))
        call("fc_bench_knn_cross", self.handle, self._other(other), check_knn_k(k, limit=False), check_max_rmsd_cap(max_rmsd),
             int(reps), C.byref(dev), C.byref(host), C.byref(strips))
        return dev.value, host.value, strips.value

    def subset(self, indices):
        """The conformers ``indices`` (in that order, repeats allowed) as a new ``DeviceEnsemble`` with this one's atom
        selection (fc_ensemble_subset): the prepared coordinates are copied on the device, not prepared again, so every
        distance within the subset has the bits it has here."""
        idx = check_indices("indices", indices, self.N)
        sub = DeviceEnsemble.__new__(DeviceEnsemble)
        sub.N, sub.A_all, sub._atom_mask = int(idx.shape[0]), self.A_all, getattr(self, "_atom_mask", None)
        sub.W = (max(sub.N, 1) + 63) // 64
        sub._h = _ens()
        call("fc_ensemble_subset", self.handle, pi(idx), sub.N, C.byref(sub._h))
        return sub

    def medoids(self, labels=None, n_groups=None, want_ms=False):
        """The medoid of every group of conformers under this ensemble's RMSD (fc_ensemble_medoids; the contract is in
        include/fc_hip.h): ``labels`` (N,) integers, negative = in no group (``None``: one group of all conformers),
        ``n_groups`` (default: the largest label + 1) -> ``(medoids (n_groups,) int64, sizes (n_groups,) int64,
        mean_distance (n_groups,), radius (n_groups,), sums_q32 (N,) uint64 in units of 2^-32 A, eccentricity (N,))``;
        an empty group has medoid -1 and NaN mean and radius.  ``want_ms=True`` appends the kernel's milliseconds."""
        lab, n_groups = check_group_labels(labels, self.N, n_groups)
        med, sizes = np.empty(n_groups, dtype=np.int64), np.empty(n_groups, dtype=np.int64)
        mean, radius = np.empty(n_groups), np.empty(n_groups)
        sums, ecc = np.zeros(self.N, dtype=np.uint64), np.zeros(self.N)
        ms = C.c_double(0)
        call("fc_ensemble_medoids", self.handle, ptr(lab, C.c_int32), n_groups, pi(med), pi(sizes), pf(mean), pf(radius),
             pw(sums), pf(ecc), C.byref(ms))
        out = (med, sizes, mean, radius, sums, ecc)
        return out + (ms.value,) if want_ms else out

    def kmedoids(self, n, init=None, max_iter=50):
        """``n`` representatives that minimise the summed RMSD of every conformer to its representative, by alternating
        "assign to the nearest" and "move to the group's medoid" (fc_ensemble_kmedoids; the contract is in
        include/fc_hip.h).  ``init``: ``n`` distinct conformers to start from (default: the picks of
        ``select_diverse(n, start=0)``) -> ``(medoids (n,) int64, labels (N,) int32 = position in ``medoids``,
        distances (N,), cost_q32 (int, units of 2^-32 A), n_iter)``."""
        n = check_count("n", n)
        max_iter = check_count("max_iter", max_iter, low=0)
        if self.N and n > self.N:
            raise FirecodeHipInputError(FC_E_INVALID, f"n={n} representatives of N={self.N} conformers")
        start = None if init is None else check_indices("init", init, self.N, distinct=True, count=n)
        med = np.empty(n, dtype=np.int64)
        lab, dist = np.empty(self.N, dtype=np.int32), np.empty(self.N)
        cost, n_iter = C.c_uint64(0), C.c_int64(0)
        call("fc_ensemble_kmedoids", self.handle, pi(start), n, max_iter, pi(med), ptr(lab, C.c_int32), pf(dist),
             C.byref(cost), C.byref(n_iter))
        return (med if self.N else med[:0]), lab, dist, int(cost.value), int(n_iter.value)

    def silhouette(self, labels=None, n_groups=None, want_ms=False):
        """The silhouette of every labelled conformer under this ensemble's RMSD (fc_ensemble_silhouette; the contract is
        in include/fc_hip.h): ``labels`` and ``n_groups`` as for ``medoids`` -> ``(s (N,), a (N,) = the mean distance to
        the other members of the conformer's own group, b (N,) = the smallest mean distance to another group, nearest
        (N,) int32 = that group, cluster_mean (n_groups,), sizes (n_groups,) int64, score)``.  A conformer in no group
        has NaN ``s``, ``a``, ``b`` and ``nearest`` -1; with fewer than two non-empty groups ``b``, ``s`` and ``score``
        are NaN.  ``want_ms=True`` appends the kernels' milliseconds."""
        lab, n_groups = check_group_labels(labels, self.N, n_groups)
        s, a, b = np.empty(self.N), np.empty(self.N), np.empty(self.N)
        nearest = np.empty(self.N, dtype=np.int32)
        mean, sizes = np.empty(n_groups), np.empty(n_groups, dtype=np.int64)
        score, ms = C.c_double(0), C.c_double(0)
        call("fc_ensemble_silhouette", self.handle, ptr(lab, C.c_int32), n_groups, pf(s), pf(a), pf(b), ptr(nearest, C.c_int32),
             pf(mean), pi(sizes), C.byref(score), C.byref(ms))
        out = (s, a, b, nearest, mean, sizes, score.value)
        return out + (ms.value,) if want_ms else out

    def group_means(self, labels=None, n_groups=None, refs=None, max_iter=50, tol=1e-9, want_rotations=True, want_ms=False):
        """The mean structure of every group of conformers, its members superposed on it (generalized Procrustes per
        group), the per-atom fluctuation about it and every member's RMSD to it (fc_ensemble_group_means; the contract,
        the order of its sums included, is in include/fc_hip.h).  ``labels`` / ``n_groups`` as for ``medoids``;
        ``refs`` (n_groups,): the member each group starts from (``None``: its lowest-index member, ``"medoids"``: the
        medoids of ``medoids(labels, n_groups)`` on this same ensemble); at most ``max_iter`` turns, a group stops once
        its mean moved by no more than ``tol`` (RMS over the selected atoms) -> ``(means (n_groups, A_sel, 3), rmsf
        (n_groups, A_sel), distances (N,), closest (n_groups,) int64, sizes (n_groups,) int64, n_iter (n_groups,) int64,
        rotations (N, 3, 3) or None)``.  An empty group has NaN mean and rmsf and closest -1; a conformer in no group NaN
        distance and the identity.  ``want_ms=True`` appends the kernels' milliseconds."""
        lab, n_groups = check_group_labels(labels, self.N, n_groups)
        max_iter = check_count("max_iter", max_iter, low=0)
        tol = check_tol("tol", tol)
        if isinstance(refs, str):
            if refs != "medoids":
                raise FirecodeHipInputError(FC_E_INVALID, f"refs={refs!r}: an array, None or 'medoids'")
            start = self.medoids(lab, n_groups)[0] if self.N else None
        else:
            start = None if refs is None else check_group_refs(refs, lab, n_groups, self.N)
        mask = getattr(self, "_atom_mask", None)
        a_sel = self.A_all if mask is None else int(np.count_nonzero(mask))
        means, rmsf = np.full((n_groups, a_sel, 3), np.nan), np.full((n_groups, a_sel), np.nan)
        dist = np.full(self.N, np.nan)
        rot = np.tile(np.eye(3), (self.N, 1, 1)) if want_rotations else None
        closest, sizes = np.full(n_groups, -1, dtype=np.int64), np.zeros(n_groups, dtype=np.int64)
        n_iter = np.zeros(n_groups, dtype=np.int64)
        ms = C.c_double(0)
        call("fc_ensemble_group_means", self.handle, ptr(lab, C.c_int32), n_groups, pi(start), max_iter, tol, pf(means),
             pf(rmsf), pf(dist), pf(rot), pi(closest), pi(sizes), pi(n_iter), C.byref(ms))
        out = (means, rmsf, dist, closest, sizes, n_iter, rot)
        return out + (ms.value,) if want_ms else out

    def _sums_perm_args(self, symmetry, prune_enantiomers):
        """``symmetry=`` (a (K, A_all) table) and the mirror flag of ``medoids_sym`` / ``kmedoids_sym`` /
        ``silhouette_sym`` -> None when neither is set, else the arguments of the ``_perm`` entry points behind the
        handle; every check made before the handle is used"""
        from firecode_amd import symmetry as S

        enant = check_flag("prune_enantiomers", prune_enantiomers)
        if symmetry is None and not enant:
            return None
        # (a twin workspace refuses here; the identity table stands for "mirror images only")
        keep, args = self._perm_args(np.arange(self.A_all, dtype=np.int64)[None] if symmetry is None else symmetry)
        S.medoid_lds_check(args[1], args[2])
        return keep, args + (int(enant),)

    def medoids_sym(self, labels=None, n_groups=None, symmetry=None, prune_enantiomers=False, want_ms=False):
        """``medoids`` under the symmetry-corrected distance (fc_ensemble_medoids_perm; the contract is in
        include/fc_hip.h): ``symmetry=`` a (K, A_all) table of atom permutations and / or ``prune_enantiomers=True`` make
        the distance the smallest RMSD over the permutations and, with the flag, over both handednesses -- the distance
        of ``knn(symmetry=, prune_enantiomers=)``, bit for bit.  The outputs of ``medoids``; ``want_ms=True`` appends the
        kernel's milliseconds and ``(formed, explicit)``, the (pair, permutation, handedness) combinations whose
        eigenvalue was formed and those taken through the explicit pass.  With neither keyword: ``medoids`` itself."""
        perm = self._sums_perm_args(symmetry, prune_enantiomers)
        if perm is None:
            out = self.medoids(labels, n_groups, want_ms=want_ms)
            return out + ((0, 0),) if want_ms else out
        lab, n_groups = check_group_labels(labels, self.N, n_groups)
        med, sizes = np.empty(n_groups, dtype=np.int64), np.empty(n_groups, dtype=np.int64)
        mean, radius = np.empty(n_groups), np.empty(n_groups)
        sums, ecc = np.zeros(self.N, dtype=np.uint64), np.zeros(self.N)
        ms, stats = C.c_double(0), np.zeros(2, dtype=np.int64)
        call("fc_ensemble_medoids_perm", self.handle, *perm[1], ptr(lab, C.c_int32), n_groups, pi(med), pi(sizes), pf(mean),
             pf(radius), pw(sums), pf(ecc), C.byref(ms), pi(stats) if want_ms else None)
        out = (med, sizes, mean, radius, sums, ecc)
        return out + (ms.value, (int(stats[0]), int(stats[1]))) if want_ms else out

    def kmedoids_sym(self, n, init=None, max_iter=50, symmetry=None, prune_enantiomers=False):
        """``kmedoids`` under the symmetry-corrected distance of ``medoids_sym`` (fc_ensemble_kmedoids_perm): the default
        start is ``select_diverse(n, start=0, symmetry=, prune_enantiomers=)``, the assignment the nearest
        representative under that distance, the move the medoid of ``medoids_sym``.  The outputs of ``kmedoids``.  With
        neither keyword: ``kmedoids`` itself."""
        perm = self._sums_perm_args(symmetry, prune_enantiomers)
        if perm is None:
            return self.kmedoids(n, init=init, max_iter=max_iter)
        n = check_count("n", n)
        max_iter = check_count("max_iter", max_iter, low=0)
        if self.N and n > self.N:
            raise FirecodeHipInputError(FC_E_INVALID, f"n={n} representatives of N={self.N} conformers")
        start = None if init is None else check_indices("init", init, self.N, distinct=True, count=n)
        med = np.empty(n, dtype=np.int64)
        lab, dist = np.empty(self.N, dtype=np.int32), np.empty(self.N)
        cost, n_iter = C.c_uint64(0), C.c_int64(0)
        call("fc_ensemble_kmedoids_perm", self.handle, *perm[1], pi(start), n, max_iter, pi(med), ptr(lab, C.c_int32), pf(dist),
             C.byref(cost), C.byref(n_iter))
        return (med if self.N else med[:0]), lab, dist, int(cost.value), int(n_iter.value)

    def silhouette_sym(self, labels=None, n_groups=None, symmetry=None, prune_enantiomers=False, want_ms=False):
        """``silhouette`` under the symmetry-corrected distance of ``medoids_sym`` (fc_ensemble_silhouette_perm).  The
        outputs of ``silhouette``; ``want_ms=True`` appends the kernels' milliseconds and ``(formed, explicit)`` as
        ``medoids_sym``.  With neither keyword: ``silhouette`` itself."""
        perm = self._sums_perm_args(symmetry, prune_enantiomers)
        if perm is None:
            out = self.silhouette(labels, n_groups, want_ms=want_ms)
            return out + ((0, 0),) if want_ms else out
        lab, n_groups = check_group_labels(labels, self.N, n_groups)
        s, a, b = np.empty(self.N), np.empty(self.N), np.empty(self.N)
        nearest = np.empty(self.N, dtype=np.int32)
        mean, sizes = np.empty(n_groups), np.empty(n_groups, dtype=np.int64)
        score, ms, stats = C.c_double(0), C.c_double(0), np.zeros(2, dtype=np.int64)
        call("fc_ensemble_silhouette_perm", self.handle, *perm[1], ptr(lab, C.c_int32), n_groups, pf(s), pf(a), pf(b),
             ptr(nearest, C.c_int32), pf(mean), pi(sizes), C.byref(score), C.byref(ms), pi(stats) if want_ms else None)
        out = (s, a, b, nearest, mean, sizes, score.value)
        return out + (ms.value, (int(stats[0]), int(stats[1]))) if want_ms else out

    def rmsd_matrix(self):
        r = np.zeros((self.N, self.N))
        m = np.zeros((self.N, self.N))
        call("fc_ensemble_rmsd_matrix", self.handle, pf(r), pf(m))
        return r, m

    def rmsd_values(self, want_matrix=True):
        """All-pairs RMSD values (no max deviation) on the matrix pipe:
        (matrix (N, N) or None, kernel ms)."""
        r = np.zeros((self.N, self.N)) if want_matrix else None
        ms = C.c_double(0)
        call("fc_ensemble_rmsd_values", self.handle, pf(r), C.byref(ms))
        return r, ms.value

    def rmsd_and_max_all(self, want_matrices=True):
        """Complete alignment of all pairs: ((rmsd, maxdev) matrices or (None, None), kernel ms)."""
        r = np.zeros((self.N, self.N)) if want_matrices else None
        m = np.zeros((self.N, self.N)) if want_matrices else None
        ms = C.c_double(0)
        call("fc_ensemble_rmsd_and_max_all", self.handle, pf(r), pf(m), C.byref(ms))
        return r, m, ms.value

    def bench_refine(self, max_rmsd, max_dev, reps=10):
        """The exact refine alone over the candidate queue one screen leaves -> (mean kernel ms, candidates)."""
        ms, n = C.c_double(0), C.c_int64(0)
        call("fc_bench_refine", self.handle, float(max_rmsd), float(max_dev), int(reps), C.byref(ms), C.byref(n))
        return ms.value, n.value

    def bench_rmsd_and_max_all(self, reps=1):
        """``reps`` complete all-pairs alignment passes, outputs resident ->
        (mean kernel ms, total ms, stats [pairs, fix-up pairs, tiled, general-form sub-tiles of the last pass])."""
        k, t = C.c_double(0), C.c_double(0)
        stats = np.zeros(4, dtype=np.int64)
        call("fc_bench_rmsd_and_max_all", self.handle, int(reps), C.byref(k), C.byref(t), pi(stats))
        return k.value, t.value, stats

    def bench_rmsd_and_max_all_sampled(self, pair_i, pair_j, reps=1):
        """``bench_rmsd_and_max_all`` + the elements (pair_i, pair_j) of the last pass's two output matrices
        -> (mean kernel ms, total ms, stats, rmsd (P,), maxdev (P,))."""
        pi_, pj_ = i64(pair_i), i64(pair_j)
        P = int(pi_.shape[0])
        r, m = np.empty(P), np.empty(P)
        k, t = C.c_double(0), C.c_double(0)
        stats = np.zeros(4, dtype=np.int64)
        call("fc_bench_rmsd_and_max_all_sampled", self.handle, int(reps), pi(pi_), pi(pj_), P, pf(r), pf(m),
             C.byref(k), C.byref(t), pi(stats))
        return k.value, t.value, stats, r, m

    def simbits(self, max_rmsd, max_dev, energies=None, max_dE=0.0, row_begin=0, row_end=None, prune_enantiomers=False,
                symmetry=None):
        """Similarity bits (fc_rmsd_simbits); ``prune_enantiomers=True``: a pair is also similar when it is so with one
        partner inverted (fc_rmsd_simbits_enant; the contract is in include/fc_hip.h).  ``symmetry=`` a (K, A_all)
        table of atom permutations: similar under any of them (fc_rmsd_simbits_perm)."""
        enant = check_flag("prune_enantiomers", prune_enantiomers)
        perm = None if symmetry is None else self._perm_args(symmetry, "prune_enantiomers", enant)
        row_end = self.N if row_end is None else int(row_end)
        bits = np.zeros((row_end - row_begin, self.W), dtype=np.uint64)
        grey = C.c_int64(0)
        en = None if energies is None else f64(energies)
        name, head = self._form("fc_rmsd_simbits", perm, enant)
        call(name, *head, float(max_rmsd), float(max_dev), pf(en), float(max_dE), int(row_begin), row_end, pw(bits),
             C.byref(grey))
        return bits, grey.value

    def prune(self, max_rmsd, max_dev, energies=None, max_dE=0.0, min_per_group=20, prune_enantiomers=False, symmetry=None):
        """The whole stage (fc_prune_rmsd) -> (mask, stats); ``prune_enantiomers=True``: mirror images count as
        duplicates (fc_prune_rmsd_enant).  ``symmetry=`` a (K, A_all) table of atom permutations: relabelled copies
        count as duplicates (fc_prune_rmsd_perm)."""
        enant = check_flag("prune_enantiomers", prune_enantiomers)
        perm = None if symmetry is None else self._perm_args(symmetry, "prune_enantiomers", enant)
        mask = np.zeros(self.N, dtype=np.uint8)
        stats = np.zeros(6, dtype=np.int64)
        en = None if energies is None else f64(energies)
        name, head = self._form("fc_prune_rmsd", perm, enant)
        call(name, *head, float(max_rmsd), float(max_dev), pf(en), float(max_dE), int(min_per_group), pb(mask), pi(stats))
        return mask.astype(bool), stats

    def clusters(self, max_rmsd, max_dev, energies=None, max_dE=0.0, prune_enantiomers=False, symmetry=None):
        """Connected components of the prune's similarity graph (fc_rmsd_clusters; ``prune_enantiomers=True``:
        fc_rmsd_clusters_enant; the contract is in include/fc_hip.h) -> ``(labels (N,) int32, reps (K,) int64, sizes (K,)
        int64, stats)`` in processing order: clusters numbered by ascending smallest member, which is their
        representative.  stats: pairs, refined, edges, grey, 1 if the bit-matrix path ran, K.  ``symmetry=`` a
        (K, A_all) table of atom permutations: the components of that graph (fc_rmsd_clusters_perm)."""
        enant = check_flag("prune_enantiomers", prune_enantiomers)
        perm = None if symmetry is None else self._perm_args(symmetry, "prune_enantiomers", enant)
        labels = np.zeros(self.N, dtype=np.int32)
        reps, sizes = np.zeros(self.N, dtype=np.int64), np.zeros(self.N, dtype=np.int64)
        stats = np.zeros(6, dtype=np.int64)
        k = C.c_int64(0)
        en = None if energies is None else f64(energies)
        name, head = self._form("fc_rmsd_clusters", perm, enant)
        call(name, *head, float(max_rmsd), float(max_dev), pf(en), float(max_dE), ptr(labels, C.c_int32), pi(reps), pi(sizes),
             C.byref(k), pi(stats))
        return labels, reps[:k.value].copy(), sizes[:k.value].copy(), stats

    def dbscan(self, max_rmsd, max_dev, min_samples, energies=None, max_dE=0.0, prune_enantiomers=False, symmetry=None):
        """Density-based clusters of the prune's similarity graph (fc_rmsd_dbscan; ``prune_enantiomers=True``:
        fc_rmsd_dbscan_enant; ``symmetry=`` a (K, A_all) table: fc_rmsd_dbscan_perm; the contract is in include/fc_hip.h)
        -> ``(labels (N,) int32 with -1 for noise, reps (K,) int64, sizes (K,) int64, core (N,) bool, degrees (N,) int32,
        stats)`` in processing order.  A conformer is core when it has at least ``min_samples - 1`` neighbours; clusters
        are the components of the core points, numbered by ascending smallest core member, their representative; a
        point that is not core joins the cluster of its smallest-index core neighbour, or is noise.  stats: as
        ``clusters``, then the numbers of core and of noise points."""
        enant = check_flag("prune_enantiomers", prune_enantiomers)
        m = check_min_samples(min_samples)
        perm = None if symmetry is None else self._perm_args(symmetry, "prune_enantiomers", enant)
        labels, degrees = np.zeros(self.N, dtype=np.int32), np.zeros(self.N, dtype=np.int32)
        reps, sizes = np.zeros(self.N, dtype=np.int64), np.zeros(self.N, dtype=np.int64)
        core = np.zeros(self.N, dtype=np.uint8)
        stats = np.zeros(8, dtype=np.int64)
        k = C.c_int64(0)
        en = None if energies is None else f64(energies)
        outs = (ptr(labels, C.c_int32), pi(reps), pi(sizes), pb(core), ptr(degrees, C.c_int32), C.byref(k), pi(stats))
        name, head = self._form("fc_rmsd_dbscan", perm, enant)
        call(name, *head, float(max_rmsd), float(max_dev), m, pf(en), float(max_dE), *outs)
        return labels, reps[:k.value].copy(), sizes[:k.value].copy(), core.astype(bool), degrees, stats

    def butina(self, max_rmsd, max_dev, energies=None, max_dE=0.0, prune_enantiomers=False, symmetry=None):
        """Sphere-exclusion (Butina) clusters of the prune's similarity graph (fc_rmsd_butina; ``prune_enantiomers=True``:
        fc_rmsd_butina_enant; ``symmetry=`` a (K, A_all) table: fc_rmsd_butina_perm; the contract is in include/fc_hip.h)
        -> ``(labels (N,) int32, centroids (K,) int64, sizes (K,) int64, degrees (N,) int32, stats)`` in processing order.
        Conformers are ranked by degree (more neighbours first, the smaller index on ties); the first unassigned one
        becomes a centroid and takes its unassigned neighbours; clusters are numbered by ascending centroid.  stats: as
        ``clusters``, then the rounds the device needed and the conformers its grid-wide rounds left to the finish."""
        enant = check_flag("prune_enantiomers", prune_enantiomers)
        perm = None if symmetry is None else self._perm_args(symmetry, "prune_enantiomers", enant)
        labels, degrees = np.zeros(self.N, dtype=np.int32), np.zeros(self.N, dtype=np.int32)
        reps, sizes = np.zeros(self.N, dtype=np.int64), np.zeros(self.N, dtype=np.int64)
        stats = np.zeros(8, dtype=np.int64)
        k = C.c_int64(0)
        en = None if energies is None else f64(energies)
        outs = (ptr(labels, C.c_int32), pi(reps), pi(sizes), ptr(degrees, C.c_int32), C.byref(k), pi(stats))
        name, head = self._form("fc_rmsd_butina", perm, enant)
        call(name, *head, float(max_rmsd), float(max_dev), pf(en), float(max_dE), *outs)
        return labels, reps[:k.value].copy(), sizes[:k.value].copy(), degrees, stats

    def prune_begin(self, max_rmsd, max_dev, rank, world, row_block=128, energies=None, max_dE=0.0):
        stats = np.zeros(6, dtype=np.int64)
        en = None if energies is None else f64(energies)
        call("fc_prune_rmsd_begin", self.handle, float(max_rmsd), float(max_dev), pf(en), float(max_dE),
             int(rank), int(world), int(row_block), pi(stats))
        return stats

    def prune_level(self, k, mask_in):
        mi = u8(mask_in)
        mo = np.zeros(self.N, dtype=np.uint8)
        call("fc_prune_level", self.handle, int(k), pb(mi), pb(mo))
        return mo

    def similar_pairs(self, count_hint=None):
        """This rank's exactly-similar pairs after ``prune_begin`` as uint64
        ``(i << 32) | j``; raises FirecodeHipInputError (FC_E_LIMIT) when the
        candidate queue overflowed (dense similarity: use ``prune_level``).
        ``count_hint``: ``stats[2]`` of ``prune_begin`` saves the size query."""
        n = C.c_int64(0)
        if count_hint is None:
            call("fc_prune_similar_pairs", self.handle, None, 0, C.byref(n))
            count_hint = n.value
        out = np.zeros(int(count_hint), dtype=np.uint64)
        call("fc_prune_similar_pairs", self.handle, pw(out), out.shape[0], C.byref(n))
        return out[: n.value]

    def prune_from_pairs(self, pairs, min_per_group=20):
        pairs = np.ascontiguousarray(pairs, dtype=np.uint64)
        mask = np.zeros(self.N, dtype=np.uint8)
        call("fc_prune_from_pairs", self.handle, pw(pairs), int(pairs.shape[0]), int(min_per_group), pb(mask))
        return mask.astype(bool)

    # device-resident exchange: device pointers are plain integers (e.g. torch's data_ptr())
    def prune_begin_async(self, max_rmsd, max_dev, rank, world, row_block=128):
        call("fc_prune_rmsd_begin_async", self.handle, float(max_rmsd), float(max_dev), int(rank), int(world),
             int(row_block))

    def prune_begin_split_async(self, max_rmsd, max_dev, rank, world, screen_stream, row_block=128, timed=True):
        call("fc_prune_rmsd_begin_split_async", self.handle, float(max_rmsd), float(max_dev), int(rank),
             int(world), int(row_block), C.c_void_p(int(screen_stream)), int(bool(timed)))

    def twin(self):
        """Second prune workspace over the same resident coordinates (owned by this ensemble)."""
        t = getattr(self, "_twin", None)
        if t is None:
            h = _ens()
            call("fc_ensemble_twin", self.handle, C.byref(h))
            t = self._twin = _EnsembleView(self, h)
        return t

    def export_pairs_dev(self, dev_ptr, cap):
        call("fc_prune_export_pairs_dev", self.handle, C.c_void_p(int(dev_ptr)), int(cap))

    def prune_from_gathered_dev(self, dev_ptr, world, cap, min_per_group=20):
        mask = np.zeros(self.N, dtype=np.uint8)
        stats = np.zeros(6, dtype=np.int64)
        call("fc_prune_from_gathered_dev", self.handle, C.c_void_p(int(dev_ptr)), int(world), int(cap),
             int(min_per_group), pb(mask), pi(stats))
        return mask.astype(bool), stats

    def prune_from_gathered_enqueue(self, dev_ptr, world, cap, slot, n_slots, min_per_group=20):
        call("fc_prune_from_gathered_dev_enqueue", self.handle, C.c_void_p(int(dev_ptr)), int(world), int(cap),
             int(min_per_group), int(slot), int(n_slots))

    def prune_collect(self, slot, n_slots):
        mask = np.zeros(self.N, dtype=np.uint8)
        stats = np.zeros(6, dtype=np.int64)
        call("fc_prune_collect", self.handle, int(slot), int(n_slots), pb(mask), pi(stats))
        return mask.astype(bool), stats

    def prune_sharded(self, max_rmsd, max_dev, min_per_group=20, row_block=0):
        """fc_prune_rmsd_sharded: this rank's part of the prune over the communicator of
        ``firecode_amd.dist.comm_init`` (a group of one without it) -> (mask, stats)."""
        mask = np.zeros(self.N, dtype=np.uint8)
        stats = np.zeros(6, dtype=np.int64)
        call("fc_prune_rmsd_sharded", self.handle, float(max_rmsd), float(max_dev), int(min_per_group),
             int(row_block), pb(mask), pi(stats))
        return mask.astype(bool), stats

    def bench_prune_sharded(self, max_rmsd, max_dev, reps=1, overlap=True):
        """``reps`` stream-ordered sharded prunes -> (screen kernel ms, step ms, mask, stats (8))."""
        mask = np.zeros(self.N, dtype=np.uint8)
        stats = np.zeros(8, dtype=np.int64)
        t_k, t_s = C.c_double(0), C.c_double(0)
        call("fc_bench_prune_rmsd_sharded", self.handle, float(max_rmsd), float(max_dev), int(reps),
             int(bool(overlap)), C.byref(t_k), C.byref(t_s), pb(mask), pi(stats))
        return t_k.value, t_s.value, mask.astype(bool), stats

    def bench_prune(self, max_rmsd, max_dev, reps=1, want_mask=True):
        mask = np.zeros(self.N, dtype=np.uint8) if want_mask else None
        stats = np.zeros(8, dtype=np.int64)  # [6], [7]: the subset stage of the lean fp32 screen
        t_k, t_s = C.c_double(0), C.c_double(0)
        call("fc_bench_prune_rmsd", self.handle, float(max_rmsd), float(max_dev), int(reps),
             C.byref(t_k), C.byref(t_s), pb(mask), pi(stats))
        return t_k.value, t_s.value, (None if mask is None else mask.astype(bool)), stats


class _EnsembleView(DeviceEnsemble):
    """A handle owned by another ensemble (its twin workspace): never destroyed from here."""

    def __init__(self, parent, handle):
        self._parent = parent
        self._view_h = handle
        self.N, self.A_all, self.W = parent.N, parent.A_all, parent.W

    @property
    def handle(self):
        self._parent.handle  # raises when the owner is gone
        return self._view_h

    def _perm_args(self, symmetry, flag_name=None, flag=False):
        raise FirecodeHipInputError(FC_E_INVALID, "symmetry= is not offered on a twin workspace: use the owning ensemble")

    def close(self):
        pass

    def twin(self):
        return self._parent


def prune_many(ensembles, max_rmsd, max_dev, min_per_group=20):
    """fc_prune_rmsd_many over DeviceEnsemble objects: list of bool masks, survivor counts."""
    n = len(ensembles)
    handles = (_ens * max(n, 1))(*[e.handle for e in ensembles])
    masks = [np.zeros(max(int(e.N), 1), dtype=np.uint8) for e in ensembles]
    ptrs = (_p_u8 * max(n, 1))(*[m.ctypes.data_as(_p_u8) for m in masks])
    survivors = np.zeros(max(n, 1), dtype=np.int64)
    call("fc_prune_rmsd_many", handles, n, float(max_rmsd), float(max_dev), int(min_per_group), ptrs,
         survivors.ctypes.data_as(_p_i64))
    return [m[: int(e.N)].astype(bool) for m, e in zip(masks, ensembles)], survivors[:n]


def unpack_bits(bits, n):
    """(rows, W) uint64 words -> (rows, n) bool."""
    b = np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")
    return b[:, :n].astype(bool)


# ---- .xyz wire format (host code of the library) --------------------------------------
def xyz_write(path, atoms, coords, label="", mode=0):
    """mode 0: Ensemble.to_xyz text (label = basename); mode 1: utils.write_xyz text per conformer."""
    X = f64(coords)
    if X.ndim == 2:
        X = X[None]
    syms = [str(a).encode() for a in atoms]
    arr = (C.c_char_p * len(syms))(*syms)
    call("fc_xyz_write", os.fsencode(str(path)), arr, len(syms), pf(X), X.shape[0], str(label).encode(), int(mode))


def xyz_read(path):
    """-> (atoms (A,) str array of the first conformer, coords (N, A, 3))"""
    n, a = C.c_int64(0), C.c_int64(0)
    p = os.fsencode(str(path))
    call("fc_xyz_scan", p, C.byref(n), C.byref(a))
    coords = np.empty((n.value, a.value, 3))
    buf = C.create_string_buffer(max(a.value, 1) * 8)
    if n.value:
        call("fc_xyz_read", p, n.value, a.value, buf, pf(coords))
    atoms = np.array([buf.raw[i * 8:(i + 1) * 8].split(b"\0", 1)[0].decode() for i in range(a.value)])
    return atoms, coords


class _PinnedBlock:
    """A block of page-locked host memory (fc_host_alloc_pinned) exposed through the array interface; freed with the last
    array that views it."""

    def __init__(self, nbytes):
        ptr = C.c_void_p()
        call("fc_host_alloc_pinned", int(nbytes), C.byref(ptr))
        self._ptr = ptr.value
        self.__array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (self._ptr, False), "version": 3}

    def __del__(self):
        p, self._ptr = getattr(self, "_ptr", None), None
        if p:
            try:
                load().fc_host_free_pinned(C.c_void_p(p))
            except Exception:  # interpreter shutdown
                pass


def pinned_empty(shape, dtype=np.float64):
    """``np.empty(shape, dtype)`` in page-locked host memory: an ensemble built into such an array is uploaded by direct DMA
    (``prune_by_rmsd`` and every other entry point take it like any other array; host arrays in -> mask out 0.78 -> 0.6 ms
    at 10 000 x 50).  The memory is released with the last array that views it."""
    dtype = np.dtype(dtype)
    shape = (int(shape),) if np.isscalar(shape) else tuple(int(v) for v in shape)
    n = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
    if n == 0:
        return np.empty(shape, dtype)
    return np.asarray(_PinnedBlock(n)).view(dtype).reshape(shape)
