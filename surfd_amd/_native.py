"""ctypes binding of libsurfd_hip.so (include/surfd_hip.h).

The product path has no CPU fallback: if the library is missing or a call fails this module
raises — it never routes around the HIP kernels.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
# SURFD_LIB: a differently built copy of the same library (A/B timing of kernel variants, tools/build_variants.py)
LIB_PATH = os.environ.get("SURFD_LIB") or os.path.join(_HERE, "lib", "libsurfd_hip.so")
GRID_MAX_LEVELS = 8

c_i64p = C.POINTER(C.c_int64)
c_f32p = C.POINTER(C.c_float)


class UNetCfg(C.Structure):
    _fields_ = [("in_channels", C.c_int), ("model_channels", C.c_int), ("out_channels", C.c_int),
                ("num_res_blocks", C.c_int), ("n_mult", C.c_int), ("channel_mult", C.c_int * 8),
                ("n_attn", C.c_int), ("attention_resolutions", C.c_int * 8), ("num_heads", C.c_int),
                ("context_dim", C.c_int), ("num_classes", C.c_int)]


class SamplerCfg(C.Structure):
    _fields_ = [("sampler", C.c_int), ("num_steps", C.c_int), ("clip_denoised", C.c_int), ("eta", C.c_float),
                ("timestep_map", c_i64p),
                ("coef1", c_f32p), ("coef2", c_f32p), ("log_variance", c_f32p),
                ("sqrt_recip_ab", c_f32p), ("sqrt_recipm1_ab", c_f32p), ("ab", c_f32p), ("ab_prev", c_f32p)]


class GridStats(C.Structure):
    _fields_ = [("n_levels", C.c_int), ("levels", C.c_int * GRID_MAX_LEVELS),
                ("fwd_points", C.c_int64 * GRID_MAX_LEVELS), ("grad_points", C.c_int64)]


_P = C.c_void_p
_SIGS = {
    "surfd_last_error": (C.c_char_p, []),
    "surfd_abi_version": (C.c_int, []),
    "surfd_device_count": (C.c_int, []),
    "surfd_build_config": (C.c_char_p, []),
    "surfd_profile_enable": (C.c_int, [C.c_int]),
    "surfd_profile_read": (C.c_int, [C.c_int, c_i64p, C.POINTER(C.c_double)]),
    "surfd_unet_debug_read": (C.c_int, [_P, C.POINTER(C.c_longlong), C.c_int]),
    "surfd_unet_create": (C.c_int, [C.POINTER(UNetCfg), C.POINTER(_P)]),
    "surfd_unet_destroy": (None, [_P]),
    "surfd_unet_num_params": (C.c_int, [_P]),
    "surfd_unet_param_info": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p), c_i64p, C.POINTER(C.c_int)]),
    "surfd_unet_set_param": (C.c_int, [_P, C.c_char_p, _P, c_i64p, C.c_int, _P]),
    "surfd_unet_finalize": (C.c_int, [_P, _P]),
    "surfd_unet_forward": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, _P]),
    "surfd_unet_set_precision": (C.c_int, [_P, C.c_int]),
    "surfd_unet_set_cu_budget": (C.c_int, [_P, C.c_int]),
    "surfd_unet_set_wide": (C.c_int, [_P, C.c_int]),
    "surfd_unet_saturation_count": (C.c_int, [_P, C.c_int, c_i64p, _P]),
    "surfd_unet_loop_progress": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "surfd_unet_debug_only_op": (C.c_int, [_P, C.c_int]),
    "surfd_unet_debug_run_module": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "surfd_sample_loop": (C.c_int, [_P, C.POINTER(SamplerCfg), _P, _P, _P, _P, _P, C.c_int, C.c_int, _P]),
    "surfd_sample_loop_begin": (C.c_int, [_P, C.POINTER(SamplerCfg), _P, _P, _P, _P, C.c_int, C.c_int, _P]),
    "surfd_sample_loop_run": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int), _P]),
    "surfd_sample_loop_end": (C.c_int, [_P, _P, _P]),
    "surfd_ddpm_step": (C.c_int, [_P, _P, _P, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, _P, C.c_int64, _P]),
    "surfd_ddim_step": (C.c_int, [_P, _P, _P, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int,
                                  C.c_int, _P, C.c_int64, _P]),
    "surfd_decoder_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "surfd_decoder_destroy": (None, [_P]),
    "surfd_decoder_num_params": (C.c_int, [_P]),
    "surfd_decoder_param_info": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p), c_i64p, C.POINTER(C.c_int)]),
    "surfd_decoder_set_param": (C.c_int, [_P, C.c_char_p, _P, c_i64p, C.c_int, _P]),
    "surfd_decoder_finalize": (C.c_int, [_P, _P]),
    "surfd_decoder_set_precision": (C.c_int, [_P, C.c_int]),
    "surfd_decoder_saturation_count": (C.c_int, [_P, C.c_int, c_i64p, _P]),
    "surfd_decoder_sustained_clock": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double), _P]),
    "surfd_decoder_set_grid_blocks": (C.c_int, [_P, C.c_int]),
    "surfd_decoder_bind_latents": (C.c_int, [_P, _P, C.c_int, _P]),
    "surfd_decoder_logits_emb": (C.c_int, [_P, C.c_int, _P, C.c_int64, _P, _P]),
    "surfd_decoder_udf": (C.c_int, [_P, C.c_int, _P, C.c_int64, _P, _P, _P]),
    "surfd_decoder_udf_grad": (C.c_int, [_P, C.c_int, _P, C.c_int64, _P, _P, _P, _P]),
    "surfd_grid_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "surfd_grid_destroy": (None, [_P]),
    "surfd_grid_set_thresholds": (C.c_int, [_P, c_f32p, C.c_int, C.c_float, C.c_float, C.c_float]),
    "surfd_grid_fill": (C.c_int, [_P, _P, C.c_int, _P, _P, _P]),
    "surfd_grid_fill_batch": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P]),
    "surfd_grid_fill_dense": (C.c_int, [_P, _P, C.c_int, C.c_float, _P, _P, _P]),
    "surfd_grid_get_stats": (C.c_int, [_P, C.POINTER(GridStats), _P]),
    "surfd_grid_get_totals": (C.c_int, [_P, C.POINTER(GridStats), c_i64p, C.c_int, _P]),
    "surfd_grid_begin": (C.c_int, [_P, _P, _P, _P]),
    "surfd_grid_level_points": (C.c_int, [_P, C.c_int, _P, C.c_int64, c_i64p, _P]),
    "surfd_grid_level_commit": (C.c_int, [_P, C.c_int, _P, C.c_int64, _P]),
    "surfd_grid_grad_points": (C.c_int, [_P, _P, C.c_int64, c_i64p, _P]),
    "surfd_grid_grad_commit": (C.c_int, [_P, _P, C.c_int64, _P]),
    "surfd_grid_shard_begin": (C.c_int, [_P, _P, _P, _P]),
    "surfd_grid_shard_level_eval": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int64, _P]),
    "surfd_grid_shard_pack": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int64, _P, _P]),
    "surfd_grid_shard_level_commit": (C.c_int, [_P, C.c_int, _P, C.c_int64, C.c_int, _P]),
    "surfd_grid_shard_grad_eval": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int64, _P]),
    "surfd_grid_shard_grad_commit": (C.c_int, [_P, _P, C.c_int64, C.c_int, _P]),
    "surfd_grid_shard_overflows": (C.c_int, [_P, c_i64p, C.c_int, _P]),
    "surfd_mc_udf": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "surfd_mc_iso": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(_P)]),
    "surfd_band_create": (C.c_int, [C.c_int, C.c_int64, C.POINTER(_P)]),
    "surfd_band_destroy": (None, [_P]),
    "surfd_band_compact": (C.c_int, [_P, _P, _P, C.c_float, _P]),
    "surfd_band_fetch": (C.c_int, [_P, _P, c_i64p, C.POINTER(_P), C.POINTER(_P)]),
    "surfd_mc_band_threshold": (C.c_int, [C.c_int, C.POINTER(C.c_float)]),
    "surfd_mc_scratch_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "surfd_mc_scratch_destroy": (None, [_P]),
    "surfd_mc_udf_band": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, C.POINTER(_P)]),
    "surfd_mc_num_vertices": (C.c_int64, [_P]),
    "surfd_mc_num_faces": (C.c_int64, [_P]),
    "surfd_mc_copy": (C.c_int, [_P, _P, _P, _P, _P]),
    "surfd_mc_destroy": (None, [_P]),
    "surfd_write_obj": (C.c_int, [C.c_char_p, _P, C.c_int64, _P, C.c_int64]),
    "surfd_xattn_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "surfd_xattn_destroy": (None, [_P]),
    "surfd_xattn_set_param": (C.c_int, [_P, C.c_char_p, _P, c_i64p, C.c_int, _P]),
    "surfd_xattn_forward": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "surfd_dgcnn_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(_P)]),
    "surfd_dgcnn_destroy": (None, [_P]),
    "surfd_dgcnn_num_params": (C.c_int, [_P]),
    "surfd_dgcnn_param_info": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p), c_i64p, C.POINTER(C.c_int)]),
    "surfd_dgcnn_set_param": (C.c_int, [_P, C.c_char_p, _P, c_i64p, C.c_int, _P]),
    "surfd_dgcnn_finalize": (C.c_int, [_P, _P]),
    "surfd_dgcnn_knn": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P]),
    "surfd_dgcnn_forward": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P]),
    "surfd_dgcnn_forward_features": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P]),
    "surfd_mesh_create": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.POINTER(_P)]),
    "surfd_mesh_destroy": (None, [_P]),
    "surfd_mesh_num_triangles": (C.c_int, [_P]),
    "surfd_mesh_closest": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    "surfd_mesh_build_bvh": (C.c_int, [_P, _P]),
    "surfd_mesh_closest_bvh": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    "surfd_mesh_visits": (C.c_int, [_P, c_i64p, c_i64p, _P]),
    "surfd_mesh_bvh_info": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int32), C.c_int]),
    "surfd_mesh_bvh_read": (C.c_int, [_P, _P, _P, _P]),
    "surfd_rayscene_create": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.POINTER(_P)]),
    "surfd_rayscene_destroy": (None, [_P]),
    "surfd_rayscene_num_triangles": (C.c_int, [_P]),
    "surfd_rayscene_cast": (C.c_int, [_P, _P, C.c_int, C.c_float, C.c_float, C.c_int, _P, _P, _P, _P, _P]),
    "surfd_rayscene_count": (C.c_int, [_P, _P, C.c_int, C.c_float, C.c_float, C.c_int, _P, _P]),
    "surfd_rayscene_skipped": (C.c_int, [_P, c_i64p, c_i64p, _P]),
    "surfd_rayscene_build_bvh": (C.c_int, [_P, _P]),
    "surfd_rayscene_visits": (C.c_int, [_P, c_i64p, c_i64p, _P]),
    "surfd_rayscene_bvh_info": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int32), C.c_int]),
    "surfd_rayscene_bvh_read": (C.c_int, [_P, _P, _P, _P]),
    "surfd_isect_create": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, _P, C.POINTER(_P)]),
    "surfd_isect_destroy": (None, [_P]),
    "surfd_isect_num_triangles": (C.c_int, [_P]),
    "surfd_isect_degenerate": (C.c_int, [_P, _P, _P, _P]),
    "surfd_isect_self": (C.c_int, [_P, C.c_int, _P, _P, C.c_int64, _P, _P]),
    "surfd_isect_between": (C.c_int, [_P, _P, C.c_int, _P, _P, _P, C.c_int64, _P, _P]),
    "surfd_isect_skipped": (C.c_int, [_P, c_i64p, c_i64p, _P]),
    "surfd_winding_create": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.POINTER(_P)]),
    "surfd_winding_destroy": (None, [_P]),
    "surfd_winding_num_triangles": (C.c_int, [_P]),
    "surfd_winding_eval": (C.c_int, [_P, _P, C.c_int64, C.c_int, _P, _P]),
    "surfd_winding_build_bvh": (C.c_int, [_P, _P]),
    "surfd_winding_eval_fast": (C.c_int, [_P, _P, C.c_int64, C.c_double, C.c_int, _P, _P]),
    "surfd_winding_visits": (C.c_int, [_P, c_i64p, c_i64p, _P]),
    "surfd_winding_bvh_info": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int32), C.c_int]),
    "surfd_winding_bvh_read": (C.c_int, [_P, _P, _P, _P, _P]),
    "surfd_meshtopo_create": (C.c_int, [_P, C.c_int, C.c_int, _P, C.POINTER(_P)]),
    "surfd_meshtopo_destroy": (None, [_P]),
    "surfd_meshtopo_counts": (C.c_int, [_P, c_i64p, c_i64p, c_i64p, c_i64p]),
    "surfd_meshtopo_read": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "surfd_meshtopo_components": (C.c_int, [_P, C.c_int, _P, c_i64p, _P]),
    "surfd_meshtopo_border_loops": (C.c_int, [_P, _P, _P, c_i64p, _P]),
    "surfd_meshtopo_orient": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "surfd_meshtopo_weld": (C.c_int, [_P, C.c_int, _P, _P, c_i64p, _P]),
    "surfd_meshsmooth_create": (C.c_int, [_P, C.c_int, C.c_int, _P, C.POINTER(_P)]),
    "surfd_meshsmooth_destroy": (None, [_P]),
    "surfd_meshsmooth_counts": (C.c_int, [_P, c_i64p, c_i64p, c_i64p, c_i64p]),
    "surfd_meshsmooth_laplacian": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "surfd_meshsmooth_umbrella": (C.c_int, [_P, _P, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, _P, _P]),
    "surfd_meshsmooth_vertex_normals": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P]),
    "surfd_meshclean_cull_and_merge": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_double, _P, _P, c_i64p, _P]),
    "surfd_meshclean_drop_duplicate_faces": (C.c_int, [_P, C.c_int, _P, c_i64p, _P]),
    "surfd_meshclean_drop_degenerate_faces": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_double, _P, c_i64p, _P]),
    "surfd_meshclean_fill_small_holes": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int64, c_i64p, _P]),
    "surfd_meshfill_plan": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, c_i64p, _P, C.POINTER(_P)]),
    "surfd_meshfill_loop_sizes": (C.c_int, [_P, _P, C.c_int64, _P]),
    "surfd_meshfill_run": (C.c_int, [_P, _P, C.c_int64, _P, c_i64p, _P]),
    "surfd_meshfill_destroy": (None, [_P]),
    "surfd_meshsimplify_cluster": (C.c_int, [_P, C.c_int, _P, C.c_int, C.POINTER(C.c_double), C.c_double, C.c_int, C.c_double, _P, _P, _P, c_i64p, _P]),
    "surfd_meshsimplify_decimate": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_uint64,
                                              _P, _P, _P, c_i64p, _P]),
    "surfd_meshremesh_create": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_double, C.c_double, C.c_double, C.c_uint64, _P, C.POINTER(_P)]),
    "surfd_meshremesh_destroy": (None, [_P]),
    "surfd_meshremesh_iterate": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, c_i64p, _P]),
    "surfd_meshremesh_sizes": (C.c_int, [_P, c_i64p, c_i64p]),
    "surfd_meshremesh_get_positions": (C.c_int, [_P, _P, _P, _P]),
    "surfd_meshremesh_set_positions": (C.c_int, [_P, _P, _P]),
    "surfd_meshremesh_emit": (C.c_int, [_P, _P, _P, _P, c_i64p, _P]),
    "surfd_cloud_nn": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "surfd_cloud_nn_matrix": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_float, _P, _P, _P]),
    "surfd_cloud_nn_matrix_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "surfd_cloud_fps_workspace_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "surfd_cloud_fps": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P, _P, _P]),
    "surfd_cloud_normals": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P, _P]),
    "surfd_raster_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "surfd_raster_destroy": (None, [_P]),
    "surfd_raster_render": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, _P, c_f32p, C.c_int, C.c_int, c_f32p, C.c_float,
                                      _P, _P, _P, _P, _P, _P, _P, _P]),
    "surfd_raster_contours": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_float, C.c_float, _P, _P]),
    "surfd_voxel_workspace_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "surfd_voxel_surface": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    "surfd_voxel_solid": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P, _P]),
    "surfd_voxel_points": (C.c_int, [_P, C.c_int, C.c_float, C.c_float, C.c_int, _P, _P, _P]),
    "surfd_voxel_iou": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "surfd_mc_lut_count": (C.c_int, []),
    "surfd_mc_lut": (C.c_int, [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.POINTER(C.c_byte)), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "surfd_mcd_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "surfd_mcd_destroy": (None, [_P]),
    "surfd_mcd_run": (C.c_int, [_P, _P, C.c_double, C.c_int, _P, c_i64p, c_i64p]),
    "surfd_mcd_emit": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "surfd_mcd_active": (C.c_int, [_P, c_i64p]),
    "surfd_mcd_classify": (C.c_int, [_P, _P, C.c_double, C.c_int, _P]),
}
EXPORTED_SYMBOLS = tuple(_SIGS)

_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the HIP extension must be built first "
                "(python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)          # AttributeError here = stale/partial library: rebuild
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        msg = lib().surfd_last_error()
        raise RuntimeError(f"libsurfd_hip error {rc}: {msg.decode() if msg else '?'}")


def ptr(t) -> Optional[int]:
    """device (or host) address of a contiguous tensor, None -> NULL"""
    if t is None:
        return None
    assert t.is_contiguous(), "libsurfd_hip needs contiguous buffers"
    return t.data_ptr()


def stream() -> int:
    import torch
    return torch.cuda.current_stream().cuda_stream


def shape_arr(shape):
    return (C.c_int64 * max(len(shape), 1))(*shape)


class ParamBinder:
    """Keeps one native handle's copy of a module's weights current (CbnDecoder, Dgcnn, MDM, CrossAttention).

    set_param / finalize: names of the handle's entry points (finalize: None where there is none); wanted: which
    state_dict keys the handle takes (None: all).  One binder per handle: ``bound`` is the key that handle was last sent."""

    def __init__(self, set_param: str, finalize: Optional[str] = None, wanted=None):
        self._set_param, self._finalize, self._wanted = set_param, finalize, wanted
        self._slots = None
        self.bound = None

    def key(self, module) -> tuple:
        # (storage address, version) of every tensor the handle is sent.  The SLOTS — (key, owning dict, leaf name) in
        # state_dict order, parameters and persistent buffers — are collected once (the module tree never changes;
        # rebuilding a 101-entry state_dict on every udf call is measurable in callback mode); the tensors are looked up in
        # them on every call, so any rebinding is seen whether or not it goes through a hook: `.to()` / `.cuda()`,
        # `load_state_dict(assign=True)` on this module or a parent, `decoder.blocks.0.fc_0.weight = nn.Parameter(...)`
        # (ADVICE r2).
        if self._slots is None:
            slots = []
            for prefix, mod in module.named_modules():
                for owner in (mod._parameters, mod._buffers):
                    for name in owner:
                        k = f"{prefix}.{name}" if prefix else name
                        if name not in mod._non_persistent_buffers_set and (self._wanted is None or self._wanted(k)):
                            slots.append((k, owner, name))
            self._slots = slots
        return tuple((t.data_ptr(), t._version) for _, d, n in self._slots for t in (d[n],) if t is not None)

    def bind(self, module, handle) -> bool:
        """Sends every tensor and finalizes if the key changed since this handle was last sent; True when it did."""
        key = self.key(module)
        if key == self.bound:
            return False
        import torch
        L, st = lib(), stream()
        set_param = getattr(L, self._set_param)
        for k, d, n in self._slots:
            t = d[n]
            if t is None:
                continue
            if n == "num_batches_tracked":
                check(set_param(handle, k.encode(), None, shape_arr(()), 0, st))
                continue
            t = t.detach()
            if t.dtype != torch.float32 or not t.is_contiguous():
                t = t.float().contiguous()
            check(set_param(handle, k.encode(), ptr(t), shape_arr(tuple(t.shape)), t.dim(), st))
        if self._finalize:
            check(getattr(L, self._finalize)(handle, st))
        torch.cuda.current_stream().synchronize()      # temporaries made above may be freed now
        self.bound = key
        return True
