"""ctypes binding of libvgt_hip.so (the C ABI declared in include/vgt_hip.h).

This is test / bench plumbing: the product is the shared library and the C++ glue in
include/vgt_hip/.  There is no CPU fallback here -- if the library is missing, or no HIP
device is usable, the calls raise.
"""
import collections
import ctypes
import threading
import weakref
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VGT_HIP_LIB") or os.path.join(_HERE, "libvgt_hip.so")  # override: diagnostic builds
# The product library plus the cross-check EDT implementations and the testing hooks (-DVGT_HIP_TESTING): what the
# parity tests load NEXT TO the product library (Context(testing=True)) to check the default pipeline against
# independent implementations.  Nothing in the product path uses it.
TESTING_LIB_PATH = os.environ.get("VGT_HIP_TESTING_LIB") or os.path.join(_HERE, "libvgt_hip_testing.so")
_LIB = None

_i64 = ctypes.c_int64
_i32 = ctypes.c_int32
_f32 = ctypes.c_float
_f64 = ctypes.c_double
_p = ctypes.c_void_p
_sz = ctypes.c_size_t
_int = ctypes.c_int

# name -> (restype, argtypes); mirrors include/vgt_hip.h one to one.
SIGNATURES = {
    "vgt_hip_abi_version": (_int, []),
    "vgt_hip_last_error": (ctypes.c_char_p, []),
    "vgt_hip_device_count": (_int, [ctypes.POINTER(_int)]),
    "vgt_hip_device_name": (_int, [_int, ctypes.c_char_p, _sz]),
    "vgt_hip_create": (_int, [_int, _int, ctypes.POINTER(_p)]),
    "vgt_hip_destroy": (None, [_p]),
    "vgt_hip_trim": (_int, [_p]),
    "vgt_hip_set_stream": (_int, [_p, _p]),
    "vgt_hip_reset_stream": (_int, [_p]),
    "vgt_hip_synchronize": (_int, [_p]),
    "vgt_hip_device_of": (_int, [_p]),
    "vgt_hip_tracking_grids_create": (_int, [_p, _i64, _i32, ctypes.POINTER(_p)]),
    "vgt_hip_tracking_grids_destroy": (None, [_p]),
    "vgt_hip_tracking_grids_num_cells": (_i64, [_p]),
    "vgt_hip_tracking_grids_num_grids": (_i32, [_p]),
    "vgt_hip_tracking_grids_offset": (_i64, [_p, _sz]),
    "vgt_hip_tracking_grids_dev_ptr": (_p, [_p, _sz]),
    "vgt_hip_tracking_grids_clear": (_int, [_p, _p]),
    "vgt_hip_raycast_points_f32": (_int, [_p, _p, _sz, _p, _i64, _f32, _p, _f32, _f32, _f32, _f32,
                                          _f32, _i32, _i32, _i32]),
    "vgt_hip_raycast_pointcloud2_f32": (_int, [_p, _p, _sz, _p, _i64, _i64, _i64, _f32, _p, _f32, _f32, _f32,
                                               _f32, _f32, _i32, _i32, _i32]),
    "vgt_hip_raycast_points_f32_dev": (_int, [_p, _p, _sz, _p, _i64, _f32, _p, _f32, _f32, _f32,
                                              _f32, _f32, _i32, _i32, _i32]),
    "vgt_hip_raycast_points_f64": (_int, [_p, _p, _sz, _p, _i64, _f64, _p, _f64, _f64, _f64, _f64,
                                          _f64, _i32, _i32, _i32]),
    "vgt_hip_filter_grid_create": (_int, [_p, _i64, _p, ctypes.POINTER(_p)]),
    "vgt_hip_filter_grid_create_deferred": (_int, [_p, _i64, _p, ctypes.POINTER(_p)]),
    "vgt_hip_filter_grid_destroy": (None, [_p]),
    "vgt_hip_filter_grid_num_cells": (_i64, [_p]),
    "vgt_hip_filter_grid_dev_ptr": (_p, [_p]),
    "vgt_hip_filter_tracking_grids": (_int, [_p, _p, _f32, _i32, _i32, _p]),
    "vgt_hip_filter_tracking_grids_f64": (_int, [_p, _p, _f64, _i32, _i32, _p]),
    "vgt_hip_retrieve_tracking_grid": (_int, [_p, _p, _sz, _p]),
    "vgt_hip_retrieve_filtered_grid": (_int, [_p, _p, _p]),
    "vgt_hip_sdf_from_occupancy_f32": (_int, [_p, _p, _i64, _i64, _i64, _f64, _int, _int, _p, _p, _p]),
    "vgt_hip_sdf_from_mask_u8": (_int, [_p, _p, _i64, _i64, _i64, _f64, _int, _p, _p, _p]),
    "vgt_hip_sdf_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "vgt_hip_sdf_workspace_bytes_for_variant": (_sz, [_i64, _i64, _i64, _int]),
    "vgt_hip_sdf_estimate_distance": (_int, [_p, _p, _i64, _i64, _i64, _f64, _p, _p, _i64, _p, _p]),
    "vgt_hip_sdf_estimate_distance_dev": (_int, [_p, _p, _i64, _i64, _i64, _f64, _p, _p, _i64, _p, _p]),
    "vgt_hip_sdf_fine_gradient": (_int, [_p, _p, _i64, _i64, _i64, _f64, _p, _p, _i64, _f64, _p, _p]),
    "vgt_hip_sdf_project_out_of_collision": (_int, [_p, _p, _i64, _i64, _i64, _f64, _p, _p, _p, _i64, _f64, _f64, _i32,
                                                    _p, _p, _p, _p]),
    "vgt_hip_sdf_project_out_of_collision_dev": (_int, [_p, _p, _i64, _i64, _i64, _f64, _p, _p, _p, _i64, _f64, _f64,
                                                        _i32, _p, _p, _p, _p]),
    "vgt_hip_cast_segments": (_int, [_p, _p, _i64, _i64, _i64, _f64, _i32, _int, _f64, ctypes.c_uint32, _p, _p, _i64,
                                     _p, _p, _p, _p, _p, _p]),
    "vgt_hip_cast_segments_dev": (_int, [_p, _p, _i64, _i64, _i64, _f64, _i32, _int, _f64, ctypes.c_uint32, _p, _p, _i64,
                                         _p, _p, _p, _p, _p, _p]),
    "vgt_hip_check_spheres": (_int, [_p, _p, _i64, _i64, _i64, _f64, _p, _p, _p, _p, _i64, _p, _i64, _i64, _f64,
                                     ctypes.c_uint32, _p, _p, _p, _p, _p, _p, _p, _p]),
    "vgt_hip_check_spheres_dev": (_int, [_p, _p, _i64, _i64, _i64, _f64, _p, _p, _p, _p, _i64, _p, _i64, _i64, _f64,
                                         ctypes.c_uint32, _p, _p, _p, _p, _p, _p, _p, _p]),
    "vgt_hip_rasterize_spheres": (_int, [_p, _i64, _i64, _i64, _f64, _p, _p, _p, _i64, _p, _i64, _i64, _f64, _i64,
                                         ctypes.c_uint32, _p]),
    "vgt_hip_rasterize_spheres_dev": (_int, [_p, _i64, _i64, _i64, _f64, _p, _p, _p, _i64, _p, _i64, _i64, _f64, _i64,
                                             ctypes.c_uint32, _p]),
    "vgt_hip_spheres_cover_points": (_int, [_p, _p, _i64, _p, _p, _p, _i64, _p, _i64, _i64, _f64, ctypes.c_uint32,
                                            _p, _p, _p]),
    "vgt_hip_spheres_cover_points_dev": (_int, [_p, _p, _i64, _p, _p, _p, _i64, _p, _i64, _i64, _f64, ctypes.c_uint32,
                                                _p, _p, _p]),
    "vgt_hip_align_points": (_int, [_p, _p, _i64, _i64, _i64, _f64, _p, _p, _p, _i64, _p, _i64, _p, _i32, _i32, _f64,
                                    _f64, _f64, _f64, _f64, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "vgt_hip_align_points_workspace_bytes": (_sz, [_i64, _i64]),
    "vgt_hip_align_points_dev": (_int, [_p, _p, _i64, _i64, _i64, _f64, _p, _p, _p, _i64, _p, _i64, _p, _i32, _i32, _f64,
                                        _f64, _f64, _f64, _f64, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _sz]),
    "vgt_hip_kinematics_create": (_int, [_p, _i64, _i64, _p, _p, _p, _p, _p, ctypes.POINTER(_p)]),
    "vgt_hip_kinematics_destroy": (None, [_p]),
    "vgt_hip_kinematics_num_links": (_i64, [_p]),
    "vgt_hip_kinematics_num_joints": (_i64, [_p]),
    "vgt_hip_kinematics_lds_links": (_i32, []),
    "vgt_hip_forward_kinematics": (_int, [_p, _p, _p, _i64, _p, _p, _p, _p]),
    "vgt_hip_forward_kinematics_dev": (_int, [_p, _p, _p, _i64, _p, _p, _p, _p]),
    "vgt_hip_clearance_joint_gradient": (_int, [_p, _p, _p, _i64, _p, _p, _i64, _p, _p, _p, _p, _p]),
    "vgt_hip_clearance_joint_gradient_dev": (_int, [_p, _p, _p, _i64, _p, _p, _i64, _p, _p, _p, _p, _p]),
    "vgt_hip_check_spheres_from_joints": (_int, [_p, _p, _i64, _i64, _i64, _f64, _p, _p, _p, _p, _i64, _p, _p, _i64, _p,
                                                 _p, _f64, ctypes.c_uint32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "vgt_hip_ik_max_chain_joints": (_i32, []),
    "vgt_hip_solve_ik": (_int, [_p, _p, _i32, _p, _i64, _i64, _p, _p, _p, _p, _i32, _f64, _f64, _f64, _f64, _p, _p, _p,
                                _p, _p, _p]),
    "vgt_hip_solve_ik_workspace_bytes": (_sz, [_i64, _i64]),
    "vgt_hip_solve_ik_dev": (_int, [_p, _p, _i32, _p, _i64, _i64, _p, _p, _p, _p, _i32, _f64, _f64, _f64, _f64, _p, _p,
                                    _p, _p, _p, _p, _p, _sz]),
    "vgt_hip_check_motions": (_int, [_p, _p, _i64, _i64, _i64, _f64, _p, _p, _p, _p, _i64, _p, _p, _p, _p, _i32, _i64, _p,
                                     _p, _f64, ctypes.c_uint32, _p, _p, _p, _p, _p, _p, _p]),
    "vgt_hip_check_motions_dev": (_int, [_p, _p, _i64, _i64, _i64, _f64, _p, _p, _p, _p, _i64, _p, _p, _p, _p, _i32, _i64,
                                         _p, _p, _f64, ctypes.c_uint32, _p, _p, _p, _p, _p, _p, _p]),
    "vgt_hip_motion_tile_samples": (_i32, [_i64]),
    "vgt_hip_clearance_cost": (_int, [_p, _p, _i64, _i64, _i64, _f64, _p, _p, _p, _p, _i64, _p, _p, _i64, _p, _p, _f64,
                                      ctypes.c_uint32, _p, _p, _p, _p, _p, _p]),
    "vgt_hip_clearance_cost_dev": (_int, [_p, _p, _i64, _i64, _i64, _f64, _p, _p, _p, _p, _i64, _p, _p, _i64, _p, _p,
                                          _f64, ctypes.c_uint32, _p, _p, _p, _p, _p, _p]),
    "vgt_hip_cost_tile_samples": (_i32, [_i64]),
    "vgt_hip_check_self_collision": (_int, [_p, _p, _p, _i64, _p, _i64, _p, _p, _i64, _p, _p, _f64, ctypes.c_uint32,
                                            _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "vgt_hip_check_self_collision_dev": (_int, [_p, _p, _p, _i64, _p, _i64, _p, _p, _i64, _p, _p, _f64, ctypes.c_uint32,
                                                _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "vgt_hip_check_self_collision_poses": (_int, [_p, _p, _p, _i64, _p, _i64, _p, _i64, _i64, _p, _f64, ctypes.c_uint32,
                                                  _p, _p, _p, _p, _p, _p, _p, _p]),
    "vgt_hip_check_self_collision_poses_dev": (_int, [_p, _p, _p, _i64, _p, _i64, _p, _i64, _i64, _p, _f64,
                                                      ctypes.c_uint32, _p, _p, _p, _p, _p, _p, _p, _p]),
    "vgt_hip_self_collision_pairs": (_int, [_p, _i64, _p, _i64, _p, _i64, ctypes.c_uint32, _p, _i64, _p]),
    "vgt_hip_self_collision_tile_samples": (_i32, [_i64, _i64]),
    "vgt_hip_check_motions_with_self": (_int, [_p, _p, _i64, _i64, _i64, _f64, _p, _p, _p, _p, _i64, _p, _i64, _p, _p, _p,
                                               _p, _i32, _i64, _p, _p, _f64, _f64, ctypes.c_uint32, _p, _p, _p, _p, _p,
                                               _p, _p, _p, _p, _p, _p]),
    "vgt_hip_check_motions_with_self_dev": (_int, [_p, _p, _i64, _i64, _i64, _f64, _p, _p, _p, _p, _i64, _p, _i64, _p, _p,
                                                   _p, _p, _i32, _i64, _p, _p, _f64, _f64, ctypes.c_uint32, _p, _p, _p,
                                                   _p, _p, _p, _p, _p, _p, _p, _p]),
    "vgt_hip_motion_self_tile_samples": (_i32, [_i64, _i64]),
    "vgt_hip_nearest_workspace_bytes": (ctypes.c_size_t, [_i64, _i64, _i64]),
    "vgt_hip_nearest_dev": (_int, [_p, _p, _i64, _i64, _i64, _int, _p, _p, _p, ctypes.c_size_t]),
    "vgt_hip_nearest_from_occupancy_f32": (_int, [_p, _p, _i64, _i64, _i64, _int, _p, _p]),
    "vgt_hip_nearest_from_mask_u8": (_int, [_p, _p, _i64, _i64, _i64, _p, _p]),
    "vgt_hip_cells_nearest": (_int, [_p, _p, _p, _i64, _int, _p, _p, _p]),
    "vgt_hip_sdf_local_extrema_map": (_int, [_p, _p, _i64, _i64, _i64, _f64, _p, _p]),
    "vgt_hip_sdf_local_extrema_map_dev": (_int, [_p, _p, _i64, _i64, _i64, _f64, _p, _p]),
    "vgt_hip_connected_components": (_int, [_p, _p, _i64, _i64, _i64, _p, _p]),
    "vgt_hip_connected_components_dev": (_int, [_p, _p, _i64, _i64, _i64, _p, _p]),
    "vgt_hip_cells_connected_components": (_int, [_p, _p, _int, _p, _p]),
    "vgt_hip_cells_spatial_segments": (_int, [_p, _p, _p, _f64, _p, _p]),
    "vgt_hip_cells_spatial_segments_dev": (_int, [_p, _p, _p, _f64, _p, _p]),
    "vgt_hip_cells_update_spatial_segments": (_int, [_p, _p, _f64, _f64, _int, _int, _p, _p, _p]),
    "vgt_hip_component_surface_mask": (_int, [_p, _p, _p, _i64, _i64, _i64, _int, _p]),
    "vgt_hip_component_surface_mask_dev": (_int, [_p, _p, _p, _i64, _i64, _i64, _int, _p]),
    "vgt_hip_select_cells": (_int, [_p, _p, _p, _i64, _i64, _i64, _int, _int, _f32, _p, _p, _p, _i64, _p]),
    "vgt_hip_select_cells_dev": (_int, [_p, _p, _p, _i64, _i64, _i64, _int, _int, _f32, _p, _p, _p, _i64, _p]),
    "vgt_hip_cells_select": (_int, [_p, _p, _p, _int, _int, _p, _p, _p, _int, _i64, _p]),
    "vgt_hip_extract_surface": (_int, [_p, _p, _i64, _i64, _i64, _f32, _int, _f64, _p, _p, _p, _i64, _p, _i64, _p, _p]),
    "vgt_hip_extract_surface_dev": (_int, [_p, _p, _i64, _i64, _i64, _f32, _int, _f64, _p, _p, _p, _i64, _p, _i64, _p,
                                           _p]),
    "vgt_hip_cells_extract_surface": (_int, [_p, _p, _f64, _p, _p, _p, _i64, _p, _i64, _p, _p]),
    "vgt_hip_travel_cost_workspace_bytes": (ctypes.c_size_t, [_i64, _i64, _i64]),
    "vgt_hip_travel_cost": (_int, [_p, _p, _i64, _i64, _i64, _i32, _int, _f64, _p, ctypes.c_uint32, _p, _p, _i64,
                                   ctypes.c_uint32, _p, _p, _p]),
    "vgt_hip_travel_cost_dev": (_int, [_p, _p, _i64, _i64, _i64, _i32, _int, _f64, _p, ctypes.c_uint32, _p, _p, _i64,
                                       ctypes.c_uint32, _p, _p, _p, _p, _sz]),
    "vgt_hip_cells_travel_cost": (_int, [_p, _p, _p, _i64, _int, _p, ctypes.c_uint32, _p, _p, _i64, ctypes.c_uint32, _p,
                                         _p, _p]),
    "vgt_hip_trace_paths": (_int, [_p, _p, _i64, _p, _i64, _i32, _p, _p, _p]),
    "vgt_hip_trace_paths_dev": (_int, [_p, _p, _i64, _p, _i64, _i32, _p, _p, _p]),
    "vgt_hip_component_topology_dev": (_int, [_p, _p, _p, _i64, _i64, _i64, _int, ctypes.c_uint32, _p]),
    "vgt_hip_component_topology": (_int, [_p, _p, _i64, _i64, _i64, _int, _p, _p, _p, ctypes.c_uint64]),
    "vgt_hip_cells_component_topology": (_int, [_p, _p, _int, _int, _p, _p, _p, ctypes.c_uint64]),
    "vgt_hip_rasterize_mesh": (_int, [_p, _p, _i64, _p, _i64, _p, _int, _i64, _i64, _i64, _f64, _p, _p, _int, _int]),
    "vgt_hip_rasterize_mesh_dev": (_int, [_p, _p, _i64, _p, _i64, _p, _int, _i64, _i64, _i64, _f64, _p, _p, _int, _int]),
    "vgt_hip_mesh_grid_for": (_int, [_p, _i64, _f64, _p, _p, _p, _p]),
    "vgt_hip_fill_enclosed": (_int, [_p, _p, _int, _i64, _i64, _i64, _int, _p]),
    "vgt_hip_fill_enclosed_dev": (_int, [_p, _p, _int, _i64, _i64, _i64, _int, _p]),
    "vgt_hipx_sdf_multi": (_int, [_p, _int, _p, _i64, _i64, _i64, _f64, _int, _int, _p, _p, _p]),
    "vgt_hipx_release": (None, []),
    "vgt_hipx_last_timing": (_int, [_p]),
    "vgt_hipx_point_share": (_int, [_i64, _i32, _i32, _p, _p]),
    "vgt_hipx_raycast_points_split": (_int, [_p, _p, _sz, _p, _int, _p, _i64, _f32, _p, _f32, _f32, _f32, _f32,
                                             _f32, _i32, _i32, _i32]),
    "vgt_hip_sdf_dev": (_int, [_p, _p, _i64, _i64, _i64, _f64, _int, _int, _p, _p, _sz, _p]),
    "vgt_hip_sdf_dev_timed": (_int, [_p, _p, _i64, _i64, _i64, _f64, _int, _int, _p, _p, _sz, _p, _p]),
    "vgt_hip_sdf_batch_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64]),
    "vgt_hip_sdf_batch_dev": (_int, [_p, _p, _i64, _i64, _i64, _i64, _f64, _int, _int, _p, _p, _sz, _p]),
    "vgt_hip_sdf_batch_from_occupancy_f32": (_int, [_p, _p, _i64, _i64, _i64, _i64, _f64, _int, _int, _p, _p, _p]),
    "vgt_hip_cells_object_sdfs": (_int, [_p, _p, _p, _i64, _f64, _int, _int, _p, _p, _p]),
    "vgt_hip_cells_create": (_int, [_p, _p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32,
                                   ctypes.c_int32, _p]),
    "vgt_hip_cells_destroy": (None, [_p]),
    "vgt_hip_cells_object_ids": (_int, [_p, _p, _p, ctypes.c_int64, _p]),
    "vgt_hip_cells_sdf": (_int, [_p, _p, _p, ctypes.c_int64, ctypes.c_double, _int, _int, _p, _p, _p]),
    "vgt_hip_cells_free_and_named_objects_sdf": (_int, [_p, _p, ctypes.c_double, _int, _int, _p, _p, _p]),
    "vgt_hip_sdf_coarse_gradient": (_int, [_p, _p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_double,
                                          _int, _p, _p, _p]),
    "vgt_hip_sdf_coarse_gradient_dev": (_int, [_p, _p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                              ctypes.c_double, _int, _p, _p, _p]),
    "vgt_hip_sdf_slab_carries_dev": (_int, [_p, _p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64,
                                            ctypes.c_int64, _p]),
    "vgt_hip_timing_start": (_int, [_p, ctypes.c_int32]),
    "vgt_hip_timing_stop": (_int, [_p, _p, _p]),
    "vgt_hip_sdf_slab_summary_bytes": (_sz, [_i64, _i64]),
    "vgt_hip_sdf_slab_carries_bytes": (_sz, [_i64, _i64]),
    "vgt_hip_sdf_slab_range": (_int, [_i64, ctypes.c_int32, ctypes.c_int32, _p, _p]),
    "vgt_hip_sdf_slab_begin_dev": (_int, [_p, _p, _i64, _i64, _i64, _i64, _int, _p, _sz, _p, _p]),
    "vgt_hip_sdf_slab_finish_dev": (_int, [_p, _i64, _i64, _i64, _i64, _i64, _f64, _int, _p, _p, _p,
                                           _sz, _p, _p]),
}


# exported by libvgt_hip_testing.so only (include/vgt_hip.h under VGT_HIP_TESTING)
TESTING_SIGNATURES = {
    "vgt_hip_set_edt_variant": (_int, [_p, _int]),
    "vgt_hip_debug_finalize_check": (_int, [_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_double, _p, _p]),
    "vgt_hip_testing_set_host_pipeline_min_voxels": (_int, [ctypes.c_int64]),
    "vgt_hip_testing_set_short_line_rows": (_int, [_int]),
    "vgt_hip_testing_set_coarse_hull": (_int, [_int]),
    "vgt_hip_testing_set_sweep_slots": (_int, [_int]),
    "vgt_hip_testing_one_class_counts": (_int, [_p, _p, _i64, _i64, _i64, _p]),
    "vgt_hip_testing_x_pass_choice": (_int, [_p, _p, _i64, _i64, _i64, _p]),
    "vgt_hip_testing_set_check_spheres_workgroups": (_int, [_int]),
    "vgt_hip_testing_set_sphere_volume_workgroups": (_int, [_int]),
    "vgt_hip_testing_set_align_workgroups": (_int, [_int]),
    "vgt_hip_testing_set_kinematics_workgroups": (_int, [_int]),
    "vgt_hip_testing_set_motion_workgroups": (_int, [_int]),
    "vgt_hip_testing_set_cost_workgroups": (_int, [_int]),
    "vgt_hip_testing_motion_launch_geometry": (_int, [_i64, _i64, _p, _p]),
    "vgt_hip_testing_cost_launch_geometry": (_int, [_i64, _i64, _int, _p, _p, _p, _p]),
    "vgt_hip_testing_set_self_collision_workgroups": (_int, [_int]),
    "vgt_hip_testing_set_motion_self_workgroups": (_int, [_int]),
    "vgt_hip_testing_set_sphere_volume_counters": (_int, [_p]),
    "vgt_hip_testing_class_record_bytes": (_sz, [_i64, _i64, _i64]),
    "vgt_hip_testing_class_records_dev": (_int, [_p, _p, _i64, _i64, _i64, _int, _i64, _p, _p]),
}


# closest-point rules of the mesh rasterizer (VGT_HIP_MESH_RULE_*)
MESH_RULE_REFERENCE = 0
MESH_RULE_NEAREST = 1

# statuses of sdf_project_out_of_collision (VGT_HIP_PROJECT_*)
PROJECT_OK = 0
PROJECT_OUTSIDE = 1
PROJECT_FLAT_GRADIENT = 2
PROJECT_LEFT_GRID = 3
PROJECT_ITERATION_LIMIT = 4

# modes, flag and statuses of cast_segments (VGT_HIP_SEGMENT_*)
SEGMENT_OCCUPANCY = 0
SEGMENT_SDF_BELOW = 1
SEGMENT_WALK_THROUGH = 1
SEGMENT_CLEAR = 0
SEGMENT_HIT = 1
SEGMENT_MISSED_GRID = 2
SEGMENT_INVALID = 3

# flag and statuses of check_spheres (VGT_HIP_SPHERES_*)
SPHERES_OUTSIDE_IS_COLLISION = 1
SPHERES_CLEAR = 0
SPHERES_COLLISION = 1
SPHERES_NO_VALUE = 2
# flag of rasterize_spheres (VGT_HIP_SPHERES_KEEP)
SPHERES_KEEP = 1
# statuses of align_points (VGT_HIP_ALIGN_*)
# joint types of a kinematic tree and the status bits of the forward kinematics (VGT_HIP_JOINT_*, VGT_HIP_FK_*)
JOINT_FIXED, JOINT_REVOLUTE, JOINT_PRISMATIC = 0, 1, 2
FK_NOT_COMPUTABLE = 1
FK_OUTSIDE_LIMITS = 2
# statuses of solve_ik (VGT_HIP_IK_*)
IK_CONVERGED = 0
IK_ITERATION_LIMIT = 1
IK_DEGENERATE = 2
IK_NOT_COMPUTABLE = 3
# flag and statuses of check_motions (VGT_HIP_MOTION_*)
MOTION_STOP_AT_COLLISION = 2
MOTION_CLEAR = 0
MOTION_COLLISION = 1
MOTION_NO_VALUE = 2
MOTION_INVALID = 3
# flags and statuses of check_self_collision and self_collision_pairs (VGT_HIP_SELF_*)
SELF_NO_VALUE_IS_COLLISION = 1
SELF_CLEAR = 0
SELF_COLLISION = 1
SELF_NO_VALUE = 2
SELF_PAIRS_SKIP_ADJACENT = 1
# flag and cause bits of check_motions_with_self (VGT_HIP_MOTION_SELF_*, VGT_HIP_MOTION_CAUSE_*)
MOTION_SELF_NO_VALUE_IS_COLLISION = 4
MOTION_CAUSE_ENVIRONMENT = 1
MOTION_CAUSE_SELF = 2
ALIGN_CONVERGED = 0
ALIGN_ITERATION_LIMIT = 1
ALIGN_DEGENERATE = 2
ALIGN_TOO_FEW = 3

# selection rules, value classes and cell members of select_cells / Cells.select (VGT_HIP_SELECT_*, VGT_HIP_CLASS_*,
# VGT_HIP_CELL_MEMBER_*)
SELECT_ALL = 0
SELECT_SURFACE_26 = 1
SELECT_COMPONENT_SURFACE = 2
CLASS_ABOVE = 0x01
CLASS_BELOW = 0x02
CLASS_EQUAL = 0x04
CLASS_UNORDERED = 0x08
CELL_MEMBER_NONE = 0
CELL_MEMBER_OBJECT_ID = 1
CELL_MEMBER_COMPONENT = 2
CELL_MEMBER_SPATIAL_SEGMENT = 3

# vgt_hip_component_topology_t
COMPONENT_TOPOLOGY = np.dtype([(name, np.int32) for name in (
    "present", "num_holes", "num_voids", "num_surfaces", "m3", "m5", "m6", "num_surface_vertices")])


# what Context.cast_segments returns: one entry per segment; min_value / min_index are None unless asked for
SegmentCasts = collections.namedtuple("SegmentCasts", "status hit_index hit_fraction cells_examined min_value min_index")


# what Context.check_spheres returns: one entry per configuration; sphere_clearance [B, S] / sphere_gradient [B, S, 3]
# are None unless per_sphere
SphereChecks = collections.namedtuple(
    "SphereChecks", "status min_clearance min_sphere num_below num_outside min_gradient sphere_clearance sphere_gradient")


# what Context.spheres_cover_points returns: one entry per point; filtered [N, 3] float32 is None unless asked for
PointCover = collections.namedtuple("PointCover", "first_configuration first_sphere filtered")


# what Context.align_points returns: one entry per pose; poses [B, 16] column-major, normal_equations [B, 27] (H's 21
# entries row-major over j <= k, then b), last_step [B, 6]
CloudAlignment = collections.namedtuple(
    "CloudAlignment",
    "poses status num_used num_outside num_rejected sum_squared evaluations normal_equations last_step")


def _cloud_poses(poses):
    """[B, 16] float64 column-major world_from_points; poses may come as [B, 4, 4] matrices."""
    poses = np.asarray(poses, dtype=np.float64)
    if poses.ndim == 3:
        if poses.shape[1:] != (4, 4):
            raise ValueError("poses must have the shape [B, 16] or [B, 4, 4]")
        poses = poses.transpose(0, 2, 1).reshape(poses.shape[0], 16)
    if poses.ndim != 2 or poses.shape[1] != 16:
        raise ValueError("poses must have the shape [B, 16] or [B, 4, 4]")
    return np.ascontiguousarray(poses)


# what Context.check_spheres_from_joints returns: SphereChecks' fields, then fk_status [B] uint8 (FK_* bits) and
# joint_gradient [B, J] (None unless asked for)
JointSphereChecks = collections.namedtuple("JointSphereChecks", SphereChecks._fields + ("fk_status", "joint_gradient"))


# what Context.solve_ik returns: one entry per problem; joints [B, J], error [B, 6], tip_pose [B, 16] column-major
IkSolutions = collections.namedtuple("IkSolutions", "joints status iterations error tip_pose fk_status")


def _task_weights(task_weights):
    if task_weights is None:
        return None
    weights = np.ascontiguousarray(task_weights, dtype=np.float64)
    if weights.shape != (6,):
        raise ValueError("task_weights must hold six values")
    return weights


# what Context.check_motions returns: one entry per motion; min_gradient [E, 3]
MotionChecks = collections.namedtuple(
    "MotionChecks", "status first_collision min_clearance min_sample min_sphere min_gradient fk_status")


# what Context.clearance_cost returns: one entry per configuration; joint_gradient [B, J]
ClearanceCosts = collections.namedtuple(
    "ClearanceCosts", "cost joint_gradient num_active num_outside num_without_gradient fk_status")


# what Context.check_self_collision returns: one entry per configuration; min_direction [B, 3], joint_gradient [B, J],
# pair_clearance [B, P] (None unless asked for); fk_status is None in the poses form
SelfCollisionChecks = collections.namedtuple(
    "SelfCollisionChecks", "status num_below num_without_value min_clearance min_pair min_direction joint_gradient "
    "fk_status pair_clearance")


# what Context.check_motions_with_self returns: one entry per motion; min_gradient [E, 3]
MotionSelfChecks = collections.namedtuple(
    "MotionSelfChecks", "status first_collision collision_cause min_clearance min_sample min_sphere min_gradient "
    "self_min_clearance self_min_sample self_min_pair fk_status")


def _sphere_pairs(pairs):
    """[P, 2] int32"""
    return np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)


def _joint_values(tree, joint_values):
    """[B, J] float64 for the tree's J columns."""
    q = np.ascontiguousarray(joint_values, dtype=np.float64)
    if q.ndim != 2 or q.shape[1] != tree.num_joints:
        raise ValueError("joint_values must have the shape [B, %d]" % tree.num_joints)
    return q


def _base_transform(world_from_base):
    """16 float64 column-major, or None; a [4, 4] matrix is transposed to column-major."""
    if world_from_base is None:
        return None
    m = np.asarray(world_from_base, dtype=np.float64)
    if m.shape == (4, 4):
        m = m.T
    if m.size != 16:
        raise ValueError("world_from_base must hold 16 values")
    return np.ascontiguousarray(m).reshape(16)


def _joint_limits(tree, joint_limits):
    if joint_limits is None:
        return None
    limits = np.ascontiguousarray(joint_limits, dtype=np.float64)
    if limits.shape != (tree.num_joints, 2):
        raise ValueError("joint_limits must have the shape [%d, 2]" % tree.num_joints)
    return limits


def _sphere_model(spheres_xyzr, sphere_link, link_poses):
    """(xyzr [S, 4] float64, link [S] int32, poses [B, L, 16] float64) as the sphere-model calls take them; poses may
    come as [B, L, 4, 4] world_from_link matrices."""
    xyzr = np.ascontiguousarray(spheres_xyzr, dtype=np.float64).reshape(-1, 4)
    link = np.ascontiguousarray(sphere_link, dtype=np.int32).reshape(-1)
    if len(link) != len(xyzr):
        raise ValueError("sphere_link must hold one link per sphere")
    poses = np.asarray(link_poses, dtype=np.float64)
    if poses.ndim == 4:
        if poses.shape[2:] != (4, 4):
            raise ValueError("link_poses must have the shape [B, L, 16] or [B, L, 4, 4]")
        poses = poses.transpose(0, 1, 3, 2).reshape(poses.shape[0], poses.shape[1], 16)
    if poses.ndim != 3 or poses.shape[2] != 16:
        raise ValueError("link_poses must have the shape [B, L, 16] or [B, L, 4, 4]")
    return xyzr, link, np.ascontiguousarray(poses)


class VgtHipError(RuntimeError):
    """HIP / runtime failure reported by libvgt_hip (std::runtime_error in the C++ glue)."""


class VgtHipUnavailable(VgtHipError):
    """No usable device (helper->IsAvailable() == false in the C++ glue)."""


_TESTING_LIB = None
_ERRORS = threading.local()


def _bind(path, signatures):
    try:
        # One HIP runtime per process: if torch is around, let it load its bundled
        # libamdhip64 (same SONAME) first so the dynamic linker reuses it for us.
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is optional for the C ABI
        pass
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)

    def remember_error(result, func, args):
        # error messages are thread-local PER LIBRARY: fetch the message from the library that failed
        if isinstance(result, int) and result != 0:
            _ERRORS.message = lib.vgt_hip_last_error().decode("utf-8", "replace")
        return result

    for name, (restype, argtypes) in signatures.items():
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
        if restype is _int and name != "vgt_hip_abi_version":
            fn.errcheck = remember_error
    return lib


def load(testing=False):
    """Loads libvgt_hip.so (or, testing=True, libvgt_hip_testing.so) once.  Raises if it has not been built (no fallback)."""
    global _LIB, _TESTING_LIB
    if testing:
        if _TESTING_LIB is None:
            if not os.path.exists(TESTING_LIB_PATH):
                raise VgtHipError("libvgt_hip_testing.so is not built (%s); run `make -C voxelized_geometry_tools_amd/csrc`"
                                  % TESTING_LIB_PATH)
            _TESTING_LIB = _bind(TESTING_LIB_PATH, dict(SIGNATURES, **TESTING_SIGNATURES))
        return _TESTING_LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise VgtHipError(
            "libvgt_hip.so is not built (%s); run `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C voxelized_geometry_tools_amd/csrc`" % LIB_PATH)
    _LIB = _bind(LIB_PATH, SIGNATURES)
    return _LIB


def last_error():
    """Message of the last failed call of this thread (whichever of the two libraries it went to)."""
    message = getattr(_ERRORS, "message", None)
    return message if message is not None else load().vgt_hip_last_error().decode("utf-8", "replace")


def check(rc):
    if rc == 0:
        return
    msg = last_error()
    if rc == 1:
        raise ValueError(msg)
    if rc == 3:
        raise VgtHipUnavailable(msg)
    raise VgtHipError(msg)


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(ctypes.c_void_p)
    return ctypes.c_void_p(int(a))


def _topology_table(call, capacity=256):
    """Runs call(table, capacity, byref(count)) and once more with the reported size when the table was too small."""
    for _ in range(2):
        table = np.zeros(capacity, dtype=COMPONENT_TOPOLOGY)
        count = ctypes.c_uint32(0xffffffff)
        rc = call(table, capacity, ctypes.byref(count))
        if rc == 1 and count.value != 0xffffffff and count.value + 1 > capacity:
            capacity = count.value + 1
            continue
        check(rc)
        return table[:count.value + 1].copy()
    raise VgtHipError("the component count changed between two calls")


TRAVEL_OCCUPANCY, TRAVEL_SDF_ABOVE = 0, 1
TRAVEL_NO_CORNER_CUTTING = 1
TRAVEL_UNREACHED = 0xffffffff
TRAVEL_NO_LIMIT = 0xfffffffe
TRACE_OK, TRACE_UNREACHED, TRACE_TRUNCATED, TRACE_INVALID = 0, 1, 2, 3


def travel_cost_workspace_bytes(shape):
    """vgt_hip_travel_cost_workspace_bytes: 0 for an empty grid or one over the limits."""
    return int(load().vgt_hip_travel_cost_workspace_bytes(*[int(s) for s in shape]))


def _travel_sources(sources, source_costs):
    src = np.ascontiguousarray(np.asarray(sources, dtype=np.int32).reshape(-1))
    costs = None
    if source_costs is not None:
        costs = np.ascontiguousarray(np.asarray(source_costs, dtype=np.uint32).reshape(-1))
        if costs.size != src.size:
            raise ValueError("one initial cost per source")
    return src, costs


def _surface_mesh(call, with_cells):
    """Runs call(vertices, cells, vertex_capacity, triangles, triangle_capacity, byref(nv), byref(nt)) of a host-output
    surface extraction twice: to count, then to fetch into arrays of exactly the counts."""
    nv, nt = ctypes.c_int64(0), ctypes.c_int64(0)
    check(call(None, None, 0, None, 0, ctypes.byref(nv), ctypes.byref(nt)))
    vertices = np.empty((int(nv.value), 3), dtype=np.float64)
    triangles = np.empty((int(nt.value), 3), dtype=np.int32)
    cells = np.empty(int(nv.value), dtype=np.int32) if with_cells else None
    if nv.value:
        check(call(vertices, cells, len(vertices), triangles, len(triangles), ctypes.byref(nv), ctypes.byref(nt)))
    return (vertices, triangles, cells) if with_cells else (vertices, triangles)


def mesh_grid_for(vertices, resolution):
    """vgt_hip_mesh_grid_for: ((nx, ny, nz), origin xyz float64[3]) of the map RasterizeMeshIntoOccupancyMap builds for
    these vertices.  Pure host code, no device needed."""
    v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    counts = (_i64 * 3)()
    origin = np.zeros(3, dtype=np.float64)
    check(load().vgt_hip_mesh_grid_for(_ptr(v), len(v), float(resolution), ctypes.byref(counts, 0),
                                       ctypes.byref(counts, 8), ctypes.byref(counts, 16), _ptr(origin)))
    return (int(counts[0]), int(counts[1]), int(counts[2])), origin


def _mesh_transforms(world_from_grid, grid_from_world):
    wfg = None if world_from_grid is None else np.ascontiguousarray(world_from_grid, dtype=np.float64).reshape(16)
    gfw = None if grid_from_world is None else np.ascontiguousarray(grid_from_world, dtype=np.float64).reshape(16)
    return wfg, gfw


def device_count():
    n = _int(0)
    check(load().vgt_hip_device_count(ctypes.byref(n)))
    return n.value


def device_name(device):
    buf = ctypes.create_string_buffer(256)
    check(load().vgt_hip_device_name(device, buf, 256))
    return buf.value.decode()


class Context:
    """One device + one stream (vgt_hip_ctx)."""

    def __init__(self, device=0, threads_per_block=-1, testing=False):
        """testing=True: a context of libvgt_hip_testing.so (set_edt_variant, debug_finalize_check,
        set_host_pipeline_min_voxels exist there only)."""
        self._lib = load(testing)
        self.testing = bool(testing)
        h = _p()
        check(self._lib.vgt_hip_create(device, threads_per_block, ctypes.byref(h)))
        self.handle = h
        self._children = weakref.WeakSet()   # grids / filter grids / cell grids created from this context

    def _adopt(self, child):
        self._children.add(child)

    def close(self):
        """Destroys the context after the handles created from it (the library also tolerates the
        other order: it keeps the context record alive until its last handle is destroyed)."""
        if getattr(self, "handle", None):
            for child in list(self._children):
                child.close()
            self._lib.vgt_hip_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def sdf_estimate_distance(self, sdf, resolution, queries, grid_from_world=None):
        """EstimateLocationDistance for a batch of query points [N, 3] -> (distance [N] float64, has_value [N] bool)."""
        field = np.ascontiguousarray(sdf, dtype=np.float32)
        q = np.ascontiguousarray(queries, dtype=np.float64).reshape(-1, 3)
        xf = None if grid_from_world is None else np.ascontiguousarray(grid_from_world, dtype=np.float64).reshape(16)
        out = np.empty(len(q), dtype=np.float64)
        has = np.empty(len(q), dtype=np.uint8)
        check(self._lib.vgt_hip_sdf_estimate_distance(self.handle, _ptr(field), *field.shape, float(resolution), _ptr(xf),
                                                      _ptr(q), len(q), _ptr(out), _ptr(has)))
        return out, has.astype(bool)

    def sdf_fine_gradient(self, sdf, resolution, queries, window, grid_from_world=None):
        """GetLocationFineGradient for a batch of query points [N, 3] -> (gradient [N, 3] float64, has_value [N] bool)."""
        field = np.ascontiguousarray(sdf, dtype=np.float32)
        q = np.ascontiguousarray(queries, dtype=np.float64).reshape(-1, 3)
        xf = None if grid_from_world is None else np.ascontiguousarray(grid_from_world, dtype=np.float64).reshape(16)
        out = np.empty((len(q), 3), dtype=np.float64)
        has = np.empty(len(q), dtype=np.uint8)
        check(self._lib.vgt_hip_sdf_fine_gradient(self.handle, _ptr(field), *field.shape, float(resolution), _ptr(xf),
                                                  _ptr(q), len(q), float(window), _ptr(out), _ptr(has)))
        return out, has.astype(bool)

    def sdf_project_out_of_collision(self, sdf, resolution, queries, minimum_distance=0.0, stepsize_multiplier=0.1,
                                     max_iterations=0, grid_from_world=None, rotation=None):
        """ProjectLocationOutOfCollisionToMinimumDistance for a batch of query points [N, 3] -> (position [N, 3] float64,
        has_value [N] bool, status [N] uint8 (PROJECT_*), iterations [N] int32); max_iterations=0: the library's limit."""
        field = np.ascontiguousarray(sdf, dtype=np.float32)
        q = np.ascontiguousarray(queries, dtype=np.float64).reshape(-1, 3)
        xf = None if grid_from_world is None else np.ascontiguousarray(grid_from_world, dtype=np.float64).reshape(16)
        rot = None if rotation is None else np.ascontiguousarray(rotation, dtype=np.float64).reshape(9)
        position = np.empty((len(q), 3), dtype=np.float64)
        has = np.empty(len(q), dtype=np.uint8)
        status = np.empty(len(q), dtype=np.uint8)
        iterations = np.empty(len(q), dtype=np.int32)
        check(self._lib.vgt_hip_sdf_project_out_of_collision(
            self.handle, _ptr(field), *field.shape, float(resolution), _ptr(xf), _ptr(rot), _ptr(q), len(q),
            float(minimum_distance), float(stepsize_multiplier), int(max_iterations), _ptr(position), _ptr(has),
            _ptr(status), _ptr(iterations)))
        return position, has.astype(bool), status, iterations

    def sdf_project_out_of_collision_dev(self, sdf_ptr, shape, resolution, queries_ptr, num_queries, position_ptr,
                                         has_value_ptr=None, status_ptr=None, iterations_ptr=None, minimum_distance=0.0,
                                         stepsize_multiplier=0.1, max_iterations=0, grid_from_world=None, rotation=None):
        """vgt_hip_sdf_project_out_of_collision_dev: field, queries and outputs on the device (the transforms are host
        arrays); enqueued on the context's stream."""
        xf = None if grid_from_world is None else np.ascontiguousarray(grid_from_world, dtype=np.float64).reshape(16)
        rot = None if rotation is None else np.ascontiguousarray(rotation, dtype=np.float64).reshape(9)
        check(self._lib.vgt_hip_sdf_project_out_of_collision_dev(
            self.handle, _ptr(sdf_ptr), *[int(c) for c in shape], float(resolution), _ptr(xf), _ptr(rot),
            _ptr(queries_ptr), int(num_queries), float(minimum_distance), float(stepsize_multiplier),
            int(max_iterations), _ptr(position_ptr), _ptr(has_value_ptr), _ptr(status_ptr), _ptr(iterations_ptr)))

    def cast_segments(self, field, resolution, segments, mode=SEGMENT_OCCUPANCY, unknown_is_filled=True, threshold=0.0,
                      walk_through=False, grid_from_world=None, with_min=False):
        """vgt_hip_cast_segments: segments [N, 6] (a, b) through an occupancy map (SEGMENT_OCCUPANCY) or an SDF
        (SEGMENT_SDF_BELOW, hit = value <= threshold) -> SegmentCasts(status uint8 (SEGMENT_*), hit_index int32,
        hit_fraction float64, cells_examined int32, min_value float32, min_index int32); the last two only with_min."""
        f = np.ascontiguousarray(field, dtype=np.float32)
        seg = np.ascontiguousarray(segments, dtype=np.float64).reshape(-1, 6)
        xf = None if grid_from_world is None else np.ascontiguousarray(grid_from_world, dtype=np.float64).reshape(16)
        n = len(seg)
        status = np.empty(n, dtype=np.uint8)
        hit_index = np.empty(n, dtype=np.int32)
        hit_fraction = np.empty(n, dtype=np.float64)
        cells_examined = np.empty(n, dtype=np.int32)
        min_value = np.empty(n, dtype=np.float32) if with_min else None
        min_index = np.empty(n, dtype=np.int32) if with_min else None
        check(self._lib.vgt_hip_cast_segments(
            self.handle, _ptr(f), *f.shape, float(resolution), int(mode), int(bool(unknown_is_filled)), float(threshold),
            SEGMENT_WALK_THROUGH if walk_through else 0, _ptr(xf), _ptr(seg), n, _ptr(status), _ptr(hit_index),
            _ptr(hit_fraction), _ptr(cells_examined), _ptr(min_value), _ptr(min_index)))
        return SegmentCasts(status, hit_index, hit_fraction, cells_examined, min_value, min_index)

    def cast_segments_dev(self, field_ptr, shape, resolution, segments_ptr, num_segments, status_ptr, hit_index_ptr=None,
                          hit_fraction_ptr=None, cells_examined_ptr=None, min_value_ptr=None, min_index_ptr=None,
                          mode=SEGMENT_OCCUPANCY, unknown_is_filled=True, threshold=0.0, walk_through=False,
                          grid_from_world=None):
        """vgt_hip_cast_segments_dev: field, segments and outputs on the device (the transform is a host array);
        enqueued on the context's stream."""
        xf = None if grid_from_world is None else np.ascontiguousarray(grid_from_world, dtype=np.float64).reshape(16)
        check(self._lib.vgt_hip_cast_segments_dev(
            self.handle, _ptr(field_ptr), *[int(c) for c in shape], float(resolution), int(mode),
            int(bool(unknown_is_filled)), float(threshold), SEGMENT_WALK_THROUGH if walk_through else 0, _ptr(xf),
            _ptr(segments_ptr), int(num_segments), _ptr(status_ptr), _ptr(hit_index_ptr), _ptr(hit_fraction_ptr),
            _ptr(cells_examined_ptr), _ptr(min_value_ptr), _ptr(min_index_ptr)))

    def check_spheres(self, sdf, resolution, spheres_xyzr, sphere_link, link_poses, minimum_clearance=0.0,
                      outside_is_collision=False, per_sphere=False, grid_from_world=None, rotation=None):
        """vgt_hip_check_spheres: a model of S spheres (spheres_xyzr [S, 4]: centre in the link's frame and radius;
        sphere_link [S]) in B configurations, link_poses [B, L, 16] (column-major world_from_link) or [B, L, 4, 4]
        (world_from_link matrices, transposed to column-major here) -> SphereChecks(status uint8 (SPHERES_*),
        min_clearance float64, min_sphere int32, num_below int32, num_outside int32, min_gradient [B, 3] float64,
        sphere_clearance [B, S], sphere_gradient [B, S, 3]); the last two only per_sphere."""
        f = np.ascontiguousarray(sdf, dtype=np.float32)
        xyzr = np.ascontiguousarray(spheres_xyzr, dtype=np.float64).reshape(-1, 4)
        link = np.ascontiguousarray(sphere_link, dtype=np.int32).reshape(-1)
        if len(link) != len(xyzr):
            raise ValueError("sphere_link must hold one link per sphere")
        poses = np.asarray(link_poses, dtype=np.float64)
        if poses.ndim == 4:
            if poses.shape[2:] != (4, 4):
                raise ValueError("link_poses must have the shape [B, L, 16] or [B, L, 4, 4]")
            poses = poses.transpose(0, 1, 3, 2).reshape(poses.shape[0], poses.shape[1], 16)
        if poses.ndim != 3 or poses.shape[2] != 16:
            raise ValueError("link_poses must have the shape [B, L, 16] or [B, L, 4, 4]")
        poses = np.ascontiguousarray(poses)
        b, links, s = poses.shape[0], poses.shape[1], len(xyzr)
        xf = None if grid_from_world is None else np.ascontiguousarray(grid_from_world, dtype=np.float64).reshape(16)
        rot = None if rotation is None else np.ascontiguousarray(rotation, dtype=np.float64).reshape(9)
        out = SphereChecks(np.empty(b, np.uint8), np.empty(b, np.float64), np.empty(b, np.int32), np.empty(b, np.int32),
                           np.empty(b, np.int32), np.empty((b, 3), np.float64),
                           np.empty((b, s), np.float64) if per_sphere else None,
                           np.empty((b, s, 3), np.float64) if per_sphere else None)
        check(self._lib.vgt_hip_check_spheres(
            self.handle, _ptr(f), *f.shape, float(resolution), _ptr(xf), _ptr(rot), _ptr(xyzr), _ptr(link), s, _ptr(poses),
            links, b, float(minimum_clearance), SPHERES_OUTSIDE_IS_COLLISION if outside_is_collision else 0,
            *[_ptr(a) for a in out]))
        return out

    def check_spheres_dev(self, sdf_ptr, shape, resolution, spheres_xyzr_ptr, sphere_link_ptr, num_spheres,
                          link_poses_ptr, num_links, num_configurations, status_ptr, min_clearance_ptr=None,
                          min_sphere_ptr=None, num_below_ptr=None, num_outside_ptr=None, min_gradient_ptr=None,
                          sphere_clearance_ptr=None, sphere_gradient_ptr=None, minimum_clearance=0.0,
                          outside_is_collision=False, grid_from_world=None, rotation=None):
        """vgt_hip_check_spheres_dev: field, model, poses and outputs on the device (the transforms are host arrays);
        enqueued on the context's stream."""
        xf = None if grid_from_world is None else np.ascontiguousarray(grid_from_world, dtype=np.float64).reshape(16)
        rot = None if rotation is None else np.ascontiguousarray(rotation, dtype=np.float64).reshape(9)
        check(self._lib.vgt_hip_check_spheres_dev(
            self.handle, _ptr(sdf_ptr), *[int(c) for c in shape], float(resolution), _ptr(xf), _ptr(rot),
            _ptr(spheres_xyzr_ptr), _ptr(sphere_link_ptr), int(num_spheres), _ptr(link_poses_ptr), int(num_links),
            int(num_configurations), float(minimum_clearance), SPHERES_OUTSIDE_IS_COLLISION if outside_is_collision else 0,
            _ptr(status_ptr), _ptr(min_clearance_ptr), _ptr(min_sphere_ptr), _ptr(num_below_ptr), _ptr(num_outside_ptr),
            _ptr(min_gradient_ptr), _ptr(sphere_clearance_ptr), _ptr(sphere_gradient_ptr)))

    def kinematics(self, parent, joint_type, joint_index, axis, origin, num_joints=None):
        """vgt_hip_kinematics_create: a tree of L links from parent [L], joint_type [L] (JOINT_*), joint_index [L],
        axis [L, 3] and origin [L, 16] (column-major parent_from_joint) or [L, 4, 4] (matrices, transposed here).
        num_joints: the number of columns of the joint values; by default 1 + the largest joint_index of a link that is
        not fixed.  Returns a KinematicTree (close() destroys it)."""
        return KinematicTree(self, parent, joint_type, joint_index, axis, origin, num_joints)

    def forward_kinematics(self, tree, joint_values, world_from_base=None, joint_limits=None):
        """vgt_hip_forward_kinematics: joint_values [B, J] -> (link_poses [B, L, 16] float64 column-major, as the
        sphere-model calls take them, status [B] uint8 of FK_* bits).  world_from_base: 16 doubles column-major or a
        [4, 4] matrix; joint_limits [J, 2]."""
        q = _joint_values(tree, joint_values)
        b = q.shape[0]
        poses = np.empty((b, tree.num_links, 16), np.float64)
        status = np.empty(b, np.uint8)
        check(self._lib.vgt_hip_forward_kinematics(self.handle, tree._handle_or_raise(), _ptr(q), b,
                                                   _ptr(_base_transform(world_from_base)),
                                                   _ptr(_joint_limits(tree, joint_limits)), _ptr(poses), _ptr(status)))
        return poses, status

    def forward_kinematics_dev(self, tree, joint_values_ptr, num_configurations, link_poses_ptr, status_ptr=None,
                               world_from_base=None, joint_limits=None):
        """vgt_hip_forward_kinematics_dev: joint values, poses and status on the device (the base transform and the
        limits are host arrays); enqueued on the context's stream."""
        check(self._lib.vgt_hip_forward_kinematics_dev(
            self.handle, tree._handle_or_raise(), _ptr(joint_values_ptr), int(num_configurations),
            _ptr(_base_transform(world_from_base)), _ptr(_joint_limits(tree, joint_limits)), _ptr(link_poses_ptr),
            _ptr(status_ptr)))

    def clearance_joint_gradient(self, tree, link_poses, spheres_xyzr, sphere_link, min_sphere=None, min_gradient=None,
                                 sphere_weight=None, sphere_gradient=None):
        """vgt_hip_clearance_joint_gradient: what check_spheres returned, mapped to joint space -> joint_gradient [B, J].
        Exactly one pair: (min_sphere [B], min_gradient [B, 3]) or (sphere_weight [B, S], sphere_gradient [B, S, 3])."""
        xyzr, link, poses = _sphere_model(spheres_xyzr, sphere_link, link_poses)
        if poses.shape[1] != tree.num_links:
            raise ValueError("link_poses must hold the tree's %d links per configuration" % tree.num_links)
        b, s = poses.shape[0], len(xyzr)
        ms = None if min_sphere is None else np.ascontiguousarray(min_sphere, dtype=np.int32).reshape(-1)
        mg = None if min_gradient is None else np.ascontiguousarray(min_gradient, dtype=np.float64).reshape(-1, 3)
        sw = None if sphere_weight is None else np.ascontiguousarray(sphere_weight, dtype=np.float64).reshape(-1, s)
        sg = None if sphere_gradient is None else np.ascontiguousarray(sphere_gradient, dtype=np.float64).reshape(-1, s, 3)
        for a in (ms, mg, sw, sg):
            if a is not None and len(a) != b:
                raise ValueError("one entry per configuration")
        out = np.empty((b, tree.num_joints), np.float64)
        check(self._lib.vgt_hip_clearance_joint_gradient(
            self.handle, tree._handle_or_raise(), _ptr(poses), b, _ptr(xyzr), _ptr(link), s, _ptr(ms), _ptr(mg), _ptr(sw),
            _ptr(sg), _ptr(out)))
        return out

    def clearance_joint_gradient_dev(self, tree, link_poses_ptr, num_configurations, spheres_xyzr_ptr, sphere_link_ptr,
                                     num_spheres, joint_gradient_ptr, min_sphere_ptr=None, min_gradient_ptr=None,
                                     sphere_weight_ptr=None, sphere_gradient_ptr=None):
        """vgt_hip_clearance_joint_gradient_dev: every array on the device; enqueued on the context's stream."""
        check(self._lib.vgt_hip_clearance_joint_gradient_dev(
            self.handle, tree._handle_or_raise(), _ptr(link_poses_ptr), int(num_configurations), _ptr(spheres_xyzr_ptr),
            _ptr(sphere_link_ptr), int(num_spheres), _ptr(min_sphere_ptr), _ptr(min_gradient_ptr),
            _ptr(sphere_weight_ptr), _ptr(sphere_gradient_ptr), _ptr(joint_gradient_ptr)))

    def solve_ik(self, tree, tip_link, targets, seeds, seeds_per_target=1, world_from_base=None, joint_limits=None,
                 task_weights=None, max_iterations=50, damping=0.01, max_step=0.5, position_tolerance=1e-6,
                 rotation_tolerance=1e-6):
        """vgt_hip_solve_ik: targets [T, 16] column-major world_from_tip (or [T, 4, 4] matrices, transposed here) and
        seeds [T * seeds_per_target, J] -> IkSolutions(joints [B, J], status uint8 (IK_*), iterations int32, error
        [B, 6], tip_pose [B, 16], fk_status uint8 (FK_* bits)): up to max_iterations damped least-squares steps per
        problem that bring link tip_link to its target (0: the seeds are evaluated only).  task_weights: six values for
        (x, y, z, rx, ry, rz), None = all 1."""
        aim = _cloud_poses(targets)
        q = _joint_values(tree, seeds)
        b = q.shape[0]
        if b != len(aim) * int(seeds_per_target):
            raise ValueError("seeds must hold seeds_per_target rows per target")
        out = IkSolutions(np.empty((b, tree.num_joints), np.float64), np.empty(b, np.uint8), np.empty(b, np.int32),
                          np.empty((b, 6), np.float64), np.empty((b, 16), np.float64), np.empty(b, np.uint8))
        check(self._lib.vgt_hip_solve_ik(
            self.handle, tree._handle_or_raise(), int(tip_link), _ptr(aim), len(aim), int(seeds_per_target), _ptr(q),
            _ptr(_base_transform(world_from_base)), _ptr(_joint_limits(tree, joint_limits)),
            _ptr(_task_weights(task_weights)), int(max_iterations), float(damping), float(max_step),
            float(position_tolerance), float(rotation_tolerance), *[_ptr(a) for a in out]))
        return out

    def solve_ik_dev(self, tree, tip_link, targets_ptr, num_targets, seeds_ptr, status_ptr, joints_out_ptr=None,
                     iterations_ptr=None, error_ptr=None, tip_pose_ptr=None, fk_status_ptr=None, workspace_ptr=None,
                     workspace_bytes=0, seeds_per_target=1, world_from_base=None, joint_limits=None, task_weights=None,
                     max_iterations=50, damping=0.01, max_step=0.5, position_tolerance=1e-6, rotation_tolerance=1e-6):
        """vgt_hip_solve_ik_dev: targets, seeds and outputs on the device (the base transform, the limits and the
        weights are host arrays); joints_out_ptr may be seeds_ptr, and only without it does the call need the workspace
        (solve_ik_workspace_bytes); enqueued on the context's stream."""
        check(self._lib.vgt_hip_solve_ik_dev(
            self.handle, tree._handle_or_raise(), int(tip_link), _ptr(targets_ptr), int(num_targets),
            int(seeds_per_target), _ptr(seeds_ptr), _ptr(_base_transform(world_from_base)),
            _ptr(_joint_limits(tree, joint_limits)), _ptr(_task_weights(task_weights)), int(max_iterations),
            float(damping), float(max_step), float(position_tolerance), float(rotation_tolerance), _ptr(joints_out_ptr),
            _ptr(status_ptr), _ptr(iterations_ptr), _ptr(error_ptr), _ptr(tip_pose_ptr), _ptr(fk_status_ptr),
            _ptr(workspace_ptr), int(workspace_bytes)))

    def check_spheres_from_joints(self, sdf, resolution, spheres_xyzr, sphere_link, tree, joint_values,
                                  minimum_clearance=0.0, outside_is_collision=False, per_sphere=False,
                                  grid_from_world=None, rotation=None, world_from_base=None, joint_limits=None,
                                  joint_gradient=False):
        """vgt_hip_check_spheres_from_joints: joint values in, the sphere-model check out.  One call uploads the field,
        the model and joint_values [B, J] and runs the forward kinematics, the check and -- joint_gradient=True -- the
        worst-sphere joint gradient on the device; the poses never visit the host.  Returns JointSphereChecks: the
        fields of SphereChecks, fk_status [B] uint8 and joint_gradient [B, J] (None unless asked for)."""
        f = np.ascontiguousarray(sdf, dtype=np.float32)
        if f.ndim != 3:
            raise ValueError("sdf must be an (nx, ny, nz) grid")
        xyzr = np.ascontiguousarray(spheres_xyzr, dtype=np.float64).reshape(-1, 4)
        link = np.ascontiguousarray(sphere_link, dtype=np.int32).reshape(-1)
        if len(link) != len(xyzr):
            raise ValueError("sphere_link must hold one link per sphere")
        q = _joint_values(tree, joint_values)
        b, s = q.shape[0], len(xyzr)
        xf = None if grid_from_world is None else np.ascontiguousarray(grid_from_world, dtype=np.float64).reshape(16)
        rot = None if rotation is None else np.ascontiguousarray(rotation, dtype=np.float64).reshape(9)
        out = JointSphereChecks(np.empty(b, np.uint8), np.empty(b, np.float64), np.empty(b, np.int32),
                                np.empty(b, np.int32), np.empty(b, np.int32), np.empty((b, 3), np.float64),
                                np.empty((b, s), np.float64) if per_sphere else None,
                                np.empty((b, s, 3), np.float64) if per_sphere else None, np.empty(b, np.uint8),
                                np.empty((b, tree.num_joints), np.float64) if joint_gradient else None)
        check(self._lib.vgt_hip_check_spheres_from_joints(
            self.handle, _ptr(f), *f.shape, float(resolution), _ptr(xf), _ptr(rot), _ptr(xyzr), _ptr(link), s,
            tree._handle_or_raise(), _ptr(q), b, _ptr(_base_transform(world_from_base)),
            _ptr(_joint_limits(tree, joint_limits)), float(minimum_clearance),
            SPHERES_OUTSIDE_IS_COLLISION if outside_is_collision else 0, *[_ptr(a) for a in out]))
        return out

    def check_motions(self, sdf, resolution, spheres_xyzr, sphere_link, tree, joint_from, joint_to, num_steps,
                      minimum_clearance=0.0, outside_is_collision=False, stop_at_collision=False, grid_from_world=None,
                      rotation=None, world_from_base=None, joint_limits=None):
        """vgt_hip_check_motions: E straight joint-space motions joint_from [E, J] -> joint_to [E, J] of num_steps steps
        each (an int for all of them, or an int32 array [E]; a motion has num_steps + 1 samples), every sample checked
        as check_spheres_from_joints checks a configuration; the poses never leave the device.  Returns
        MotionChecks(status uint8 (MOTION_*), first_collision int32, min_clearance float64, min_sample int32,
        min_sphere int32, min_gradient [E, 3] float64, fk_status uint8 (FK_* bits))."""
        f = np.ascontiguousarray(sdf, dtype=np.float32)
        if f.ndim != 3:
            raise ValueError("sdf must be an (nx, ny, nz) grid")
        xyzr = np.ascontiguousarray(spheres_xyzr, dtype=np.float64).reshape(-1, 4)
        link = np.ascontiguousarray(sphere_link, dtype=np.int32).reshape(-1)
        if len(link) != len(xyzr):
            raise ValueError("sphere_link must hold one link per sphere")
        a, b = _joint_values(tree, joint_from), _joint_values(tree, joint_to)
        if a.shape != b.shape:
            raise ValueError("joint_from and joint_to must have the same shape")
        e, s = a.shape[0], len(xyzr)
        if np.ndim(num_steps) == 0:
            steps, uniform = None, int(num_steps)
        else:
            steps, uniform = np.ascontiguousarray(num_steps, dtype=np.int32).reshape(-1), 0
            if len(steps) != e:
                raise ValueError("num_steps must hold one count per motion")
        xf = None if grid_from_world is None else np.ascontiguousarray(grid_from_world, dtype=np.float64).reshape(16)
        rot = None if rotation is None else np.ascontiguousarray(rotation, dtype=np.float64).reshape(9)
        out = MotionChecks(np.empty(e, np.uint8), np.empty(e, np.int32), np.empty(e, np.float64), np.empty(e, np.int32),
                           np.empty(e, np.int32), np.empty((e, 3), np.float64), np.empty(e, np.uint8))
        flags = (SPHERES_OUTSIDE_IS_COLLISION if outside_is_collision else 0) | \
            (MOTION_STOP_AT_COLLISION if stop_at_collision else 0)
        check(self._lib.vgt_hip_check_motions(
            self.handle, _ptr(f), *f.shape, float(resolution), _ptr(xf), _ptr(rot), _ptr(xyzr), _ptr(link), s,
            tree._handle_or_raise(), _ptr(a), _ptr(b), _ptr(steps), uniform, e, _ptr(_base_transform(world_from_base)),
            _ptr(_joint_limits(tree, joint_limits)), float(minimum_clearance), flags, *[_ptr(o) for o in out]))
        return out

    def check_motions_dev(self, sdf_ptr, shape, resolution, spheres_xyzr_ptr, sphere_link_ptr, num_spheres, tree,
                          joint_from_ptr, joint_to_ptr, num_steps, num_motions, status_ptr, first_collision_ptr=None,
                          min_clearance_ptr=None, min_sample_ptr=None, min_sphere_ptr=None, min_gradient_ptr=None,
                          fk_status_ptr=None, minimum_clearance=0.0, outside_is_collision=False,
                          stop_at_collision=False, grid_from_world=None, rotation=None, world_from_base=None,
                          joint_limits=None, num_steps_ptr=None):
        """vgt_hip_check_motions_dev: field, model, joint arrays and outputs on the device (the transforms and the limits
        are host arrays); num_steps: the step count of every motion, unless num_steps_ptr gives an int32 array [E] on
        the device; enqueued on the context's stream."""
        xf = None if grid_from_world is None else np.ascontiguousarray(grid_from_world, dtype=np.float64).reshape(16)
        rot = None if rotation is None else np.ascontiguousarray(rotation, dtype=np.float64).reshape(9)
        flags = (SPHERES_OUTSIDE_IS_COLLISION if outside_is_collision else 0) | \
            (MOTION_STOP_AT_COLLISION if stop_at_collision else 0)
        check(self._lib.vgt_hip_check_motions_dev(
            self.handle, _ptr(sdf_ptr), *[int(c) for c in shape], float(resolution), _ptr(xf), _ptr(rot),
            _ptr(spheres_xyzr_ptr), _ptr(sphere_link_ptr), int(num_spheres), tree._handle_or_raise(),
            _ptr(joint_from_ptr), _ptr(joint_to_ptr), _ptr(num_steps_ptr), int(num_steps or 0), int(num_motions),
            _ptr(_base_transform(world_from_base)), _ptr(_joint_limits(tree, joint_limits)), float(minimum_clearance),
            flags, _ptr(status_ptr), _ptr(first_collision_ptr), _ptr(min_clearance_ptr), _ptr(min_sample_ptr),
            _ptr(min_sphere_ptr), _ptr(min_gradient_ptr), _ptr(fk_status_ptr)))

    @staticmethod
    def _motion_self_flags(outside_is_collision, stop_at_collision, self_no_value_is_collision):
        return (SPHERES_OUTSIDE_IS_COLLISION if outside_is_collision else 0) | \
            (MOTION_STOP_AT_COLLISION if stop_at_collision else 0) | \
            (MOTION_SELF_NO_VALUE_IS_COLLISION if self_no_value_is_collision else 0)

    def check_motions_with_self(self, sdf, resolution, spheres_xyzr, sphere_link, pairs, tree, joint_from, joint_to,
                                num_steps, minimum_clearance=0.0, self_minimum_clearance=0.0,
                                outside_is_collision=False, stop_at_collision=False, self_no_value_is_collision=False,
                                grid_from_world=None, rotation=None, world_from_base=None, joint_limits=None):
        """vgt_hip_check_motions_with_self: check_motions' motions, every sample checked against the field (sdf, or None
        for no environment part) as check_spheres_from_joints checks a configuration and against the robot itself over
        the sphere pairs `pairs` [P, 2] (None or empty for no self part) as check_self_collision does; poses and centres
        are made once per sample and never leave the device.  Returns MotionSelfChecks(status uint8 (MOTION_*),
        first_collision int32, collision_cause uint8 (MOTION_CAUSE_* bits), min_clearance float64, min_sample int32,
        min_sphere int32, min_gradient [E, 3] float64, self_min_clearance float64, self_min_sample int32, self_min_pair
        int32, fk_status uint8 (FK_* bits))."""
        f = None if sdf is None else np.ascontiguousarray(sdf, dtype=np.float32)
        if f is not None and f.ndim != 3:
            raise ValueError("sdf must be an (nx, ny, nz) grid")
        shape = (0, 0, 0) if f is None else f.shape
        xyzr = np.ascontiguousarray(spheres_xyzr, dtype=np.float64).reshape(-1, 4)
        link = np.ascontiguousarray(sphere_link, dtype=np.int32).reshape(-1)
        if len(link) != len(xyzr):
            raise ValueError("sphere_link must hold one link per sphere")
        ab = _sphere_pairs(np.zeros((0, 2), np.int32) if pairs is None else pairs)
        a, b = _joint_values(tree, joint_from), _joint_values(tree, joint_to)
        if a.shape != b.shape:
            raise ValueError("joint_from and joint_to must have the same shape")
        e, s = a.shape[0], len(xyzr)
        if np.ndim(num_steps) == 0:
            steps, uniform = None, int(num_steps)
        else:
            steps, uniform = np.ascontiguousarray(num_steps, dtype=np.int32).reshape(-1), 0
            if len(steps) != e:
                raise ValueError("num_steps must hold one count per motion")
        xf = None if grid_from_world is None else np.ascontiguousarray(grid_from_world, dtype=np.float64).reshape(16)
        rot = None if rotation is None else np.ascontiguousarray(rotation, dtype=np.float64).reshape(9)
        out = MotionSelfChecks(np.empty(e, np.uint8), np.empty(e, np.int32), np.empty(e, np.uint8),
                               np.empty(e, np.float64), np.empty(e, np.int32), np.empty(e, np.int32),
                               np.empty((e, 3), np.float64), np.empty(e, np.float64), np.empty(e, np.int32),
                               np.empty(e, np.int32), np.empty(e, np.uint8))
        flags = self._motion_self_flags(outside_is_collision, stop_at_collision, self_no_value_is_collision)
        check(self._lib.vgt_hip_check_motions_with_self(
            self.handle, _ptr(f), *shape, float(resolution), _ptr(xf), _ptr(rot), _ptr(xyzr), _ptr(link), s, _ptr(ab),
            len(ab), tree._handle_or_raise(), _ptr(a), _ptr(b), _ptr(steps), uniform, e,
            _ptr(_base_transform(world_from_base)), _ptr(_joint_limits(tree, joint_limits)), float(minimum_clearance),
            float(self_minimum_clearance), flags, *[_ptr(o) for o in out]))
        return out

    def check_motions_with_self_dev(self, sdf_ptr, shape, resolution, spheres_xyzr_ptr, sphere_link_ptr, num_spheres,
                                    pairs_ptr, num_pairs, tree, joint_from_ptr, joint_to_ptr, num_steps, num_motions,
                                    status_ptr, first_collision_ptr=None, collision_cause_ptr=None,
                                    min_clearance_ptr=None, min_sample_ptr=None, min_sphere_ptr=None,
                                    min_gradient_ptr=None, self_min_clearance_ptr=None, self_min_sample_ptr=None,
                                    self_min_pair_ptr=None, fk_status_ptr=None, minimum_clearance=0.0,
                                    self_minimum_clearance=0.0, outside_is_collision=False, stop_at_collision=False,
                                    self_no_value_is_collision=False, grid_from_world=None, rotation=None,
                                    world_from_base=None, joint_limits=None, num_steps_ptr=None):
        """vgt_hip_check_motions_with_self_dev: field (or None, with shape (0, 0, 0)), model, pairs, joint arrays and
        outputs on the device (the transforms and the limits are host arrays); num_steps: the step count of every motion,
        unless num_steps_ptr gives an int32 array [E] on the device; enqueued on the context's stream."""
        xf = None if grid_from_world is None else np.ascontiguousarray(grid_from_world, dtype=np.float64).reshape(16)
        rot = None if rotation is None else np.ascontiguousarray(rotation, dtype=np.float64).reshape(9)
        flags = self._motion_self_flags(outside_is_collision, stop_at_collision, self_no_value_is_collision)
        check(self._lib.vgt_hip_check_motions_with_self_dev(
            self.handle, _ptr(sdf_ptr), *[int(c) for c in shape], float(resolution), _ptr(xf), _ptr(rot),
            _ptr(spheres_xyzr_ptr), _ptr(sphere_link_ptr), int(num_spheres), _ptr(pairs_ptr), int(num_pairs),
            tree._handle_or_raise(), _ptr(joint_from_ptr), _ptr(joint_to_ptr), _ptr(num_steps_ptr), int(num_steps or 0),
            int(num_motions), _ptr(_base_transform(world_from_base)), _ptr(_joint_limits(tree, joint_limits)),
            float(minimum_clearance), float(self_minimum_clearance), flags, _ptr(status_ptr), _ptr(first_collision_ptr),
            _ptr(collision_cause_ptr), _ptr(min_clearance_ptr), _ptr(min_sample_ptr), _ptr(min_sphere_ptr),
            _ptr(min_gradient_ptr), _ptr(self_min_clearance_ptr), _ptr(self_min_sample_ptr), _ptr(self_min_pair_ptr),
            _ptr(fk_status_ptr)))

    def clearance_cost(self, sdf, resolution, spheres_xyzr, sphere_link, tree, joint_values, margin, grid_from_world=None,
                       rotation=None, world_from_base=None, joint_limits=None, with_gradient=True):
        """vgt_hip_clearance_cost: the obstacle cost of B configurations joint_values [B, J] -- the hinge of `margin` on
        the clearance of every sphere, summed -- and its gradient with respect to the joints; poses and per-sphere values
        never leave the device.  Returns ClearanceCosts(cost float64, joint_gradient [B, J] float64 (None without
        with_gradient: then no gradient is loaded), num_active int32, num_outside int32, num_without_gradient int32
        (None without with_gradient), fk_status uint8 (FK_* bits))."""
        f = np.ascontiguousarray(sdf, dtype=np.float32)
        if f.ndim != 3:
            raise ValueError("sdf must be an (nx, ny, nz) grid")
        xyzr = np.ascontiguousarray(spheres_xyzr, dtype=np.float64).reshape(-1, 4)
        link = np.ascontiguousarray(sphere_link, dtype=np.int32).reshape(-1)
        if len(link) != len(xyzr):
            raise ValueError("sphere_link must hold one link per sphere")
        q = _joint_values(tree, joint_values)
        b, s = q.shape[0], len(xyzr)
        xf = None if grid_from_world is None else np.ascontiguousarray(grid_from_world, dtype=np.float64).reshape(16)
        rot = None if rotation is None else np.ascontiguousarray(rotation, dtype=np.float64).reshape(9)
        out = ClearanceCosts(np.empty(b, np.float64), np.empty((b, q.shape[1]), np.float64) if with_gradient else None,
                             np.empty(b, np.int32), np.empty(b, np.int32),
                             np.empty(b, np.int32) if with_gradient else None, np.empty(b, np.uint8))
        check(self._lib.vgt_hip_clearance_cost(
            self.handle, _ptr(f), *f.shape, float(resolution), _ptr(xf), _ptr(rot), _ptr(xyzr), _ptr(link), s,
            tree._handle_or_raise(), _ptr(q), b, _ptr(_base_transform(world_from_base)),
            _ptr(_joint_limits(tree, joint_limits)), float(margin), 0, *[_ptr(o) for o in out]))
        return out

    def clearance_cost_dev(self, sdf_ptr, shape, resolution, spheres_xyzr_ptr, sphere_link_ptr, num_spheres, tree,
                           joint_values_ptr, num_configurations, margin, cost_ptr, joint_gradient_ptr=None,
                           num_active_ptr=None, num_outside_ptr=None, num_without_gradient_ptr=None, fk_status_ptr=None,
                           grid_from_world=None, rotation=None, world_from_base=None, joint_limits=None, flags=0):
        """vgt_hip_clearance_cost_dev: field, model, joint values and outputs on the device (the transforms and the limits
        are host arrays); enqueued on the context's stream.  Without joint_gradient_ptr and num_without_gradient_ptr the
        cost-only kernel runs."""
        xf = None if grid_from_world is None else np.ascontiguousarray(grid_from_world, dtype=np.float64).reshape(16)
        rot = None if rotation is None else np.ascontiguousarray(rotation, dtype=np.float64).reshape(9)
        check(self._lib.vgt_hip_clearance_cost_dev(
            self.handle, _ptr(sdf_ptr), *[int(c) for c in shape], float(resolution), _ptr(xf), _ptr(rot),
            _ptr(spheres_xyzr_ptr), _ptr(sphere_link_ptr), int(num_spheres), tree._handle_or_raise(),
            _ptr(joint_values_ptr), int(num_configurations), _ptr(_base_transform(world_from_base)),
            _ptr(_joint_limits(tree, joint_limits)), float(margin), int(flags), _ptr(cost_ptr), _ptr(joint_gradient_ptr),
            _ptr(num_active_ptr), _ptr(num_outside_ptr), _ptr(num_without_gradient_ptr), _ptr(fk_status_ptr)))

    def check_self_collision(self, spheres_xyzr, sphere_link, pairs, tree, joint_values, minimum_clearance=0.0,
                             no_value_is_collision=False, per_pair=False, with_gradient=True, world_from_base=None,
                             joint_limits=None):
        """vgt_hip_check_self_collision: the sphere pairs `pairs` [P, 2] (a < b; self_collision_pairs makes a list) of a
        model in the B configurations joint_values [B, J]; poses and centres never leave the device.  Returns
        SelfCollisionChecks(status uint8 (SELF_*), num_below int32, num_without_value int32, min_clearance float64,
        min_pair int32 (-1: none), min_direction [B, 3] float64, joint_gradient [B, J] float64 (None without
        with_gradient), fk_status uint8 (FK_* bits), pair_clearance [B, P] float64 (None without per_pair))."""
        xyzr = np.ascontiguousarray(spheres_xyzr, dtype=np.float64).reshape(-1, 4)
        link = np.ascontiguousarray(sphere_link, dtype=np.int32).reshape(-1)
        if len(link) != len(xyzr):
            raise ValueError("sphere_link must hold one link per sphere")
        ab = _sphere_pairs(pairs)
        q = _joint_values(tree, joint_values)
        b = q.shape[0]
        out = SelfCollisionChecks(np.empty(b, np.uint8), np.empty(b, np.int32), np.empty(b, np.int32),
                                  np.empty(b, np.float64), np.empty(b, np.int32), np.empty((b, 3), np.float64),
                                  np.empty((b, q.shape[1]), np.float64) if with_gradient else None,
                                  np.empty(b, np.uint8), np.empty((b, len(ab)), np.float64) if per_pair else None)
        flags = SELF_NO_VALUE_IS_COLLISION if no_value_is_collision else 0
        check(self._lib.vgt_hip_check_self_collision(
            self.handle, _ptr(xyzr), _ptr(link), len(xyzr), _ptr(ab), len(ab), tree._handle_or_raise(), _ptr(q), b,
            _ptr(_base_transform(world_from_base)), _ptr(_joint_limits(tree, joint_limits)), float(minimum_clearance),
            flags, *[_ptr(o) for o in out]))
        return out

    def check_self_collision_dev(self, spheres_xyzr_ptr, sphere_link_ptr, num_spheres, pairs_ptr, num_pairs, tree,
                                 joint_values_ptr, num_configurations, status_ptr, minimum_clearance=0.0,
                                 num_below_ptr=None, num_without_value_ptr=None, min_clearance_ptr=None,
                                 min_pair_ptr=None, min_direction_ptr=None, joint_gradient_ptr=None, fk_status_ptr=None,
                                 pair_clearance_ptr=None, world_from_base=None, joint_limits=None, flags=0):
        """vgt_hip_check_self_collision_dev: model, pairs, joint values and outputs on the device (the base transform and
        the limits are host arrays); enqueued on the context's stream."""
        check(self._lib.vgt_hip_check_self_collision_dev(
            self.handle, _ptr(spheres_xyzr_ptr), _ptr(sphere_link_ptr), int(num_spheres), _ptr(pairs_ptr),
            int(num_pairs), tree._handle_or_raise(), _ptr(joint_values_ptr), int(num_configurations),
            _ptr(_base_transform(world_from_base)), _ptr(_joint_limits(tree, joint_limits)), float(minimum_clearance),
            int(flags), _ptr(status_ptr), _ptr(num_below_ptr), _ptr(num_without_value_ptr), _ptr(min_clearance_ptr),
            _ptr(min_pair_ptr), _ptr(min_direction_ptr), _ptr(joint_gradient_ptr), _ptr(fk_status_ptr),
            _ptr(pair_clearance_ptr)))

    def check_self_collision_poses(self, spheres_xyzr, sphere_link, pairs, link_poses, tree=None, minimum_clearance=0.0,
                                   no_value_is_collision=False, per_pair=False):
        """vgt_hip_check_self_collision_poses: the same from link_poses [B, L, 16] (as check_spheres takes them); the
        joint gradient only with a tree (of L links).  fk_status is None."""
        xyzr = np.ascontiguousarray(spheres_xyzr, dtype=np.float64).reshape(-1, 4)
        link = np.ascontiguousarray(sphere_link, dtype=np.int32).reshape(-1)
        if len(link) != len(xyzr):
            raise ValueError("sphere_link must hold one link per sphere")
        ab = _sphere_pairs(pairs)
        poses = np.ascontiguousarray(link_poses, dtype=np.float64)
        if poses.ndim != 3 or poses.shape[2] != 16:
            raise ValueError("link_poses must be [B, L, 16]")
        b, links = poses.shape[0], poses.shape[1]
        joints = tree.num_joints if tree is not None else 0
        out = SelfCollisionChecks(np.empty(b, np.uint8), np.empty(b, np.int32), np.empty(b, np.int32),
                                  np.empty(b, np.float64), np.empty(b, np.int32), np.empty((b, 3), np.float64),
                                  np.empty((b, joints), np.float64) if tree is not None else None, None,
                                  np.empty((b, len(ab)), np.float64) if per_pair else None)
        flags = SELF_NO_VALUE_IS_COLLISION if no_value_is_collision else 0
        check(self._lib.vgt_hip_check_self_collision_poses(
            self.handle, _ptr(xyzr), _ptr(link), len(xyzr), _ptr(ab), len(ab), _ptr(poses), b, links,
            tree._handle_or_raise() if tree is not None else None, float(minimum_clearance), flags,
            *[_ptr(o) for i, o in enumerate(out) if i != 7]))
        return out

    def check_self_collision_poses_dev(self, spheres_xyzr_ptr, sphere_link_ptr, num_spheres, pairs_ptr, num_pairs,
                                       link_poses_ptr, num_configurations, num_links, status_ptr, tree=None,
                                       minimum_clearance=0.0, num_below_ptr=None, num_without_value_ptr=None,
                                       min_clearance_ptr=None, min_pair_ptr=None, min_direction_ptr=None,
                                       joint_gradient_ptr=None, pair_clearance_ptr=None, flags=0):
        """vgt_hip_check_self_collision_poses_dev: everything on the device; enqueued on the context's stream."""
        check(self._lib.vgt_hip_check_self_collision_poses_dev(
            self.handle, _ptr(spheres_xyzr_ptr), _ptr(sphere_link_ptr), int(num_spheres), _ptr(pairs_ptr),
            int(num_pairs), _ptr(link_poses_ptr), int(num_configurations), int(num_links),
            tree._handle_or_raise() if tree is not None else None, float(minimum_clearance), int(flags),
            _ptr(status_ptr), _ptr(num_below_ptr), _ptr(num_without_value_ptr), _ptr(min_clearance_ptr),
            _ptr(min_pair_ptr), _ptr(min_direction_ptr), _ptr(joint_gradient_ptr), _ptr(pair_clearance_ptr)))

    def rasterize_spheres(self, shape, resolution, spheres_xyzr, sphere_link, link_poses, padding=0.0, base=0, into=None,
                          grid_from_world=None):
        """vgt_hip_rasterize_spheres: the cells of a grid of `shape` that the model's spheres (as for check_spheres;
        radius + padding) cover in B configurations -> first_configuration int32 of `shape`: base + the least b that
        covers the cell, -1 where none does.  into: an int32 array of `shape` that is kept (VGT_HIP_SPHERES_KEEP) and
        lowered in place as an unsigned minimum -- the result of an earlier call, for a motion given in pieces."""
        xyzr, link, poses = _sphere_model(spheres_xyzr, sphere_link, link_poses)
        shape = tuple(int(c) for c in shape)
        if len(shape) != 3:
            raise ValueError("shape must be (nx, ny, nz)")
        xf = None if grid_from_world is None else np.ascontiguousarray(grid_from_world, dtype=np.float64).reshape(16)
        if into is None:
            out = np.empty(tuple(max(c, 0) for c in shape), np.int32)
        else:
            out = into
            if not (isinstance(out, np.ndarray) and out.dtype == np.int32 and out.flags.c_contiguous and
                    out.flags.writeable and out.shape == shape):
                raise ValueError("into must be a writeable C-contiguous int32 array of the grid's shape")
        check(self._lib.vgt_hip_rasterize_spheres(
            self.handle, *shape, float(resolution), _ptr(xf), _ptr(xyzr), _ptr(link), len(xyzr), _ptr(poses),
            poses.shape[1], poses.shape[0], float(padding), int(base), SPHERES_KEEP if into is not None else 0,
            _ptr(out)))
        return out

    def rasterize_spheres_dev(self, shape, resolution, spheres_xyzr_ptr, sphere_link_ptr, num_spheres, link_poses_ptr,
                              num_links, num_configurations, first_configuration_ptr, padding=0.0, base=0, keep=False,
                              grid_from_world=None):
        """vgt_hip_rasterize_spheres_dev: model, poses and the int32 output on the device (the transform is a host
        array); enqueued on the context's stream."""
        xf = None if grid_from_world is None else np.ascontiguousarray(grid_from_world, dtype=np.float64).reshape(16)
        check(self._lib.vgt_hip_rasterize_spheres_dev(
            self.handle, *[int(c) for c in shape], float(resolution), _ptr(xf), _ptr(spheres_xyzr_ptr),
            _ptr(sphere_link_ptr), int(num_spheres), _ptr(link_poses_ptr), int(num_links), int(num_configurations),
            float(padding), int(base), SPHERES_KEEP if keep else 0, _ptr(first_configuration_ptr)))

    def spheres_cover_points(self, points, spheres_xyzr, sphere_link, link_poses, padding=0.0, world_from_points=None,
                             filtered=False):
        """vgt_hip_spheres_cover_points: points [N, 3] float32 (under world_from_points, 16 doubles column-major or 4 x 4
        transposed by the caller) against the model in B configurations -> PointCover(first_configuration int32,
        first_sphere int32, filtered): the least (b, s) that covers each point or (-1, -1); filtered=True also gives
        the cloud with the covered points set to NaN, which the raycast entry points skip."""
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        xyzr, link, poses = _sphere_model(spheres_xyzr, sphere_link, link_poses)
        xf = None if world_from_points is None else np.ascontiguousarray(world_from_points, dtype=np.float64).reshape(16)
        n = len(pts)
        out = PointCover(np.empty(n, np.int32), np.empty(n, np.int32), np.empty((n, 3), np.float32) if filtered else None)
        check(self._lib.vgt_hip_spheres_cover_points(
            self.handle, _ptr(pts), n, _ptr(xf), _ptr(xyzr), _ptr(link), len(xyzr), _ptr(poses), poses.shape[1],
            poses.shape[0], float(padding), 0, *[_ptr(a) for a in out]))
        return out

    def spheres_cover_points_dev(self, points_ptr, num_points, spheres_xyzr_ptr, sphere_link_ptr, num_spheres,
                                 link_poses_ptr, num_links, num_configurations, first_configuration_ptr=None,
                                 first_sphere_ptr=None, filtered_ptr=None, padding=0.0, world_from_points=None):
        """vgt_hip_spheres_cover_points_dev: cloud, model, poses and outputs on the device (the transform is a host
        array; filtered_ptr may be points_ptr); enqueued on the context's stream."""
        xf = None if world_from_points is None else np.ascontiguousarray(world_from_points, dtype=np.float64).reshape(16)
        check(self._lib.vgt_hip_spheres_cover_points_dev(
            self.handle, _ptr(points_ptr), int(num_points), _ptr(xf), _ptr(spheres_xyzr_ptr), _ptr(sphere_link_ptr),
            int(num_spheres), _ptr(link_poses_ptr), int(num_links), int(num_configurations), float(padding), 0,
            _ptr(first_configuration_ptr), _ptr(first_sphere_ptr), _ptr(filtered_ptr)))

    def align_points(self, sdf, resolution, points, poses, max_iterations=10, min_points=6, damping=0.0,
                     max_residual=float("inf"), target_distance=0.0, translation_tolerance=0.0, rotation_tolerance=0.0,
                     pivot=None, grid_from_world=None, rotation=None):
        """vgt_hip_align_points: a cloud [N, 3] float32 under B pose hypotheses (poses [B, 16] column-major
        world_from_points, or [B, 4, 4] matrices, transposed here) against an SDF: each pose scored and refined by up to
        max_iterations damped Gauss-Newton steps (0: scored only) -> CloudAlignment(poses [B, 16], status uint8
        (ALIGN_*), num_used, num_outside, num_rejected int32, sum_squared float64, evaluations int32, normal_equations
        [B, 27], last_step [B, 6]).  pivot: 3 doubles in the poses' frame (None: the origin)."""
        f = np.ascontiguousarray(sdf, dtype=np.float32)
        if f.ndim != 3:
            raise ValueError("sdf must be (nx, ny, nz)")
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        start = _cloud_poses(poses)
        b = len(start)
        xf = None if grid_from_world is None else np.ascontiguousarray(grid_from_world, dtype=np.float64).reshape(16)
        rot = None if rotation is None else np.ascontiguousarray(rotation, dtype=np.float64).reshape(9)
        about = None if pivot is None else np.ascontiguousarray(pivot, dtype=np.float64).reshape(3)
        out = CloudAlignment(np.empty((b, 16), np.float64), np.empty(b, np.uint8), np.empty(b, np.int32),
                             np.empty(b, np.int32), np.empty(b, np.int32), np.empty(b, np.float64),
                             np.empty(b, np.int32), np.empty((b, 27), np.float64), np.empty((b, 6), np.float64))
        check(self._lib.vgt_hip_align_points(
            self.handle, _ptr(f), *f.shape, float(resolution), _ptr(xf), _ptr(rot), _ptr(pts), len(pts), _ptr(start), b,
            _ptr(about), int(max_iterations), int(min_points), float(damping), float(max_residual),
            float(target_distance), float(translation_tolerance), float(rotation_tolerance), *[_ptr(a) for a in out]))
        return out

    def align_points_dev(self, sdf_ptr, shape, resolution, points_ptr, num_points, poses_ptr, num_poses, status_ptr,
                         workspace_ptr, workspace_bytes, poses_out_ptr=None, num_used_ptr=None, num_outside_ptr=None,
                         num_rejected_ptr=None, sum_squared_ptr=None, evaluations_ptr=None, normal_equations_ptr=None,
                         last_step_ptr=None, max_iterations=10, min_points=6, damping=0.0, max_residual=float("inf"),
                         target_distance=0.0, translation_tolerance=0.0, rotation_tolerance=0.0, pivot=None,
                         grid_from_world=None, rotation=None):
        """vgt_hip_align_points_dev: field, cloud, poses, outputs and the workspace (align_points_workspace_bytes) on
        the device, the transforms and the pivot host arrays; poses_out_ptr may be poses_ptr; enqueued on the context's
        stream."""
        xf = None if grid_from_world is None else np.ascontiguousarray(grid_from_world, dtype=np.float64).reshape(16)
        rot = None if rotation is None else np.ascontiguousarray(rotation, dtype=np.float64).reshape(9)
        about = None if pivot is None else np.ascontiguousarray(pivot, dtype=np.float64).reshape(3)
        check(self._lib.vgt_hip_align_points_dev(
            self.handle, _ptr(sdf_ptr), *[int(c) for c in shape], float(resolution), _ptr(xf), _ptr(rot),
            _ptr(points_ptr), int(num_points), _ptr(poses_ptr), int(num_poses), _ptr(about), int(max_iterations),
            int(min_points), float(damping), float(max_residual), float(target_distance), float(translation_tolerance),
            float(rotation_tolerance), _ptr(poses_out_ptr), _ptr(status_ptr), _ptr(num_used_ptr), _ptr(num_outside_ptr),
            _ptr(num_rejected_ptr), _ptr(sum_squared_ptr), _ptr(evaluations_ptr), _ptr(normal_equations_ptr),
            _ptr(last_step_ptr), _ptr(workspace_ptr), int(workspace_bytes)))

    def sdf_coarse_gradient_dev(self, sdf_ptr, shape, resolution, gradient_ptr, has_value_ptr=None,
                                enable_edge_gradients=False, rotation=None):
        """vgt_hip_sdf_coarse_gradient_dev: field and outputs (3 doubles and, optionally, a byte per voxel) on the
        device; enqueued on the context's stream."""
        rot = None if rotation is None else np.ascontiguousarray(rotation, dtype=np.float64).reshape(9)
        check(self._lib.vgt_hip_sdf_coarse_gradient_dev(
            self.handle, _ptr(sdf_ptr), *[int(c) for c in shape], float(resolution), int(bool(enable_edge_gradients)),
            _ptr(rot), _ptr(gradient_ptr), _ptr(has_value_ptr)))

    def sdf_estimate_distance_dev(self, sdf_ptr, shape, resolution, queries_ptr, num_queries, distance_ptr,
                                  has_value_ptr=None, grid_from_world=None):
        """vgt_hip_sdf_estimate_distance_dev: field, queries and outputs on the device (the transform is a host array);
        enqueued on the context's stream."""
        xf = None if grid_from_world is None else np.ascontiguousarray(grid_from_world, dtype=np.float64).reshape(16)
        check(self._lib.vgt_hip_sdf_estimate_distance_dev(
            self.handle, _ptr(sdf_ptr), *[int(c) for c in shape], float(resolution), _ptr(xf), _ptr(queries_ptr),
            int(num_queries), _ptr(distance_ptr), _ptr(has_value_ptr)))

    def sdf_local_extrema_map_dev(self, sdf_ptr, shape, resolution, extrema_ptr, rotation=None):
        """vgt_hip_sdf_local_extrema_map_dev: field and the 3 doubles per voxel on the device; runs on the context's
        stream and returns when it is done (its scratch goes with the call)."""
        rot = None if rotation is None else np.ascontiguousarray(rotation, dtype=np.float64).reshape(9)
        check(self._lib.vgt_hip_sdf_local_extrema_map_dev(
            self.handle, _ptr(sdf_ptr), *[int(c) for c in shape], float(resolution), _ptr(rot), _ptr(extrema_ptr)))

    def sdf_local_extrema_map(self, sdf, resolution, rotation=None):
        """ComputeLocalExtremaMap: [nx, ny, nz, 3] float64 (grid-frame extremum location per voxel, +inf = off the grid)."""
        field = np.ascontiguousarray(sdf, dtype=np.float32)
        rot = None if rotation is None else np.ascontiguousarray(rotation, dtype=np.float64).reshape(9)
        out = np.empty(field.shape + (3,), dtype=np.float64)
        check(self._lib.vgt_hip_sdf_local_extrema_map(self.handle, _ptr(field), *field.shape, float(resolution),
                                                      _ptr(rot), _ptr(out)))
        return out

    def connected_components(self, occupancy):
        """UpdateConnectedComponents of an occupancy grid: (uint32 labels of the grid's shape, number of components).
        Components are numbered from 1 in ascending order of the smallest linear index they contain."""
        occ = np.ascontiguousarray(occupancy, dtype=np.float32)
        if occ.ndim != 3:
            raise ValueError("occupancy must be (nx, ny, nz)")
        labels = np.empty(occ.shape, dtype=np.uint32)
        count = ctypes.c_uint32(0)
        check(self._lib.vgt_hip_connected_components(self.handle, _ptr(occ), *occ.shape, _ptr(labels),
                                                     ctypes.byref(count)))
        return labels, int(count.value)

    def connected_components_dev(self, occ_ptr, shape, labels_ptr):
        """vgt_hip_connected_components_dev: device buffers in and out -> number of components."""
        count = ctypes.c_uint32(0)
        check(self._lib.vgt_hip_connected_components_dev(self.handle, _ptr(occ_ptr), *[int(v) for v in shape],
                                                         _ptr(labels_ptr), ctypes.byref(count)))
        return int(count.value)

    def component_surface_mask(self, occupancy, labels, component_types):
        """Dense ExtractComponentSurfaces: bool array, True where the cell's class is selected by component_types
        (1 filled | 2 empty | 4 unknown) and the cell is a surface cell of its component."""
        occ = np.ascontiguousarray(occupancy, dtype=np.float32)
        lab = np.ascontiguousarray(labels, dtype=np.uint32)
        if occ.ndim != 3 or lab.shape != occ.shape:
            raise ValueError("occupancy and labels must be (nx, ny, nz) grids of one shape")
        mask = np.empty(occ.shape, dtype=np.uint8)
        check(self._lib.vgt_hip_component_surface_mask(self.handle, _ptr(occ), _ptr(lab), *occ.shape,
                                                       int(component_types), _ptr(mask)))
        return mask.astype(bool)

    def component_surface_mask_dev(self, occ_ptr, labels_ptr, shape, component_types, mask_ptr):
        check(self._lib.vgt_hip_component_surface_mask_dev(self.handle, _ptr(occ_ptr), _ptr(labels_ptr),
                                                           *[int(v) for v in shape], int(component_types),
                                                           _ptr(mask_ptr)))

    def select_cells(self, values, rule, class_mask, threshold=0.5, labels=None, with_values=False,
                     with_labels=False):
        """The cells of a float grid that `rule` (SELECT_*) selects among the classes of class_mask (CLASS_* against
        `threshold`), as int32 linear indices in ascending order; with_values / with_labels add float32 values and
        uint32 labels of those cells: indices, or (indices[, values][, labels]).  One call counts, a second one fetches."""
        val = np.ascontiguousarray(values, dtype=np.float32)
        lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.uint32)
        if val.ndim != 3 or (lab is not None and lab.shape != val.shape):
            raise ValueError("values and labels must be (nx, ny, nz) grids of one shape")
        count = ctypes.c_int64(0)

        def call(indices, vals, labs, capacity):
            check(self._lib.vgt_hip_select_cells(self.handle, _ptr(val), _ptr(lab), *val.shape, int(rule),
                                                 int(class_mask), float(threshold), _ptr(indices), _ptr(vals),
                                                 _ptr(labs), capacity, ctypes.byref(count)))

        call(None, None, None, 0)
        n = int(count.value)
        indices = np.empty(n, dtype=np.int32)
        vals = np.empty(n, dtype=np.float32) if with_values else None
        labs = np.empty(n, dtype=np.uint32) if with_labels else None
        if n:
            call(indices, vals, labs, n)
        out = (indices,) + ((vals,) if with_values else ()) + ((labs,) if with_labels else ())
        return out if len(out) > 1 else indices

    def select_cells_dev(self, values_ptr, shape, rule, class_mask, threshold=0.5, labels_ptr=None, indices_ptr=None,
                         values_out_ptr=None, labels_out_ptr=None, capacity=0):
        """vgt_hip_select_cells_dev: device buffers in and out -> the number of selected cells (indices_ptr=None with
        capacity=0 only counts)."""
        count = ctypes.c_int64(0)
        check(self._lib.vgt_hip_select_cells_dev(self.handle, _ptr(values_ptr), _ptr(labels_ptr),
                                                 *[int(v) for v in shape], int(rule), int(class_mask), float(threshold),
                                                 _ptr(indices_ptr), _ptr(values_out_ptr), _ptr(labels_out_ptr),
                                                 int(capacity), ctypes.byref(count)))
        return int(count.value)

    def cells_select(self, cells, rule, class_mask, payload_member=CELL_MEMBER_NONE, labels_ptr=None,
                     with_occupancy=False):
        """vgt_hip_cells_select on a Cells handle of this context: see Cells.select."""
        return cells.select(rule, class_mask, payload_member, labels_ptr, with_occupancy)

    def extract_surface(self, values, resolution, iso=0.0, inside_above=False, world_from_grid=None, with_cells=False):
        """vgt_hip_extract_surface: the iso-surface of a float grid as an indexed mesh (surface nets on the lattice of
        cell centres; include/vgt_hip.h states the rules) -> (vertices float64 [V, 3], triangles int32 [T, 3]) and, with
        with_cells=True, the int32 linear index [V] of each vertex's cube.  inside is v < iso, or v > iso with
        inside_above (occupancy: iso=0.5, inside_above=True).  world_from_grid: 16 doubles column-major, None = the grid
        frame.  One call counts, a second one fetches."""
        val = np.ascontiguousarray(values, dtype=np.float32)
        if val.ndim != 3:
            raise ValueError("values must be an (nx, ny, nz) grid")
        wfg, _ = _mesh_transforms(world_from_grid, None)

        def call(vertices, cells, vertex_capacity, triangles, triangle_capacity, nv, nt):
            return self._lib.vgt_hip_extract_surface(
                self.handle, _ptr(val), *val.shape, float(iso), int(bool(inside_above)), float(resolution), _ptr(wfg),
                _ptr(vertices), _ptr(cells), vertex_capacity, _ptr(triangles), triangle_capacity, nv, nt)

        return _surface_mesh(call, with_cells)

    def extract_surface_dev(self, values, resolution, iso=0.0, inside_above=False, world_from_grid=None,
                            with_cells=False, shape=None):
        """vgt_hip_extract_surface_dev: `values` is a float32 torch tensor (nx, ny, nz) on the context's device, or a
        device pointer with `shape`.  Returns torch tensors on that device, (vertices float64 [V, 3], triangles int32
        [T, 3][, cells int32 [V]]): valid inputs of rasterize_mesh_dev as they stand.  The field must be complete before
        the call (it runs on the context's stream); the mesh is complete when the call returns."""
        import torch
        device = "cuda:%d" % self._lib.vgt_hip_device_of(self.handle)
        if shape is None:
            if values.dtype != torch.float32 or values.dim() != 3 or not values.is_contiguous():
                raise ValueError("values must be a contiguous float32 (nx, ny, nz) tensor")
            shape, values_ptr = tuple(values.shape), values.data_ptr()
        else:
            values_ptr = values.data_ptr() if hasattr(values, "data_ptr") else values
        shape = [int(c) for c in shape]
        wfg, _ = _mesh_transforms(world_from_grid, None)
        nv, nt = ctypes.c_int64(0), ctypes.c_int64(0)

        def call(vertices, cells, vertex_capacity, triangles, triangle_capacity):
            check(self._lib.vgt_hip_extract_surface_dev(
                self.handle, _ptr(values_ptr), *shape, float(iso), int(bool(inside_above)), float(resolution), _ptr(wfg),
                _ptr(vertices), _ptr(cells), vertex_capacity, _ptr(triangles), triangle_capacity, ctypes.byref(nv),
                ctypes.byref(nt)))

        call(None, None, 0, None, 0)
        vertices = torch.empty((int(nv.value), 3), dtype=torch.float64, device=device)
        triangles = torch.empty((int(nt.value), 3), dtype=torch.int32, device=device)
        cells = torch.empty(int(nv.value), dtype=torch.int32, device=device) if with_cells else None
        if nv.value:
            torch.cuda.synchronize(device)  # (the buffers are torch's: nothing of its streams may still use them)
            call(vertices.data_ptr(), cells.data_ptr() if with_cells else None, len(vertices), triangles.data_ptr(),
                 len(triangles))
        return (vertices, triangles, cells) if with_cells else (vertices, triangles)

    def travel_cost(self, field, sources, weights=(10, 14, 17), mode=TRAVEL_OCCUPANCY, unknown_is_filled=True,
                    threshold=0.0, no_corner_cutting=False, source_costs=None, cost_limit=TRAVEL_NO_LIMIT,
                    with_toward=True):
        """vgt_hip_travel_cost: the least cost from the sources (linear indices) to every cell through passable cells
        (include/vgt_hip.h states the rules) -> (cost uint32 (nx, ny, nz), toward int32 or None, num_reached)."""
        f = np.ascontiguousarray(field, dtype=np.float32)
        if f.ndim != 3:
            raise ValueError("field must be an (nx, ny, nz) grid")
        src, costs = _travel_sources(sources, source_costs)
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.uint32).reshape(3))
        cost = np.empty(f.shape, dtype=np.uint32)
        toward = np.empty(f.shape, dtype=np.int32) if with_toward else None
        reached = ctypes.c_int64(0)
        check(self._lib.vgt_hip_travel_cost(
            self.handle, _ptr(f), *f.shape, int(mode), int(bool(unknown_is_filled)), float(threshold), _ptr(w),
            TRAVEL_NO_CORNER_CUTTING if no_corner_cutting else 0, _ptr(src), _ptr(costs), src.size, int(cost_limit),
            _ptr(cost), _ptr(toward), ctypes.byref(reached)))
        return cost, toward, int(reached.value)

    def travel_cost_dev(self, field_ptr, shape, sources_ptr, num_sources, cost_ptr, ws_ptr, ws_bytes, toward_ptr=None,
                        source_costs_ptr=None, weights=(10, 14, 17), mode=TRAVEL_OCCUPANCY, unknown_is_filled=True,
                        threshold=0.0, no_corner_cutting=False, cost_limit=TRAVEL_NO_LIMIT):
        """vgt_hip_travel_cost_dev: field, sources, outputs and workspace on the device -> num_reached.  Synchronises
        the context's stream; the outputs are complete when it returns."""
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.uint32).reshape(3))
        reached = ctypes.c_int64(0)
        check(self._lib.vgt_hip_travel_cost_dev(
            self.handle, _ptr(field_ptr), *[int(c) for c in shape], int(mode), int(bool(unknown_is_filled)),
            float(threshold), _ptr(w), TRAVEL_NO_CORNER_CUTTING if no_corner_cutting else 0, _ptr(sources_ptr),
            _ptr(source_costs_ptr), int(num_sources), int(cost_limit), _ptr(cost_ptr), _ptr(toward_ptr),
            ctypes.byref(reached), _ptr(ws_ptr), int(ws_bytes)))
        return int(reached.value)

    def trace_paths(self, toward, starts, max_cells, fill=-1):
        """vgt_hip_trace_paths: follows `toward` from every start -> (paths int32 [N, max_cells], pre-filled with `fill`
        beyond each length, lengths int32 [N], status uint8 [N] (TRACE_*))."""
        t = np.ascontiguousarray(toward, dtype=np.int32).reshape(-1)
        st = np.ascontiguousarray(np.asarray(starts, dtype=np.int32).reshape(-1))
        paths = np.full((st.size, max(int(max_cells), 0)), fill, dtype=np.int32)
        lengths = np.zeros(st.size, dtype=np.int32)
        status = np.zeros(st.size, dtype=np.uint8)
        check(self._lib.vgt_hip_trace_paths(self.handle, _ptr(t), t.size, _ptr(st), st.size, int(max_cells), _ptr(paths),
                                            _ptr(lengths), _ptr(status)))
        return paths, lengths, status

    def trace_paths_dev(self, toward_ptr, num_cells, starts_ptr, num_starts, max_cells, paths_ptr, lengths_ptr,
                        status_ptr):
        """vgt_hip_trace_paths_dev: everything on the device; enqueued on the context's stream."""
        check(self._lib.vgt_hip_trace_paths_dev(self.handle, _ptr(toward_ptr), int(num_cells), _ptr(starts_ptr),
                                                int(num_starts), int(max_cells), _ptr(paths_ptr), _ptr(lengths_ptr),
                                                _ptr(status_ptr)))

    def component_topology(self, occupancy, component_types, with_labels=False):
        """ComputeComponentTopology of an occupancy grid (it labels the grid first): a COMPONENT_TOPOLOGY array with one
        entry per label, [c] for component c, [0] and the components of classes not selected all zero.
        with_labels=True: (table, uint32 labels)."""
        occ = np.ascontiguousarray(occupancy, dtype=np.float32)
        if occ.ndim != 3:
            raise ValueError("occupancy must be (nx, ny, nz)")
        labels = np.empty(occ.shape, dtype=np.uint32) if with_labels else None
        table = _topology_table(
            lambda out, capacity, count: self._lib.vgt_hip_component_topology(
                self.handle, _ptr(occ), *occ.shape, int(component_types), _ptr(labels), count, _ptr(out), capacity))
        return (table, labels) if with_labels else table

    def component_topology_dev(self, occ_ptr, labels_ptr, shape, component_types, num_components):
        """vgt_hip_component_topology_dev: occupancy and labels on the device -> the table (host)."""
        table = np.zeros(int(num_components) + 1, dtype=COMPONENT_TOPOLOGY)
        check(self._lib.vgt_hip_component_topology_dev(self.handle, _ptr(occ_ptr), _ptr(labels_ptr),
                                                       *[int(v) for v in shape], int(component_types),
                                                       int(num_components), _ptr(table)))
        return table

    def rasterize_mesh(self, vertices, triangles, cells, resolution, world_from_grid=None, grid_from_world=None,
                       enforce_contains=False, rule=MESH_RULE_REFERENCE):
        """RasterizeMesh into a host map, in place: `cells` is a C-contiguous (nx, ny, nz) array of float32 or of
        8-byte records with the float occupancy first (OCCUPANCY_COMPONENT_CELL).  Transforms: 16 doubles column-major
        each, both or neither (None = the grid frame).  Returns `cells`."""
        v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
        t = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
        if not isinstance(cells, np.ndarray) or cells.ndim != 3 or not cells.flags.c_contiguous or \
                not cells.flags.writeable:
            raise ValueError("cells must be a writeable C-contiguous (nx, ny, nz) array")
        wfg, gfw = _mesh_transforms(world_from_grid, grid_from_world)
        check(self._lib.vgt_hip_rasterize_mesh(self.handle, _ptr(v), len(v), _ptr(t), len(t), _ptr(cells),
                                               cells.dtype.itemsize, *cells.shape, float(resolution), _ptr(wfg),
                                               _ptr(gfw), int(bool(enforce_contains)), int(rule)))
        return cells

    def rasterize_mesh_dev(self, vertices_ptr, num_vertices, triangles_ptr, num_triangles, cells_ptr, cell_bytes, shape,
                           resolution, world_from_grid=None, grid_from_world=None, enforce_contains=False,
                           rule=MESH_RULE_REFERENCE):
        """vgt_hip_rasterize_mesh_dev: vertices (float64), triangles (int32) and the map on the device, the map
        modified in place (the transforms are host arrays)."""
        wfg, gfw = _mesh_transforms(world_from_grid, grid_from_world)
        check(self._lib.vgt_hip_rasterize_mesh_dev(self.handle, _ptr(vertices_ptr), int(num_vertices),
                                                   _ptr(triangles_ptr), int(num_triangles), _ptr(cells_ptr),
                                                   int(cell_bytes), *[int(c) for c in shape], float(resolution),
                                                   _ptr(wfg), _ptr(gfw), int(bool(enforce_contains)), int(rule)))

    def fill_enclosed(self, cells, unknown_is_filled=True):
        """vgt_hip_fill_enclosed on a host map, in place: every passable cell that no chain of face-adjacent passable
        cells joins to the grid's border gets occupancy 1.0 (scipy.ndimage.binary_fill_holes, face connectivity).
        `cells` as for rasterize_mesh.  Returns the number of cells filled."""
        if not isinstance(cells, np.ndarray) or cells.ndim != 3 or not cells.flags.c_contiguous or \
                not cells.flags.writeable:
            raise ValueError("cells must be a writeable C-contiguous (nx, ny, nz) array")
        count = _i64(0)
        check(self._lib.vgt_hip_fill_enclosed(self.handle, _ptr(cells), cells.dtype.itemsize, *cells.shape,
                                              int(bool(unknown_is_filled)), ctypes.byref(count)))
        return int(count.value)

    def fill_enclosed_dev(self, cells_ptr, cell_bytes, shape, unknown_is_filled=True, want_count=True):
        """vgt_hip_fill_enclosed_dev: the map on the device, filled in place.  want_count=True waits and returns the
        number of cells filled; want_count=False leaves the work enqueued on the context's stream and returns None."""
        count = _i64(0)
        check(self._lib.vgt_hip_fill_enclosed_dev(self.handle, _ptr(cells_ptr), int(cell_bytes),
                                                  *[int(c) for c in shape], int(bool(unknown_is_filled)),
                                                  ctypes.byref(count) if want_count else None))
        return int(count.value) if want_count else None

    def mesh_sdf(self, vertices, triangles, resolution, rule=MESH_RULE_REFERENCE, unknown_is_filled=True,
                 add_virtual_border=False, with_occupancy=False, solid=False):
        """Mesh -> SDF: mesh_grid_for -> a zeroed device map -> rasterize_mesh_dev -> sdf_dev; the grid never visits the
        host in between.  Returns (sdf float32 (nx, ny, nz), minimum, maximum, origin xyz) -- the map's transform is the
        translation to `origin` -- and, with_occupancy=True, the rasterized occupancy as a fifth item.
        solid=True puts fill_enclosed_dev (no count, nothing waited for) between the two: the field is negative inside
        the body and the occupancy handed back is the filled one.  Only MESH_RULE_NEAREST guarantees a sealed shell for
        a closed mesh; under MESH_RULE_REFERENCE the interior is filled only where the shell happens to be sealed."""
        import torch
        v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
        t = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
        shape, origin = mesh_grid_for(v, resolution)
        wfg = np.eye(4)
        wfg[:3, 3] = origin
        gfw = np.eye(4)
        gfw[:3, 3] = -origin
        device = "cuda:%d" % self._lib.vgt_hip_device_of(self.handle)
        v_dev = torch.from_numpy(v).to(device)
        t_dev = torch.from_numpy(t).to(device)
        occ_dev = torch.zeros(shape, dtype=torch.float32, device=device)
        sdf_dev = torch.empty(shape, dtype=torch.float32, device=device)
        ws_bytes = sdf_workspace_bytes(shape)
        ws_dev = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
        minmax_dev = torch.empty(2, dtype=torch.float32, device=device)
        torch.cuda.synchronize(device)
        self.rasterize_mesh_dev(v_dev.data_ptr(), len(v), t_dev.data_ptr(), len(t), occ_dev.data_ptr(), 4, shape,
                                resolution, wfg.T.reshape(16), gfw.T.reshape(16), True, rule)
        if solid:
            self.fill_enclosed_dev(occ_dev.data_ptr(), 4, shape, unknown_is_filled, want_count=False)
        self.sdf_dev(occ_dev.data_ptr(), shape, resolution, sdf_dev.data_ptr(), ws_dev.data_ptr(), ws_bytes,
                     minmax_dev.data_ptr(), unknown_is_filled, add_virtual_border)
        self.synchronize()
        lo, hi = (float(x) for x in minmax_dev.cpu().numpy())
        out = (sdf_dev.cpu().numpy(), lo, hi, origin)
        return out + (occ_dev.cpu().numpy(),) if with_occupancy else out

    def trim(self):
        """Frees the device buffers the context caches between host-pointer calls."""
        check(self._lib.vgt_hip_trim(self.handle))

    def set_stream(self, stream_ptr):
        """Run on an external hipStream_t; 0 / None = HIP's legacy default stream (torch's default)."""
        check(self._lib.vgt_hip_set_stream(self.handle, _ptr(stream_ptr) if stream_ptr else None))

    def reset_stream(self):
        check(self._lib.vgt_hip_reset_stream(self.handle))

    def synchronize(self):
        check(self._lib.vgt_hip_synchronize(self.handle))

    def timing_start(self, max_calls):
        """Deferred per-kernel timing of the following SDF calls (no synchronisation until timing_stop)."""
        self._timing_capacity = int(max_calls)
        check(self._lib.vgt_hip_timing_start(self.handle, int(max_calls)))

    def timing_stop(self):
        """-> float32 array [calls, 3]: ms of (pass 1 [+ slab record fix-up], Y pass, X pass) per recorded call."""
        out = np.zeros((self._timing_capacity, 3), dtype=np.float32)
        n = ctypes.c_int32(0)
        check(self._lib.vgt_hip_timing_stop(self.handle, _ptr(out), ctypes.byref(n)))
        return out[:n.value].copy()

    def set_edt_variant(self, variant):
        """Testing library only: 0 default, 1 the cross-check pipeline (int16 Z scan + pruned search)."""
        if not self.testing:
            if int(variant) == 0:
                return
            raise VgtHipError("EDT variants other than 0 exist in libvgt_hip_testing.so only: Context(testing=True)")
        check(self._lib.vgt_hip_set_edt_variant(self.handle, int(variant)))

    def class_records(self, occ_ptr, shape, unknown_is_filled=True, z_offset=0, records_ptr=None, summary_ptr=None):
        """Testing library only: pass 1 alone (vgt_hip_testing_class_records_dev)."""
        nx, ny, nz = shape
        check(self._lib.vgt_hip_testing_class_records_dev(self.handle, _ptr(occ_ptr), nx, ny, nz,
                                                          int(bool(unknown_is_filled)), int(z_offset), _ptr(records_ptr),
                                                          _ptr(summary_ptr)))

    def set_short_line_rows(self, rows):
        """Testing library only: lines of at most `rows` rows take the short-line kernels whatever the item count
        (0 = sweeps everywhere, negative = back to the product's rule)."""
        check(self._lib.vgt_hip_testing_set_short_line_rows(int(rows)))

    def one_class_counts(self, workspace_ptr, shape):
        """Testing library only: (Z lines of one class, lines counted) of pass 1's sample in the last sdf_dev call with
        this workspace (waits for the stream)."""
        counts = (ctypes.c_uint32 * 2)()
        check(self._lib.vgt_hip_testing_one_class_counts(self.handle, _ptr(workspace_ptr), *[int(v) for v in shape],
                                                         ctypes.cast(counts, ctypes.c_void_p)))
        return int(counts[0]), int(counts[1])

    def set_sweep_slots(self, slots):
        """Testing library only (process-wide there): at most `slots` workgroups per sweep launch (0 = back to the
        product's 4096)."""
        check(self._lib.vgt_hip_testing_set_sweep_slots(int(slots)))

    def set_coarse_hull(self, mode):
        """Testing library only (process-wide there): the plain X pass's kernel on whole single grids -- 0 by scene (the
        product's rule), 1 the coarse-hull kernel wherever it applies, 2 never."""
        check(self._lib.vgt_hip_testing_set_coarse_hull(int(mode)))

    def x_pass_choice(self, workspace_ptr, shape):
        """Testing library only: which plain X kernel did the work of the last sdf_dev call with this workspace (waits for
        the stream): 0 neither, 1 plain, 2 coarse hull; + 4 when both were enqueued and the device chose."""
        choice = ctypes.c_int32(-1)
        check(self._lib.vgt_hip_testing_x_pass_choice(self.handle, _ptr(workspace_ptr), *[int(v) for v in shape],
                                                      ctypes.byref(choice)))
        return int(choice.value)

    def set_check_spheres_workgroups(self, workgroups):
        """Testing library only (process-wide there): at most `workgroups` workgroups per check_spheres launch (0 = back
        to the product's limit)."""
        check(self._lib.vgt_hip_testing_set_check_spheres_workgroups(int(workgroups)))

    def set_sphere_volume_workgroups(self, workgroups):
        """Testing library only (process-wide there): at most `workgroups` workgroups per rasterize_spheres and
        spheres_cover_points launch (0 = back to the product's limit)."""
        check(self._lib.vgt_hip_testing_set_sphere_volume_workgroups(int(workgroups)))

    def set_align_workgroups(self, workgroups):
        """Testing library only (process-wide there): at most `workgroups` workgroups per evaluation launch of
        align_points (0 = back to the product's limit)."""
        check(self._lib.vgt_hip_testing_set_align_workgroups(int(workgroups)))

    def set_kinematics_workgroups(self, workgroups):
        """Testing library only (process-wide there): at most `workgroups` workgroups per launch of forward_kinematics
        and clearance_joint_gradient (0 = back to the product's limit).  It caps the launch of solve_ik in the same
        way."""
        check(self._lib.vgt_hip_testing_set_kinematics_workgroups(int(workgroups)))

    def set_motion_workgroups(self, workgroups):
        """Testing library only (process-wide there): at most `workgroups` workgroups per launch of check_motions
        (0 = back to the product's limit)."""
        check(self._lib.vgt_hip_testing_set_motion_workgroups(int(workgroups)))

    def set_cost_workgroups(self, workgroups):
        """Testing library only (process-wide there): at most `workgroups` workgroups per launch of clearance_cost
        (0 = back to the product's limit)."""
        check(self._lib.vgt_hip_testing_set_cost_workgroups(int(workgroups)))

    def set_self_collision_workgroups(self, workgroups):
        """Testing library only (process-wide there): at most `workgroups` workgroups per launch of check_self_collision
        (0 = back to the product's limit)."""
        check(self._lib.vgt_hip_testing_set_self_collision_workgroups(int(workgroups)))

    def set_motion_self_workgroups(self, workgroups):
        """Testing library only (process-wide there): at most `workgroups` workgroups per launch of
        check_motions_with_self (0 = back to the product's limit)."""
        check(self._lib.vgt_hip_testing_set_motion_self_workgroups(int(workgroups)))

    def set_sphere_volume_counters(self, counters_ptr):
        """Testing library only (process-wide there): three uint64 on the device to which every rasterize_spheres launch
        adds its (cell, sphere) tests, those that covered and the atomics issued; None = back to the product's kernel."""
        check(self._lib.vgt_hip_testing_set_sphere_volume_counters(_ptr(counters_ptr)))

    def set_host_pipeline_min_voxels(self, min_voxels):
        """Testing library only (process-wide there): smallest grid the host-pointer SDF entry points pipeline."""
        check(self._lib.vgt_hip_testing_set_host_pipeline_min_voxels(int(min_voxels)))

    def debug_finalize_check(self, first_d2, count, resolution):
        """(mismatches, first mismatching d2 or None) of the fast vs exact final conversion."""
        bad = ctypes.c_uint64(0)
        first = ctypes.c_uint64(0)
        check(self._lib.vgt_hip_debug_finalize_check(self.handle, int(first_d2), int(count), float(resolution),
                                                     ctypes.byref(bad), ctypes.byref(first)))
        return int(bad.value), (None if first.value == 2 ** 64 - 1 else int(first.value))

    def sdf_coarse_gradient(self, sdf, resolution, enable_edge_gradients=False, rotation=None):
        """Grid-aligned (or rotated) coarse gradient of every voxel: (gradient [nx, ny, nz, 3] float64, has_value)."""
        field = np.ascontiguousarray(sdf, dtype=np.float32)
        nx, ny, nz = field.shape
        grad = np.empty((nx, ny, nz, 3), dtype=np.float64)
        has = np.empty((nx, ny, nz), dtype=np.uint8)
        rot = None if rotation is None else np.ascontiguousarray(rotation, dtype=np.float64).reshape(9)
        check(self._lib.vgt_hip_sdf_coarse_gradient(self.handle, _ptr(field), nx, ny, nz, float(resolution),
                                                    int(bool(enable_edge_gradients)), _ptr(rot), _ptr(grad),
                                                    _ptr(has)))
        return grad, has.astype(bool)

    def cells(self, records, shape, object_id_offset=4):
        """Uploads a grid of cell records (see Cells)."""
        return Cells(self, records, shape, object_id_offset)

    # ---- SDF ----
    def sdf_from_occupancy(self, occupancy, resolution, unknown_is_filled=True,
                           add_virtual_border=False, out=None):
        occ = np.ascontiguousarray(occupancy, dtype=np.float32)
        if occ.ndim != 3:
            raise ValueError("occupancy must be (nx, ny, nz)")
        nx, ny, nz = occ.shape
        if out is None:
            out = np.empty(occ.shape, dtype=np.float32)
        elif out.shape != occ.shape or out.dtype != np.float32 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous float32 array of the occupancy's shape")
        lo, hi = _f32(), _f32()
        check(self._lib.vgt_hip_sdf_from_occupancy_f32(
            self.handle, _ptr(occ), nx, ny, nz, float(resolution), int(bool(unknown_is_filled)),
            int(bool(add_virtual_border)), _ptr(out), ctypes.byref(lo), ctypes.byref(hi)))
        return out, lo.value, hi.value

    def sdf_batch_from_occupancy(self, grids, resolution, unknown_is_filled=True, add_virtual_border=False):
        """vgt_hip_sdf_batch_from_occupancy_f32: a list of equal-shape float32 grids (any addresses) ->
        (list of fields, mins, maxs) from one batched extraction."""
        grids = [np.ascontiguousarray(g, dtype=np.float32) for g in grids]
        if not grids or any(g.ndim != 3 or g.shape != grids[0].shape for g in grids):
            raise ValueError("a batch is a non-empty list of (nx, ny, nz) grids of one shape")
        nx, ny, nz = grids[0].shape
        outs = [np.empty(g.shape, dtype=np.float32) for g in grids]
        batch = len(grids)
        in_ptrs = (ctypes.c_void_p * batch)(*[g.ctypes.data for g in grids])
        out_ptrs = (ctypes.c_void_p * batch)(*[o.ctypes.data for o in outs])
        lo = np.zeros(batch, dtype=np.float32)
        hi = np.zeros(batch, dtype=np.float32)
        check(self._lib.vgt_hip_sdf_batch_from_occupancy_f32(
            self.handle, ctypes.cast(in_ptrs, ctypes.c_void_p), batch, nx, ny, nz, float(resolution),
            int(bool(unknown_is_filled)), int(bool(add_virtual_border)), ctypes.cast(out_ptrs, ctypes.c_void_p),
            _ptr(lo), _ptr(hi)))
        return outs, lo, hi

    def sdf_batch_dev(self, occ_ptr, batch, shape, resolution, sdf_ptr, ws_ptr, ws_bytes, minmax_ptr=None,
                      unknown_is_filled=True, add_virtual_border=False):
        """vgt_hip_sdf_batch_dev: [batch][nx][ny][nz] device buffers in and out."""
        nx, ny, nz = shape
        check(self._lib.vgt_hip_sdf_batch_dev(
            self.handle, _ptr(occ_ptr), int(batch), nx, ny, nz, float(resolution), int(bool(unknown_is_filled)),
            int(bool(add_virtual_border)), _ptr(sdf_ptr), _ptr(ws_ptr), ws_bytes, _ptr(minmax_ptr)))

    def sdf_from_mask(self, mask, resolution, add_virtual_border=False):
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        nx, ny, nz = m.shape
        out = np.empty(m.shape, dtype=np.float32)
        lo, hi = _f32(), _f32()
        check(self._lib.vgt_hip_sdf_from_mask_u8(
            self.handle, _ptr(m), nx, ny, nz, float(resolution), int(bool(add_virtual_border)),
            _ptr(out), ctypes.byref(lo), ctypes.byref(hi)))
        return out, lo.value, hi.value

    def sdf_dev(self, occ_ptr, shape, resolution, sdf_ptr, ws_ptr, ws_bytes, minmax_ptr=None,
                unknown_is_filled=True, add_virtual_border=False, kernel_ms=None):
        nx, ny, nz = shape
        if kernel_ms is None:
            check(self._lib.vgt_hip_sdf_dev(
                self.handle, _ptr(occ_ptr), nx, ny, nz, float(resolution),
                int(bool(unknown_is_filled)), int(bool(add_virtual_border)), _ptr(sdf_ptr),
                _ptr(ws_ptr), ws_bytes, _ptr(minmax_ptr)))
        else:
            check(self._lib.vgt_hip_sdf_dev_timed(
                self.handle, _ptr(occ_ptr), nx, ny, nz, float(resolution),
                int(bool(unknown_is_filled)), int(bool(add_virtual_border)), _ptr(sdf_ptr),
                _ptr(ws_ptr), ws_bytes, _ptr(minmax_ptr), _ptr(kernel_ms)))

    # ---- nearest cell of the other class (contract: include/vgt_hip.h, vgt_hip_nearest_dev) ----
    def nearest_from_occupancy(self, occupancy, unknown_is_filled=True, with_d2=False):
        """vgt_hip_nearest_from_occupancy_f32: int32 [nx, ny, nz] linear index of the nearest cell of the other class
        (-1: none), or (nearest, d2) with_d2 (int32 squared distance in cells, 0x7fffffff with -1)."""
        occ = np.ascontiguousarray(occupancy, dtype=np.float32)
        if occ.ndim != 3:
            raise ValueError("occupancy must be (nx, ny, nz)")
        nearest = np.empty(occ.shape, dtype=np.int32)
        d2 = np.empty(occ.shape, dtype=np.int32) if with_d2 else None
        check(self._lib.vgt_hip_nearest_from_occupancy_f32(
            self.handle, _ptr(occ), *occ.shape, int(bool(unknown_is_filled)), _ptr(nearest), _ptr(d2)))
        return (nearest, d2) if with_d2 else nearest

    def nearest_from_mask(self, mask, with_d2=False):
        """vgt_hip_nearest_from_mask_u8: as nearest_from_occupancy for one byte per cell, filled = non-zero."""
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        if m.ndim != 3:
            raise ValueError("mask must be (nx, ny, nz)")
        nearest = np.empty(m.shape, dtype=np.int32)
        d2 = np.empty(m.shape, dtype=np.int32) if with_d2 else None
        check(self._lib.vgt_hip_nearest_from_mask_u8(self.handle, _ptr(m), *m.shape, _ptr(nearest), _ptr(d2)))
        return (nearest, d2) if with_d2 else nearest

    def nearest_dev(self, occ_ptr, shape, nearest_ptr, ws_ptr, ws_bytes, d2_ptr=None, unknown_is_filled=True):
        """vgt_hip_nearest_dev: everything on the device, enqueued on the context's stream."""
        nx, ny, nz = (int(s) for s in shape)
        check(self._lib.vgt_hip_nearest_dev(self.handle, _ptr(occ_ptr), nx, ny, nz, int(bool(unknown_is_filled)),
                                            _ptr(nearest_ptr), _ptr(d2_ptr), _ptr(ws_ptr), int(ws_bytes)))

    # ---- multi-GPU Z slabs ----
    def sdf_slab_begin(self, occ_ptr, local_shape, z_offset, ws_ptr, ws_bytes, summary_ptr,
                       unknown_is_filled=True, kernel_ms=None):
        nx, ny, nz = local_shape
        check(self._lib.vgt_hip_sdf_slab_begin_dev(
            self.handle, _ptr(occ_ptr), nx, ny, nz, int(z_offset), int(bool(unknown_is_filled)),
            _ptr(ws_ptr), ws_bytes, _ptr(summary_ptr), _ptr(kernel_ms)))

    def sdf_slab_carries(self, gathered_ptr, world, rank, nx, ny, nz_global, carries_ptr):
        check(self._lib.vgt_hip_sdf_slab_carries_dev(self.handle, _ptr(gathered_ptr), int(world), int(rank),
                                                     int(nx), int(ny), int(nz_global), _ptr(carries_ptr)))

    def sdf_slab_finish(self, local_shape, z_offset, nz_global, resolution, carries_ptr, sdf_ptr,
                        ws_ptr, ws_bytes, minmax_ptr=None, add_virtual_border=False,
                        kernel_ms=None):
        nx, ny, nz = local_shape
        check(self._lib.vgt_hip_sdf_slab_finish_dev(
            self.handle, nx, ny, nz, int(z_offset), int(nz_global), float(resolution),
            int(bool(add_virtual_border)), _ptr(carries_ptr), _ptr(sdf_ptr), _ptr(ws_ptr), ws_bytes,
            _ptr(minmax_ptr), _ptr(kernel_ms)))

    # ---- voxelizer ----
    def tracking_grids(self, num_cells, num_grids):
        return TrackingGrids(self, num_cells, num_grids)

    def filter_grid(self, occupancy):
        return FilterGrid(self, occupancy)


def sdf_multi(devices, occupancy, resolution, unknown_is_filled=True, add_virtual_border=False, out=None):
    """vgt_hipx_sdf_multi: one process, one Z slab per entry of `devices` (a device may repeat)."""
    lib = load()
    occ = np.ascontiguousarray(occupancy, dtype=np.float32)
    if occ.ndim != 3:
        raise ValueError("occupancy must be (nx, ny, nz)")
    nx, ny, nz = occ.shape
    devs = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
    if out is None:
        out = np.empty(occ.shape, dtype=np.float32)
    lo, hi = _f32(), _f32()
    check(lib.vgt_hipx_sdf_multi(devs, len(devices), _ptr(occ) if occ.size else None, nx, ny, nz, float(resolution),
                                 int(bool(unknown_is_filled)), int(bool(add_virtual_border)), _ptr(out),
                                 ctypes.byref(lo), ctypes.byref(hi)))
    return out, lo.value, hi.value


def point_share(num_points, shares, share):
    """vgt_hipx_point_share -> (first, count) of `share` among `shares` contiguous shares of a cloud."""
    first, count = ctypes.c_int64(0), ctypes.c_int64(0)
    check(load().vgt_hipx_point_share(int(num_points), int(shares), int(share), ctypes.byref(first), ctypes.byref(count)))
    return first.value, count.value


def sdf_multi_release():
    """Frees the device state vgt_hipx_sdf_multi keeps between calls."""
    load().vgt_hipx_release()


def sdf_multi_last_timing():
    """Phases of the last sdf_multi call in ms: setup, upload, compute, download (slowest slab each), total."""
    ms = (ctypes.c_float * 5)()
    check(load().vgt_hipx_last_timing(ms))
    return dict(zip(("setup_ms", "upload_ms", "compute_ms", "download_ms", "total_ms"), [float(v) for v in ms]))


def sdf_batch_workspace_bytes(batch, shape):
    return int(load().vgt_hip_sdf_batch_workspace_bytes(int(batch), *[int(v) for v in shape]))


def nearest_workspace_bytes(shape):
    """Workspace of Context.nearest_dev; 0 for an empty or over-limit grid."""
    return int(load().vgt_hip_nearest_workspace_bytes(*[int(s) for s in shape]))


def align_points_workspace_bytes(num_points, num_poses):
    """Workspace of Context.align_points_dev; 0 for sizes the call refuses."""
    return int(load().vgt_hip_align_points_workspace_bytes(int(num_points), int(num_poses)))


def sdf_workspace_bytes(shape, variant=0):
    """Workspace of the device-resident SDF entry points (variant != 0: a cross-check pipeline of the testing library)."""
    lib = load(testing=int(variant) != 0)
    return int(lib.vgt_hip_sdf_workspace_bytes_for_variant(*[int(s) for s in shape], int(variant)))


def ik_max_chain_joints():
    """vgt_hip_ik_max_chain_joints: the most moving links solve_ik takes on a chain (a constant of the kernel)."""
    return int(load().vgt_hip_ik_max_chain_joints())


def solve_ik_workspace_bytes(num_joints, num_problems):
    """Workspace of Context.solve_ik_dev without joints_out_ptr; 0 for sizes the call refuses."""
    return int(load().vgt_hip_solve_ik_workspace_bytes(int(num_joints), int(num_problems)))


def kinematics_lds_links():
    """vgt_hip_kinematics_lds_links: how many links' poses the forward kinematics keeps in LDS (a constant of the kernel)."""
    return int(load().vgt_hip_kinematics_lds_links())


def motion_tile_samples(num_links):
    """vgt_hip_motion_tile_samples: the samples per tile check_motions uses for a tree of so many links; 0: too many."""
    return int(load().vgt_hip_motion_tile_samples(int(num_links)))


def cost_tile_samples(num_links):
    """vgt_hip_cost_tile_samples: the configurations per tile clearance_cost uses for a tree of so many links; 0: too
    many."""
    return int(load().vgt_hip_cost_tile_samples(int(num_links)))


MotionLaunchGeometry = collections.namedtuple("MotionLaunchGeometry", "tile_samples table_in_lds")
CostLaunchGeometry = collections.namedtuple("CostLaunchGeometry", "tile_samples passes table_in_lds links_in_lds")


def motion_launch_geometry(num_links, num_spheres):
    """Testing library only (vgt_hip_testing_motion_launch_geometry): what a check_motions launch for so many links and
    spheres is made of, from the launcher's own selection.  Raises ValueError for a tree the kernel does not take."""
    out = [_i32(), _i32()]
    check(load(testing=True).vgt_hip_testing_motion_launch_geometry(int(num_links), int(num_spheres),
                                                                    *[ctypes.byref(o) for o in out]))
    return MotionLaunchGeometry(*[int(o.value) for o in out])


def cost_launch_geometry(num_links, num_spheres, gradient_form=True):
    """Testing library only (vgt_hip_testing_cost_launch_geometry): what a clearance_cost launch for so many links and
    spheres is made of in the gradient form or the cost-only form, from the launcher's own selection.  Raises ValueError
    for a tree the kernel does not take."""
    out = [_i32(), _i32(), _i32(), _i32()]
    check(load(testing=True).vgt_hip_testing_cost_launch_geometry(int(num_links), int(num_spheres),
                                                                  int(bool(gradient_form)),
                                                                  *[ctypes.byref(o) for o in out]))
    return CostLaunchGeometry(*[int(o.value) for o in out])


def self_collision_tile_samples(num_links, num_spheres):
    """vgt_hip_self_collision_tile_samples: the configurations per tile check_self_collision uses for a tree of so many
    links carrying so many spheres; 0: the kernel does not take the shape."""
    return int(load().vgt_hip_self_collision_tile_samples(int(num_links), int(num_spheres)))


def motion_self_tile_samples(num_links, num_spheres):
    """vgt_hip_motion_self_tile_samples: the samples per tile check_motions_with_self uses for a tree of so many links
    carrying so many spheres; 0: the kernel does not take the shape."""
    return int(load().vgt_hip_motion_self_tile_samples(int(num_links), int(num_spheres)))


def self_collision_pairs(sphere_link, num_links, parent=None, ignored_link_pairs=None, skip_adjacent=False,
                         capacity=None):
    """vgt_hip_self_collision_pairs (host only, no context): -> (pairs [min(count, capacity), 2] int32, count): in
    lexicographic order every (a, b), a < b, of spheres on different links that are not an ignored link pair
    (`ignored_link_pairs` [K, 2], unordered) and, with skip_adjacent and `parent` [L], not parent and child.  capacity
    None: room for all of them."""
    link = np.ascontiguousarray(sphere_link, dtype=np.int32).reshape(-1)
    up = None if parent is None else np.ascontiguousarray(parent, dtype=np.int32).reshape(-1)
    if up is not None and len(up) != int(num_links):
        raise ValueError("parent must hold one entry per link")
    ignored = None if ignored_link_pairs is None else _sphere_pairs(ignored_link_pairs)
    flags = SELF_PAIRS_SKIP_ADJACENT if skip_adjacent else 0
    lib = load()
    count = ctypes.c_int64(-1)

    def call(out, room):
        check(lib.vgt_hip_self_collision_pairs(_ptr(link), len(link), _ptr(up), int(num_links), _ptr(ignored),
                                               0 if ignored is None else len(ignored), flags, _ptr(out), room,
                                               ctypes.byref(count)))
    if capacity is None:
        call(None, 0)
        capacity = count.value
    out = np.empty((int(capacity), 2), np.int32)
    call(out if capacity > 0 else None, int(capacity))
    return out[:min(count.value, int(capacity))], int(count.value)


class KinematicTree:
    """A kinematic tree on the device (vgt_hip_kinematics): made by Context.kinematics, used by forward_kinematics and
    clearance_joint_gradient any number of times."""

    def __init__(self, ctx, parent, joint_type, joint_index, axis, origin, num_joints=None):
        self.handle = None
        parent = np.ascontiguousarray(parent, dtype=np.int32).reshape(-1)
        joint_type = np.ascontiguousarray(joint_type, dtype=np.int32).reshape(-1)
        joint_index = np.ascontiguousarray(joint_index, dtype=np.int32).reshape(-1)
        links = len(parent)
        axis = np.ascontiguousarray(axis, dtype=np.float64)
        origin = np.asarray(origin, dtype=np.float64)
        if origin.ndim == 3:
            if origin.shape[1:] != (4, 4):
                raise ValueError("origin must have the shape [L, 16] or [L, 4, 4]")
            origin = origin.transpose(0, 2, 1).reshape(origin.shape[0], 16)
        origin = np.ascontiguousarray(origin)
        if len(joint_type) != links or len(joint_index) != links or axis.shape != (links, 3) or \
                origin.shape != (links, 16):
            raise ValueError("a kinematic tree holds one parent, joint type, joint index, axis [3] and origin [16] per link")
        if num_joints is None:
            moving = joint_index[joint_type != JOINT_FIXED]
            num_joints = int(moving.max()) + 1 if len(moving) else 0
        h = _p()
        check(ctx._lib.vgt_hip_kinematics_create(ctx.handle, links, int(num_joints), _ptr(parent), _ptr(joint_type),
                                                 _ptr(joint_index), _ptr(axis), _ptr(origin), ctypes.byref(h)))
        self._lib = ctx._lib
        self.handle = h
        self.num_links = links
        self.num_joints = int(num_joints)
        ctx._adopt(self)

    def _handle_or_raise(self):
        if not self.handle:
            raise ValueError("the kinematic tree has been closed")
        return self.handle

    def close(self):
        if getattr(self, "handle", None):
            self._lib.vgt_hip_kinematics_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class TrackingGrids:
    def __init__(self, ctx, num_cells, num_grids):
        self.ctx = ctx
        self._lib = ctx._lib
        h = _p()
        check(self._lib.vgt_hip_tracking_grids_create(ctx.handle, int(num_cells), int(num_grids),
                                                      ctypes.byref(h)))
        self.handle = h
        ctx._adopt(self)
        ctx._adopt(self)
        self.num_cells = int(num_cells)
        self.num_grids = int(num_grids)

    def close(self):
        if getattr(self, "handle", None):
            self._lib.vgt_hip_tracking_grids_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def offset(self, index):
        return int(self._lib.vgt_hip_tracking_grids_offset(self.handle, index))

    def dev_ptr(self, index):
        return self._lib.vgt_hip_tracking_grids_dev_ptr(self.handle, index)

    def clear(self):
        check(self._lib.vgt_hip_tracking_grids_clear(self.ctx.handle, self.handle))

    def raycast_f32(self, index, points, max_range, xform, voxel_size, inverse_voxel_size,
                    grid_sizes, counts):
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1)
        T = np.ascontiguousarray(xform, dtype=np.float32).reshape(16)
        check(self._lib.vgt_hip_raycast_points_f32(
            self.ctx.handle, self.handle, index, _ptr(pts) if pts.size else None, pts.size // 3,
            float(max_range), _ptr(T), float(voxel_size), float(inverse_voxel_size),
            float(grid_sizes[0]), float(grid_sizes[1]), float(grid_sizes[2]),
            int(counts[0]), int(counts[1]), int(counts[2])))

    def raycast_f32_split(self, index, helper_devices, points, max_range, xform, voxel_size, inverse_voxel_size,
                          grid_sizes, counts):
        """vgt_hipx_raycast_points_split: one cloud over this context's device + `helper_devices` (a device may
        repeat); the private grids are summed into grid `index`."""
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1)
        T = np.ascontiguousarray(xform, dtype=np.float32).reshape(16)
        devs = (ctypes.c_int * max(len(helper_devices), 1))(*[int(d) for d in helper_devices])
        check(self._lib.vgt_hipx_raycast_points_split(
            self.ctx.handle, self.handle, index, devs, len(helper_devices), _ptr(pts) if pts.size else None,
            pts.size // 3, float(max_range), _ptr(T), float(voxel_size), float(inverse_voxel_size),
            float(grid_sizes[0]), float(grid_sizes[1]), float(grid_sizes[2]),
            int(counts[0]), int(counts[1]), int(counts[2])))

    def raycast_pointcloud2(self, index, data, num_points, point_step, xyz_offset, max_range, xform, voxel_size,
                            inverse_voxel_size, grid_sizes, counts):
        """sensor_msgs/PointCloud2 data buffer (bytes) with x, y, z FLOAT32 at xyz_offset of every record."""
        buf = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray)
                                   else data.view(np.uint8).reshape(-1))
        if buf.size < int(num_points) * int(point_step):
            raise ValueError("data buffer shorter than num_points * point_step")
        T = np.ascontiguousarray(xform, dtype=np.float32).reshape(16)
        check(self._lib.vgt_hip_raycast_pointcloud2_f32(
            self.ctx.handle, self.handle, index, _ptr(buf) if buf.size else None, int(num_points),
            int(point_step), int(xyz_offset), float(max_range), _ptr(T), float(voxel_size),
            float(inverse_voxel_size), float(grid_sizes[0]), float(grid_sizes[1]), float(grid_sizes[2]),
            int(counts[0]), int(counts[1]), int(counts[2])))

    def raycast_f32_dev(self, index, points_ptr, num_points, max_range, xform, voxel_size,
                        inverse_voxel_size, grid_sizes, counts):
        T = np.ascontiguousarray(xform, dtype=np.float32).reshape(16)
        check(self._lib.vgt_hip_raycast_points_f32_dev(
            self.ctx.handle, self.handle, index, _ptr(points_ptr), int(num_points),
            float(max_range), _ptr(T), float(voxel_size), float(inverse_voxel_size),
            float(grid_sizes[0]), float(grid_sizes[1]), float(grid_sizes[2]),
            int(counts[0]), int(counts[1]), int(counts[2])))

    def raycast_f64(self, index, points, max_range, xform, voxel_size, inverse_voxel_size,
                    grid_sizes, counts):
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1)
        T = np.ascontiguousarray(xform, dtype=np.float64).reshape(16)
        check(self._lib.vgt_hip_raycast_points_f64(
            self.ctx.handle, self.handle, index, _ptr(pts) if pts.size else None, pts.size // 3,
            float(max_range), _ptr(T), float(voxel_size), float(inverse_voxel_size),
            float(grid_sizes[0]), float(grid_sizes[1]), float(grid_sizes[2]),
            int(counts[0]), int(counts[1]), int(counts[2])))

    def retrieve(self, index, counts=None):
        out = np.empty((self.num_cells, 2), dtype=np.int32)
        check(self._lib.vgt_hip_retrieve_tracking_grid(self.ctx.handle, self.handle, index,
                                                       _ptr(out)))
        if counts is not None:
            out = out.reshape(tuple(counts) + (2,))
        return out


class FilterGrid:
    def __init__(self, ctx, occupancy):
        self.ctx = ctx
        self._lib = ctx._lib
        occ = np.ascontiguousarray(occupancy, dtype=np.float32)
        self.shape = occ.shape
        h = _p()
        check(self._lib.vgt_hip_filter_grid_create(ctx.handle, occ.size,
                                                   _ptr(occ) if occ.size else None,
                                                   ctypes.byref(h)))
        self.handle = h
        ctx._adopt(self)

    def close(self):
        if getattr(self, "handle", None):
            self._lib.vgt_hip_filter_grid_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def dev_ptr(self):
        return self._lib.vgt_hip_filter_grid_dev_ptr(self.handle)

    def filter(self, grids, percent_seen_free=1.0, outlier_points_threshold=1,
               num_cameras_seen_free=1, ratio_in_double=False):
        if ratio_in_double:
            check(self._lib.vgt_hip_filter_tracking_grids_f64(
                self.ctx.handle, grids.handle, float(percent_seen_free),
                int(outlier_points_threshold), int(num_cameras_seen_free), self.handle))
        else:
            check(self._lib.vgt_hip_filter_tracking_grids(
                self.ctx.handle, grids.handle, float(percent_seen_free),
                int(outlier_points_threshold), int(num_cameras_seen_free), self.handle))

    def retrieve(self):
        out = np.empty(self.shape, dtype=np.float32)
        check(self._lib.vgt_hip_retrieve_filtered_grid(self.ctx.handle, self.handle, _ptr(out)))
        return out


# numpy record layouts of the reference's cell types (occupancy first, then uint32 fields)
OCCUPANCY_COMPONENT_CELL = np.dtype([("occupancy", np.float32), ("component", np.uint32)])
TAGGED_OBJECT_CELL = np.dtype([("occupancy", np.float32), ("object_id", np.uint32)])
TAGGED_OBJECT_COMPONENT_CELL = np.dtype([("occupancy", np.float32), ("object_id", np.uint32),
                                         ("component", np.uint32), ("spatial_segment", np.uint32)])


class Cells:
    """Device copy of the raw cell store of an OccupancyComponentMap / TaggedObjectOccupancyMap /
    TaggedObjectOccupancyComponentMap, for any number of SDF extractions (vgt_hip_cells_*)."""

    def __init__(self, ctx, records, shape, object_id_offset=4):
        self.ctx = ctx
        self._lib = ctx._lib
        rec = np.ascontiguousarray(records)
        self.shape = tuple(int(s) for s in shape)
        if rec.size != int(np.prod(self.shape)):
            raise ValueError("records do not match the grid shape")
        h = _p()
        check(self._lib.vgt_hip_cells_create(ctx.handle, _ptr(rec), self.shape[0], self.shape[1], self.shape[2],
                                             rec.dtype.itemsize, int(object_id_offset), ctypes.byref(h)))
        self.handle = h
        ctx._adopt(self)

    def close(self):
        if getattr(self, "handle", None):
            self._lib.vgt_hip_cells_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def object_ids(self, capacity=4096):
        ids = np.zeros(capacity, dtype=np.uint32)
        count = ctypes.c_int64(0)
        check(self._lib.vgt_hip_cells_object_ids(self.ctx.handle, self.handle, _ptr(ids), capacity,
                                                 ctypes.byref(count)))
        if count.value > capacity:
            return self.object_ids(int(count.value))
        return ids[:count.value].copy()

    def sdf(self, resolution, objects_to_use=(), unknown_is_filled=True, add_virtual_border=False):
        objs = np.ascontiguousarray(np.asarray(list(objects_to_use), dtype=np.uint32))
        out = np.empty(self.shape, dtype=np.float32)
        lo, hi = ctypes.c_float(0), ctypes.c_float(0)
        check(self._lib.vgt_hip_cells_sdf(self.ctx.handle, self.handle, _ptr(objs) if objs.size else None,
                                          objs.size, float(resolution), int(bool(unknown_is_filled)),
                                          int(bool(add_virtual_border)), _ptr(out), ctypes.byref(lo),
                                          ctypes.byref(hi)))
        return out, float(lo.value), float(hi.value)

    def nearest(self, objects_to_use=(), unknown_is_filled=True, with_d2=False, with_object_ids=False):
        """vgt_hip_cells_nearest: the nearest cell of the other class under the filled predicate of sdf() -> int32
        nearest, or (nearest[, d2][, object]) -- object: uint32, the id of the cell itself where it is filled, else of
        its nearest cell, 0 where there is none."""
        objs = np.ascontiguousarray(np.asarray(list(objects_to_use), dtype=np.uint32))
        nearest = np.empty(self.shape, dtype=np.int32)
        d2 = np.empty(self.shape, dtype=np.int32) if with_d2 else None
        obj = np.empty(self.shape, dtype=np.uint32) if with_object_ids else None
        check(self._lib.vgt_hip_cells_nearest(self.ctx.handle, self.handle, _ptr(objs) if objs.size else None, objs.size,
                                              int(bool(unknown_is_filled)), _ptr(nearest), _ptr(d2), _ptr(obj)))
        out = (nearest,) + ((d2,) if with_d2 else ()) + ((obj,) if with_object_ids else ())
        return out if len(out) > 1 else nearest

    def separate_object_sdfs(self, resolution, object_ids, unknown_is_filled=True, add_virtual_border=False):
        """MakeSeparateObjectSDFs: {object id: (sdf, min, max)}, all objects in one batched extraction
        (vgt_hip_cells_object_sdfs)."""
        ids = np.ascontiguousarray(np.asarray(list(object_ids), dtype=np.uint32))
        if ids.size == 0:
            return {}
        outs = [np.empty(self.shape, dtype=np.float32) for _ in range(ids.size)]
        out_ptrs = (ctypes.c_void_p * ids.size)(*[o.ctypes.data for o in outs])
        lo = np.zeros(ids.size, dtype=np.float32)
        hi = np.zeros(ids.size, dtype=np.float32)
        check(self._lib.vgt_hip_cells_object_sdfs(
            self.ctx.handle, self.handle, _ptr(ids), ids.size, float(resolution), int(bool(unknown_is_filled)),
            int(bool(add_virtual_border)), ctypes.cast(out_ptrs, ctypes.c_void_p), _ptr(lo), _ptr(hi)))
        return {int(i): (outs[k], float(lo[k]), float(hi[k])) for k, i in enumerate(ids)}

    def separate_object_sdfs_one_by_one(self, resolution, object_ids, **kw):
        """The reference's own loop: one ExtractSignedDistanceField({id}) per object (vgt_hip_cells_sdf)."""
        return {int(i): self.sdf(resolution, [int(i)], **kw) for i in object_ids}

    def all_object_sdfs(self, resolution, **kw):
        """MakeAllObjectSDFs."""
        return self.separate_object_sdfs(resolution, self.object_ids(), **kw)

    def free_and_named_objects_sdf(self, resolution, unknown_is_filled=True, add_virtual_border=False):
        out = np.empty(self.shape, dtype=np.float32)
        lo, hi = ctypes.c_float(0), ctypes.c_float(0)
        check(self._lib.vgt_hip_cells_free_and_named_objects_sdf(
            self.ctx.handle, self.handle, float(resolution), int(bool(unknown_is_filled)),
            int(bool(add_virtual_border)), _ptr(out), ctypes.byref(lo), ctypes.byref(hi)))
        return out, float(lo.value), float(hi.value)

    def connected_components(self, connect_across_objects=False):
        """UpdateConnectedComponents: (uint32 labels, number of components)."""
        labels = np.empty(self.shape, dtype=np.uint32)
        count = ctypes.c_uint32(0)
        check(self._lib.vgt_hip_cells_connected_components(self.ctx.handle, self.handle,
                                                           int(bool(connect_across_objects)), _ptr(labels),
                                                           ctypes.byref(count)))
        return labels, int(count.value)

    def select(self, rule, class_mask, payload_member=CELL_MEMBER_NONE, labels_ptr=None, with_occupancy=False):
        """The uploaded cells that `rule` selects among the occupancy classes of class_mask (threshold 0.5): int32 linear
        indices in ascending order, or (indices[, occupancy][, payload]) with with_occupancy and a payload_member
        (CELL_MEMBER_*).  labels_ptr: device labels for SELECT_COMPONENT_SURFACE; None: the cells' `component` member."""
        count = ctypes.c_int64(0)

        def call(indices, occ, payload, capacity):
            check(self._lib.vgt_hip_cells_select(self.ctx.handle, self.handle, _ptr(labels_ptr), int(rule),
                                                 int(class_mask), _ptr(indices), _ptr(occ), _ptr(payload),
                                                 int(payload_member), capacity, ctypes.byref(count)))

        call(None, None, None, 0)
        n = int(count.value)
        want_payload = int(payload_member) != CELL_MEMBER_NONE
        indices = np.empty(n, dtype=np.int32)
        occ = np.empty(n, dtype=np.float32) if with_occupancy else None
        payload = np.empty(n, dtype=np.uint32) if want_payload else None
        if n:
            call(indices, occ, payload, n)
        out = (indices,) + ((occ,) if with_occupancy else ()) + ((payload,) if want_payload else ())
        return out if len(out) > 1 else indices

    def extract_surface(self, resolution, world_from_grid=None, with_cells=False):
        """vgt_hip_cells_extract_surface: the surface of the uploaded cells' occupancy (inside: > 0.5) as an indexed
        mesh, as Context.extract_surface(occupancy, resolution, 0.5, True, ...) returns it."""
        wfg, _ = _mesh_transforms(world_from_grid, None)

        def call(vertices, cells, vertex_capacity, triangles, triangle_capacity, nv, nt):
            return self._lib.vgt_hip_cells_extract_surface(
                self.ctx.handle, self.handle, float(resolution), _ptr(wfg), _ptr(vertices), _ptr(cells),
                vertex_capacity, _ptr(triangles), triangle_capacity, nv, nt)

        return _surface_mesh(call, with_cells)

    def travel_cost(self, sources, weights=(10, 14, 17), objects_to_use=(), unknown_is_filled=True,
                    no_corner_cutting=False, source_costs=None, cost_limit=TRAVEL_NO_LIMIT, with_toward=True):
        """vgt_hip_cells_travel_cost: Context.travel_cost on the uploaded cells; blocked is the filled predicate of
        sdf() -> (cost, toward or None, num_reached)."""
        objs = np.ascontiguousarray(np.asarray(list(objects_to_use), dtype=np.uint32))
        src, costs = _travel_sources(sources, source_costs)
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.uint32).reshape(3))
        cost = np.empty(self.shape, dtype=np.uint32)
        toward = np.empty(self.shape, dtype=np.int32) if with_toward else None
        reached = ctypes.c_int64(0)
        check(self._lib.vgt_hip_cells_travel_cost(
            self.ctx.handle, self.handle, _ptr(objs) if objs.size else None, objs.size, int(bool(unknown_is_filled)),
            _ptr(w), TRAVEL_NO_CORNER_CUTTING if no_corner_cutting else 0, _ptr(src), _ptr(costs), src.size,
            int(cost_limit), _ptr(cost), _ptr(toward), ctypes.byref(reached)))
        return cost, toward, int(reached.value)

    def component_topology(self, component_types, connect_across_objects=False, with_labels=False):
        """ComputeComponentTopology of the uploaded cells: the COMPONENT_TOPOLOGY table of Context.component_topology;
        with_labels=True: (table, uint32 labels)."""
        labels = np.empty(self.shape, dtype=np.uint32) if with_labels else None
        table = _topology_table(
            lambda out, capacity, count: self._lib.vgt_hip_cells_component_topology(
                self.ctx.handle, self.handle, int(bool(connect_across_objects)), int(component_types), _ptr(labels),
                count, _ptr(out), capacity))
        return (table, labels) if with_labels else table

    def spatial_segments(self, extrema, threshold):
        """The labelling step of UpdateSpatialSegments on a given local-extrema map [nx, ny, nz, 3] float64:
        (uint32 labels, number of segments)."""
        ext = np.ascontiguousarray(extrema, dtype=np.float64)
        if ext.shape != self.shape + (3,):
            raise ValueError("the extrema map must be (nx, ny, nz, 3)")
        labels = np.empty(self.shape, dtype=np.uint32)
        count = ctypes.c_uint32(0)
        check(self._lib.vgt_hip_cells_spatial_segments(self.ctx.handle, self.handle, _ptr(ext), float(threshold),
                                                       _ptr(labels), ctypes.byref(count)))
        return labels, int(count.value)

    def spatial_segments_dev(self, extrema_ptr, threshold, labels_ptr):
        count = ctypes.c_uint32(0)
        check(self._lib.vgt_hip_cells_spatial_segments_dev(self.ctx.handle, self.handle, _ptr(extrema_ptr),
                                                           float(threshold), _ptr(labels_ptr), ctypes.byref(count)))
        return int(count.value)

    def update_spatial_segments(self, threshold, resolution, unknown_is_filled=True, add_virtual_border=False,
                                rotation=None):
        """UpdateSpatialSegments in one call (SDF -> local extrema -> segments on the device):
        (uint32 labels, number of segments)."""
        rot = None if rotation is None else np.ascontiguousarray(rotation, dtype=np.float64).reshape(9)
        labels = np.empty(self.shape, dtype=np.uint32)
        count = ctypes.c_uint32(0)
        check(self._lib.vgt_hip_cells_update_spatial_segments(
            self.ctx.handle, self.handle, float(threshold), float(resolution), int(bool(unknown_is_filled)),
            int(bool(add_virtual_border)), _ptr(rot), _ptr(labels), ctypes.byref(count)))
        return labels, int(count.value)
