"""ctypes binding of libmav_trajectory_generation.so (the C ABI, include/mtg.h).

The product path has no CPU fallback: if the HIP library is missing or no GPU
is visible, calls raise.  PyTorch is only used (in solver.py) as an optional
holder of device memory and streams.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libmav_trajectory_generation.so")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "mtg.h")

MTG_OK = 0
MTG_ERR_INVALID_ARGUMENT = -1
MTG_ERR_UNSUPPORTED_N = -2
MTG_ERR_BAD_DERIVATIVE = -3
MTG_ERR_SIZE_MISMATCH = -4
MTG_ERR_HIP = -5
MTG_ERR_NO_DEVICE = -6
MTG_ERR_OUT_OF_MEMORY = -7
MTG_ERR_TOO_LARGE = -8

MTG_TRAJ_OK = 0
MTG_TRAJ_BAD_TIME = 1
MTG_TRAJ_NOT_SPD = 2
MTG_TRAJ_ROW_TOO_SHORT = 4
MTG_TRAJ_WARN_DROPPED = 256
MTG_TRAJ_ERROR_MASK = 255

MTG_FLAG_DEVICE_PTRS = 1
MTG_FLAG_ASYNC = 2
MTG_FLAG_SPLIT_KERNELS = 4
MTG_FLAG_GENERAL_KERNEL = 8
MTG_FLAG_DL_KERNEL = 64
MTG_FLAG_COLUMN_KERNEL = 128
MTG_DL_MIN_BATCH = 1

MTG_KERNEL_COLUMN = 2
MTG_KERNEL_GENERAL = 3
MTG_KERNEL_SPLIT = 4
MTG_KERNEL_DL = 6
MTG_KERNEL_DLX = 7
KERNEL_NAMES = {MTG_KERNEL_COLUMN: "solve_reg_kernel",
                MTG_KERNEL_GENERAL: "solve_fused_kernel", MTG_KERNEL_SPLIT: "assemble+block_cholesky",
                MTG_KERNEL_DL: "solve_dl_kernel", MTG_KERNEL_DLX: "solve_dlx_kernel"}

MTG_EVALUATE_AT_LANE = 1
MTG_EVALUATE_AT_STAGED = 2

MTG_OBJECTIVE_FREE_CONSTRAINTS = 0
MTG_OBJECTIVE_FREE_CONSTRAINTS_AND_COLLISION = 1
MTG_OBJECTIVE_FREE_CONSTRAINTS_AND_COLLISION_AND_TIME = 2
MTG_OBJECTIVE_TIME = 3                      # mtg_objective_time_batch (mtg_objective_batch rejects 3 and 4)
MTG_OBJECTIVE_TIME_AND_CONSTRAINTS = 4
MTG_OBJECTIVE_USE_NUMERIC_GRAD = 1          # bits of ObjectiveParams.reserved: not covered
MTG_OBJECTIVE_SIMPLE_NUMGRAD_TIME = 2
MTG_OBJECTIVE_SIMPLE_NUMGRAD_CONSTRAINTS = 4

_c_dp = ctypes.c_void_p  # every array argument is passed as a raw address


class SdfGrid(ctypes.Structure):
    """struct mtg_sdf_grid (include/mtg.h)."""
    _fields_ = [("distance", ctypes.c_void_p), ("nx", ctypes.c_int32), ("ny", ctypes.c_int32), ("nz", ctypes.c_int32),
                ("origin", ctypes.c_double * 3), ("resolution", ctypes.c_double), ("oob_distance", ctypes.c_double)]


class CollisionParams(ctypes.Structure):
    """struct mtg_collision_params (include/mtg.h)."""
    _fields_ = [("coll_check_time_increment", ctypes.c_double), ("map_resolution", ctypes.c_double),
                ("epsilon", ctypes.c_double), ("robot_radius", ctypes.c_double),
                ("coll_pot_multiplier", ctypes.c_double), ("min_bound", ctypes.c_double * 3),
                ("max_bound", ctypes.c_double * 3), ("use_continuous_distance", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class SoftConstraintParams(ctypes.Structure):
    """struct mtg_soft_constraint_params (include/mtg.h)."""
    _fields_ = [("n_constraints", ctypes.c_int32), ("derivative", ctypes.c_int32 * 8), ("limit", ctypes.c_double * 8),
                ("weight", ctypes.c_double), ("maximum_cost", ctypes.c_double), ("increment", ctypes.c_double)]


class ObjectiveParams(ctypes.Structure):
    """struct mtg_objective_params (include/mtg.h)."""
    _fields_ = [("objective", ctypes.c_int32), ("derivative_to_optimize", ctypes.c_int32), ("w_d", ctypes.c_double),
                ("w_c", ctypes.c_double), ("w_t", ctypes.c_double), ("w_sc", ctypes.c_double),
                ("increment_time", ctypes.c_double), ("use_soft_constraints", ctypes.c_int32),
                ("is_collision_safe", ctypes.c_int32), ("is_coll_raise_first_iter", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("add_coll_raise", ctypes.c_double)]


class ObjectiveTimeParams(ctypes.Structure):
    """struct mtg_objective_time_params (include/mtg.h)."""
    _fields_ = [("objective", ctypes.c_int32), ("derivative_to_optimize", ctypes.c_int32),
                ("time_penalty", ctypes.c_double), ("w_c", ctypes.c_double), ("use_soft_constraints", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class ObjectiveParts(ctypes.Structure):
    """struct mtg_objective_parts (include/mtg.h): nine nullable double pointers."""
    _fields_ = [(k, ctypes.c_void_p) for k in ("J_d", "J_c", "J_sc", "J_t", "dJd_dt", "dJc_dt", "grad_d", "grad_c",
                                               "grad_sc")]


_SIGNATURES = {
    "mtg_abi_version": (ctypes.c_int, []),
    "mtg_solve_kernel": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint]),
    "mtg_solve_kernel_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                              ctypes.c_uint]),
    "mtg_status_string": (ctypes.c_char_p, [ctypes.c_int]),
    "mtg_last_error": (ctypes.c_char_p, [ctypes.c_void_p]),
    "mtg_device_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    "mtg_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    "mtg_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "mtg_set_stream": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "mtg_reset_stream": (ctypes.c_int, [ctypes.c_void_p]),
    "mtg_get_stream": (ctypes.c_void_p, [ctypes.c_void_p]),
    "mtg_synchronize": (ctypes.c_int, [ctypes.c_void_p]),
    "mtg_solve_linear_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int64, _c_dp, _c_dp, _c_dp, _c_dp,
                                              _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_uint]),
    "mtg_solve_linear_ragged_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                     ctypes.c_int64, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp,
                                                     _c_dp, _c_dp, ctypes.c_uint]),
    "mtg_solve_ragged_plan": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64, _c_dp,
                                             ctypes.c_uint, ctypes.POINTER(ctypes.c_int64),
                                             ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    "mtg_host_solve_linear_ragged_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                                          _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp,
                                                          _c_dp, ctypes.c_int]),
    "mtg_evaluate_at_ragged_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int64, _c_dp,
                                                    _c_dp, _c_dp, _c_dp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                                                    ctypes.c_int, _c_dp, _c_dp, _c_dp, ctypes.c_uint]),
    "mtg_evaluate_at_ragged_path": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                                   ctypes.c_int]),
    "mtg_host_evaluate_at_ragged_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, _c_dp, _c_dp,
                                                         _c_dp, _c_dp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                                                         ctypes.c_int, _c_dp, _c_dp, _c_dp, ctypes.c_int]),
    "mtg_min_max_magnitude_ragged_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                                          _c_dp, _c_dp, _c_dp, ctypes.c_int, ctypes.c_uint32, _c_dp,
                                                          _c_dp, ctypes.c_uint]),
    "mtg_host_min_max_magnitude_ragged_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, _c_dp, _c_dp,
                                                               _c_dp, ctypes.c_int, ctypes.c_uint32, _c_dp, _c_dp,
                                                               ctypes.c_int]),
    "mtg_coefficients_from_vertices_ragged_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                                   ctypes.c_int64, _c_dp, _c_dp, _c_dp, _c_dp,
                                                                   ctypes.c_uint]),
    "mtg_vertex_derivatives_ragged_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                                           _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_uint]),
    "mtg_vertex_ragged_tile": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    "mtg_collision_cost_ragged_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                                       _c_dp, _c_dp, _c_dp, _c_dp, ctypes.POINTER(SdfGrid),
                                                       ctypes.POINTER(CollisionParams), _c_dp, _c_dp, _c_dp, _c_dp,
                                                       _c_dp, ctypes.c_uint]),
    "mtg_host_collision_cost_ragged_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, _c_dp, _c_dp,
                                                            _c_dp, _c_dp, ctypes.POINTER(SdfGrid),
                                                            ctypes.POINTER(CollisionParams), _c_dp, _c_dp, _c_dp,
                                                            _c_dp, _c_dp, ctypes.c_int]),
    "mtg_host_vertex_derivatives_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                                         _c_dp, _c_dp, _c_dp, ctypes.c_int]),
    "mtg_host_vertex_derivatives_ragged_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, _c_dp,
                                                                _c_dp, _c_dp, _c_dp, ctypes.c_int]),
    "mtg_host_coefficients_from_vertices_ragged_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                                                        _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_int]),
    "mtg_shard_range": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int64),
                                       ctypes.POINTER(ctypes.c_int64)]),
    "mtg_solve_linear_batch_multi": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                    ctypes.c_int, ctypes.c_int, ctypes.c_int64, _c_dp, _c_dp, _c_dp,
                                                    _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_uint]),
    "mtg_debug_fail_next_solve": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "mtg_evaluate_range_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_int64, _c_dp, _c_dp, ctypes.c_double, ctypes.c_double,
                                                ctypes.c_double, ctypes.c_int, _c_dp, _c_dp, _c_dp, _c_dp,
                                                ctypes.c_uint]),
    "mtg_evaluate_range_batch_full": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                     ctypes.c_int64, _c_dp, _c_dp, ctypes.c_double, ctypes.c_double,
                                                     ctypes.c_double, ctypes.c_int, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp,
                                                     ctypes.c_int64, ctypes.c_uint]),
    "mtg_evaluate_range_ragged_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                                       _c_dp, _c_dp, _c_dp, ctypes.c_double, ctypes.c_double,
                                                       ctypes.c_double, ctypes.c_int, _c_dp, _c_dp, _c_dp, _c_dp,
                                                       ctypes.c_uint]),
    "mtg_evaluate_range_ragged_batch_full": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                            ctypes.c_int64, _c_dp, _c_dp, _c_dp, ctypes.c_double,
                                                            ctypes.c_double, ctypes.c_double, ctypes.c_int, _c_dp,
                                                            _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_int64,
                                                            ctypes.c_uint]),
    "mtg_evaluate_at_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                             _c_dp, _c_dp, _c_dp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                                             ctypes.c_int, _c_dp, _c_dp, _c_dp, ctypes.c_uint]),
    "mtg_evaluate_at_path": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int]),
    "mtg_host_evaluate_at_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64, _c_dp,
                                                  _c_dp, _c_dp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                                                  ctypes.c_int, _c_dp, _c_dp, _c_dp, ctypes.c_int]),
    "mtg_time_sweep_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_int64, _c_dp, _c_dp, _c_dp, ctypes.c_int,
                                            _c_dp, _c_dp, _c_dp, ctypes.c_uint]),
    "mtg_cost_at_times_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_int64, _c_dp, _c_dp, _c_dp, ctypes.c_int,
                                               _c_dp, _c_dp, _c_dp, ctypes.c_uint]),
    "mtg_collision_cost_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_int64, _c_dp, _c_dp, _c_dp, ctypes.POINTER(SdfGrid),
                                                ctypes.POINTER(CollisionParams), _c_dp, _c_dp, _c_dp, _c_dp, _c_dp,
                                                ctypes.c_uint]),
    "mtg_host_collision_cost_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64, _c_dp,
                                                     _c_dp, _c_dp, ctypes.POINTER(SdfGrid),
                                                     ctypes.POINTER(CollisionParams), _c_dp, _c_dp, _c_dp, _c_dp,
                                                     _c_dp, ctypes.c_int]),
    "mtg_collision_time_gradient_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                         ctypes.c_int64, _c_dp, _c_dp, ctypes.POINTER(SdfGrid),
                                                         ctypes.POINTER(CollisionParams), ctypes.c_double, _c_dp, _c_dp,
                                                         _c_dp, _c_dp, _c_dp, ctypes.c_uint]),
    "mtg_host_collision_time_gradient_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                                              _c_dp, _c_dp, ctypes.POINTER(SdfGrid),
                                                              ctypes.POINTER(CollisionParams), ctypes.c_double, _c_dp,
                                                              _c_dp, _c_dp, _c_dp, ctypes.c_int]),
    "mtg_soft_constraint_cost_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                      ctypes.c_int64, _c_dp, _c_dp, _c_dp,
                                                      ctypes.POINTER(SoftConstraintParams), _c_dp, _c_dp, _c_dp, _c_dp,
                                                      ctypes.c_uint]),
    "mtg_host_soft_constraint_cost_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                                           _c_dp, _c_dp, _c_dp, ctypes.POINTER(SoftConstraintParams),
                                                           _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_int]),
    "mtg_objective_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                           _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_int64, ctypes.POINTER(ObjectiveParams),
                                           ctypes.POINTER(SdfGrid), ctypes.POINTER(CollisionParams),
                                           ctypes.POINTER(SoftConstraintParams), _c_dp, _c_dp, _c_dp, _c_dp, _c_dp,
                                           ctypes.POINTER(ObjectiveParts), _c_dp, ctypes.c_uint]),
    "mtg_host_objective_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                                _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_int64,
                                                ctypes.POINTER(ObjectiveParams), ctypes.POINTER(SdfGrid),
                                                ctypes.POINTER(CollisionParams), ctypes.POINTER(SoftConstraintParams),
                                                _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, ctypes.POINTER(ObjectiveParts), _c_dp,
                                                ctypes.c_int]),
    "mtg_host_objective_bounds_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64, _c_dp,
                                                       ctypes.c_int, _c_dp, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                                       ctypes.POINTER(SoftConstraintParams), _c_dp, _c_dp,
                                                       ctypes.c_double, _c_dp, _c_dp, _c_dp]),
    "mtg_objective_time_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_int64, _c_dp, _c_dp, _c_dp, ctypes.c_int64,
                                                ctypes.POINTER(ObjectiveTimeParams), _c_dp, ctypes.POINTER(SdfGrid),
                                                ctypes.POINTER(CollisionParams), ctypes.POINTER(SoftConstraintParams),
                                                _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp,
                                                ctypes.POINTER(ObjectiveParts), _c_dp, ctypes.c_uint]),
    "mtg_host_objective_time_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64, _c_dp,
                                                     _c_dp, _c_dp, ctypes.c_int64, ctypes.POINTER(ObjectiveTimeParams),
                                                     _c_dp, ctypes.POINTER(SdfGrid), ctypes.POINTER(CollisionParams),
                                                     ctypes.POINTER(SoftConstraintParams), _c_dp, _c_dp, _c_dp, _c_dp,
                                                     _c_dp, _c_dp, _c_dp, _c_dp, ctypes.POINTER(ObjectiveParts), _c_dp,
                                                     ctypes.c_int]),
    "mtg_host_objective_time_bounds_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                                            _c_dp, ctypes.c_int, _c_dp, ctypes.c_int64, ctypes.c_double,
                                                            _c_dp, _c_dp, _c_dp]),
    "mtg_time_jacobian_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_int64, _c_dp, _c_dp, ctypes.c_int, _c_dp,
                                               ctypes.c_double, _c_dp, _c_dp, ctypes.c_uint]),
    "mtg_coefficients_from_vertices_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                            ctypes.c_int64, _c_dp, _c_dp, _c_dp, ctypes.c_uint]),
    "mtg_vertex_derivatives_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                    ctypes.c_int64, _c_dp, _c_dp, _c_dp, ctypes.c_uint]),
    "mtg_min_max_magnitude_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                   ctypes.c_int64, _c_dp, _c_dp, ctypes.c_int, ctypes.c_uint32,
                                                   _c_dp, _c_dp, ctypes.c_uint]),
    "mtg_last_kernel_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]),
    "mtg_enable_timing": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "mtg_kernel_times": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.c_int,
                                        ctypes.POINTER(ctypes.c_int)]),
    "mtg_host_solve_linear_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                   ctypes.c_int64, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp,
                                                   _c_dp, _c_dp, ctypes.c_int]),
    "mtg_host_default_threads": (ctypes.c_int, []),
    "mtg_host_min_max_magnitude_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                                        _c_dp, _c_dp, ctypes.c_int, ctypes.c_uint32, _c_dp, _c_dp,
                                                        ctypes.c_int]),
    "mtg_segment_min_max_magnitude_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                                           _c_dp, _c_dp, _c_dp, ctypes.c_int, ctypes.c_uint32, _c_dp,
                                                           _c_dp, _c_dp, _c_dp, ctypes.c_int, _c_dp, ctypes.c_uint]),
    "mtg_segment_min_max_axis_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                                      _c_dp, _c_dp, _c_dp, ctypes.c_int, _c_dp, _c_dp, _c_dp, _c_dp,
                                                      ctypes.c_int, _c_dp, ctypes.c_uint]),
    "mtg_host_segment_min_max_magnitude_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, _c_dp,
                                                                _c_dp, _c_dp, ctypes.c_int, ctypes.c_uint32, _c_dp,
                                                                _c_dp, _c_dp, _c_dp, ctypes.c_int, _c_dp,
                                                                ctypes.c_int]),
    "mtg_host_segment_min_max_axis_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, _c_dp, _c_dp,
                                                           _c_dp, ctypes.c_int, _c_dp, _c_dp, _c_dp, _c_dp,
                                                           ctypes.c_int, _c_dp, ctypes.c_int]),
    "mtg_host_estimate_segment_times": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _c_dp, ctypes.c_double,
                                                       ctypes.c_double, ctypes.c_double, _c_dp]),
    "mtg_host_segment_matrices": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_double, _c_dp, _c_dp,
                                                 _c_dp, _c_dp]),
    "mtg_host_coefficients_from_vertices_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                                 ctypes.c_int64, _c_dp, _c_dp, _c_dp,
                                                                 ctypes.c_int]),
    "mtg_host_random_vertices_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                      _c_dp, _c_dp, ctypes.c_uint32, ctypes.c_int64,
                                                      ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                                      _c_dp, _c_dp, _c_dp, ctypes.c_int]),
    "mtg_host_random_vertices_path_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                           ctypes.c_double, ctypes.c_int, ctypes.c_uint32,
                                                           ctypes.c_int64, ctypes.c_double, ctypes.c_double,
                                                           ctypes.c_double, _c_dp, _c_dp, _c_dp,
                                                           ctypes.c_int]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


class MTGError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("%s (code %d)" % (message, code))
        self.code = code


def hip_runtimes_mapped():
    """Paths of the libamdhip64 images mapped into this process (Linux)."""
    found = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                p = line.split()[-1]
                if "libamdhip64.so" in os.path.basename(p):
                    found.add(os.path.realpath(p))
    except OSError:
        pass
    return sorted(found)


def _share_torch_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64 (soname libamdhip64.so.7, the
    same as /opt/rocm's).  Loading torch first makes the dynamic linker bind the library's
    libamdhip64.so.7 dependency to torch's already-loaded copy, so the process has ONE
    HIP runtime: torch stream handles and allocations are then valid in the library.  Loading
    the library first would map /opt/rocm's runtime and torch would later map a second one,
    whose streams/devices the library cannot see.  Set MTG_NO_TORCH=1 to skip (torch-free use)."""
    if os.environ.get("MTG_NO_TORCH") == "1":
        return
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def load(path=None):
    """Load the library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("MTG_LIBRARY", LIB_PATH)
    if not os.path.exists(p):
        raise MTGError(MTG_ERR_NO_DEVICE, "libmav_trajectory_generation.so not found at %s: run __graft_entry__.build()" % p)
    _share_torch_runtime()
    lib = ctypes.CDLL(p)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def status_string(code):
    return load().mtg_status_string(code).decode()


def check(code, ctx=None):
    if code != MTG_OK:
        msg = status_string(code)
        if ctx is not None:
            detail = load().mtg_last_error(ctx)
            if detail:
                msg += ": " + detail.decode()
        raise MTGError(code, msg)
    return code


def solve_kernel(N, D, K, r, flags=0, B=None):
    """Name of the solve kernel mtg_solve_linear_batch runs for this shape (mtg_solve_kernel), or for a
    batch of B trajectories (mtg_solve_kernel_batch: the default depends on B)."""
    lib = load()
    code = lib.mtg_solve_kernel(N, D, K, r, flags) if B is None else lib.mtg_solve_kernel_batch(N, D, K, r, B, flags)
    if code < 0:
        raise MTGError(code, status_string(code))
    return KERNEL_NAMES[code]


def evaluate_at_path(N, D, K, M, n_derivatives=1):
    """The kernel mtg_evaluate_at_batch runs for this shape (mtg_evaluate_at_path): MTG_EVALUATE_AT_LANE or
    MTG_EVALUATE_AT_STAGED.  Depends on the shape only."""
    code = load().mtg_evaluate_at_path(N, D, K, M, n_derivatives)
    if code < 0:
        raise MTGError(code, status_string(code))
    return code


def evaluate_at_ragged_path(N, D, K_max, M, n_derivatives=1):
    """The kernel mtg_evaluate_at_ragged_batch runs for a batch whose largest segment count is K_max
    (mtg_evaluate_at_ragged_path): the rule of evaluate_at_path at K = K_max."""
    code = load().mtg_evaluate_at_ragged_path(N, D, K_max, M, n_derivatives)
    if code < 0:
        raise MTGError(code, status_string(code))
    return code


def device_count():
    n = ctypes.c_int(0)
    rc = load().mtg_device_count(ctypes.byref(n))
    return n.value if rc == MTG_OK else 0
