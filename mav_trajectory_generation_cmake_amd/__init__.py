"""MI355X-native batched minimum-derivative polynomial trajectory optimizer.

Drop-in for the linear solve path of magrimm/mav_trajectory_generation_cmake
(PolynomialOptimization<N>::setupFromVertices + solveLinear, and
Trajectory::evaluateRange).  The compute path is hand-written HIP for gfx950
behind a C ABI (include/mtg.h, lib/libmav_trajectory_generation.so); this package is a thin Python
host layer over that ABI.  See DESIGN.md.
"""
from . import _native
from ._native import MTGError, device_count, load, solve_kernel
from .solver import (OBJECTIVE_STATE_DTYPE, ObjectiveParams, ObjectiveTimeParams, host_objective_batch, host_objective_bounds_batch, host_objective_time_batch, host_objective_time_bounds_batch, number_of_free_constraints, pack_optimization_variables, unpack_optimization_variables, CollisionParams, Context, SdfGrid, SoftConstraintParams, collision_cost_batch, collision_time_gradient_batch, time_gradient_batch, host_collision_time_gradient_batch, soft_constraint_cost_batch, host_soft_constraint_cost_batch, default_context, host_collision_cost_batch, full_vertex_values, host_evaluate_at_batch, host_min_max_magnitude_batch, host_solve_linear_batch, random_vertices_batch,
                     random_vertices_path_batch, shard_range, solve_linear_batch, solve_linear_batch_multi,
                     host_solve_linear_ragged_batch, pack_ragged, ragged_offsets, solve_ragged_plan, split_ragged,
                     host_evaluate_at_ragged_batch, host_min_max_magnitude_ragged_batch, join_ragged,
                     extrema_from_bytes, host_segment_min_max_magnitude_batch, host_segment_min_max_axis_batch,
                     host_vertex_derivatives_batch, host_vertex_derivatives_ragged_batch,
                     host_coefficients_from_vertices_ragged_batch, host_collision_cost_ragged_batch)

__all__ = ["MTGError", "OBJECTIVE_STATE_DTYPE", "ObjectiveParams", "ObjectiveTimeParams", "host_objective_batch", "host_objective_bounds_batch", "host_objective_time_batch", "host_objective_time_bounds_batch", "number_of_free_constraints", "pack_optimization_variables", "unpack_optimization_variables", "CollisionParams", "Context", "SdfGrid", "SoftConstraintParams", "collision_cost_batch", "collision_time_gradient_batch", "time_gradient_batch", "host_collision_time_gradient_batch", "soft_constraint_cost_batch", "host_soft_constraint_cost_batch", "host_collision_cost_batch", "default_context", "device_count", "full_vertex_values", "host_evaluate_at_batch", "host_min_max_magnitude_batch",
           "host_solve_linear_batch",
           "load",
           "random_vertices_batch",
           "random_vertices_path_batch", "shard_range", "solve_kernel", "solve_linear_batch",
           "solve_linear_batch_multi", "host_solve_linear_ragged_batch", "pack_ragged", "ragged_offsets",
           "solve_ragged_plan", "split_ragged", "host_evaluate_at_ragged_batch", "host_min_max_magnitude_ragged_batch",
           "join_ragged", "extrema_from_bytes", "host_segment_min_max_magnitude_batch",
           "host_segment_min_max_axis_batch", "host_vertex_derivatives_batch", "host_vertex_derivatives_ragged_batch",
           "host_coefficients_from_vertices_ragged_batch", "host_collision_cost_ragged_batch",
           "_native"]
