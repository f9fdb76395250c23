"""Every (N, r) of the solve against 60-digit truth on the CPU (no GPU): the condition on the inputs of
the truth grid (tests/_solve_truth_cases.py), the library's host path on every case at the GPU test's
tolerances (tests/test_gpu_solve_truth.py), and the written kernel map against mtg_solve_kernel.

The condition is checked against an independent reference, not the project's solver: the best FP64
solve of every generated problem (make_golden.fp64_best_solve: the 60-digit system rounded once, LAPACK)
is within BEST_TOL = 2.5e-10 of truth, a quarter of the 1e-9 gate.  Measured over this grid: worst
6.5e-11, at (N, r) = (12, 0).  If a seed breaks it, the seed changes, not the gate (_RESEED in
_solve_truth_cases.py lists the one draw that did).

The host path (mtg_host_solve_linear_batch) is another implementation of the kernels' algorithm: the
CPU-side pin of all 21 (N, r).  Measured over this grid: coefficients <= 1.7e-10 (worst at (12, 0)),
cost <= 4.5e-12 relative (at (12, 5)), free values <= 2.5e-10 (at (12, 0)); per (N, r): DESIGN.md 4.
"""
import numpy as np
import pytest

import _solve_truth_cases as C
from _util import scale_normalised_error

B_HOST = 5  # three replicas of problem 0, two of problem 1


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("N,r", C.NR)
def test_inputs_well_conditioned_and_host_path_vs_truth(N, r, kind):
    import mav_trajectory_generation_cmake_amd as mtg
    worst_best = worst_host = 0.0
    for K, D in C.shapes(N, r):
        vals, mask, times, tr = C.batch(N, r, K, D, kind, B_HOST)
        where = (N, r, K, D, kind)
        best = scale_normalised_error(tr["best"], tr["coeffs"], times[:C.PROBLEMS])
        worst_best = max(worst_best, best)
        assert best <= C.BEST_TOL, (where, "the best FP64 solve against truth", best)
        out = mtg.host_solve_linear_batch(N, r, vals, mask, times, free=True, n_free=True, cost=True, status=True)
        worst_host = max(worst_host, C.check_outputs(out, N, times, tr, where))
    print("solve truth host N=%d r=%d %-7s best FP64 %.1e host %.1e" % (N, r, kind, worst_best, worst_host))


def test_every_lane_width_and_bucket_edge_is_visited():
    """The grid's own coverage: every (N, r) runs the column kernel at 8, 16 and 32 lanes per chain
    (shapes() asserts it), at K == KMAX of every bucket, and visits the K on both sides of every bucket
    edge; the DL shapes at every D in 1..4; and the K the column kernel's register bound excludes
    (N = 10: 11, 12; N = 12: 9..12)."""
    for N, r in C.NR:
        sh = C.shapes(N, r)
        Ks = {K for K, _ in sh}
        assert {1, 3, 4, 8, 10, 12, 13} <= Ks and (N <= 4 or {5, 9, 11, 20, 21} <= Ks)
        assert {C.lanes_per_chain(N, D) for K, D in sh if C.column_shape(N, D, K)} == {8, 16, 32}
        if N in C.DL_SHAPES:
            assert {D for K, D in sh if K == C.DL_SHAPES[N]} == {1, 2, 3, 4}
    # the long-chain kernel meets each of its D at every N it serves
    for N in (6, 8, 10, 12):
        seen = {D for r in range(1, N // 2) for K, D in C.shapes(N, r)
                if C.expected_kernel(N, D, K, r, "default") == C.DLX}
        assert seen == {1, 2, 3, 4}, (N, seen)


def test_written_kernel_map_is_the_library_s():
    """expected_kernel (the map of DESIGN.md 3.0, written out from the documents) names the kernel
    mtg_solve_kernel[_batch] reports, at every (N, D, K, r, path) the grid visits -- N = 10 with K = 11, 12
    and N = 12 with K = 9..12, which are not column shapes, among them."""
    from mav_trajectory_generation_cmake_amd import _native as nat
    flag = {"default": 0, "general": nat.MTG_FLAG_GENERAL_KERNEL, "split": nat.MTG_FLAG_SPLIT_KERNELS,
            "dl": nat.MTG_FLAG_DL_KERNEL, "column": nat.MTG_FLAG_COLUMN_KERNEL}
    visited = 0
    for N, r in C.NR:
        for K, D in C.shapes(N, r):
            for path in C.PATHS:
                want = C.expected_kernel(N, D, K, r, path)
                assert nat.solve_kernel(N, D, K, r, flag[path], B=37) == want, (N, D, K, r, path)
                assert nat.solve_kernel(N, D, K, r, flag[path]) == want, (N, D, K, r, path)
                visited += 1
    assert visited == 5 * sum(len(C.shapes(N, r)) for N, r in C.NR)
    for K in (11, 12):
        assert C.expected_kernel(10, 3, K, 4, "default") == C.DLX and C.expected_kernel(10, 3, K, 4, "column") == C.GENERAL
    for K in (9, 10, 11, 12):
        assert C.expected_kernel(12, 3, K, 3, "default") == C.DLX and C.expected_kernel(12, 3, K, 0, "default") == C.GENERAL
