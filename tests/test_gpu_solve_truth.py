"""Every solve kernel instantiation against 60-digit truth over the (N, r, K, D) grid
(tests/_solve_truth_cases.py): all 21 (N, r), the K on both sides of every bucket edge of the column
kernel and at every KMAX (the interior-waypoint body: kind "pattern" at K == KMAX; the general body: the
other kinds and K), the DL shapes at every D in 1..4, the long-chain kernel at each of its D, the column
kernel at 8, 16 and 32 lanes per chain, and the general and split paths everywhere.

The FP64 oracle cannot stand in for truth here (it is 1e-5 from truth at (10, 0) and 1e-2 at (12, 0) on
these well-conditioned inputs), so truth is computed at test time (make_golden.truth_solve_banded,
mpmath at 60 digits; about 5 s of it for an N = 12 test, well under 1 s for N <= 6), once per (K, D, kind),
and shared by the five paths.  The inputs' condition -- the best FP64 solve within a quarter of the gate
of truth on every problem -- is asserted on the CPU (tests/test_solve_truth_host.py), which is what lets
every trajectory be held to 1e-9 with no arbitration.

Each call solves B = 37 trajectories, the two truth problems cycled (b % 2): every block and wave has a
tail and mixed neighbours.  Per call (tests/_solve_truth_cases.check_outputs): the kernel the written
map names is the one the library reports; status 0 and n_free exact; coefficients within
1e-9 of truth scale-normalised and 1e-6 element-wise (on coefficients >= 1e-4 of the segment's scale);
cost within 1e-9 relative (truth's cost is > 0 in every case: asserted where truth is computed); free
values within 1e-7 of their dimension's largest; and the replicas of a problem bit-identical in every
output -- DESIGN's claim that a trajectory's bits do not depend on its place in the call.
"""
import numpy as np
import pytest

import _solve_truth_cases as C

pytestmark = pytest.mark.gpu

B = 37


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("N,r", C.NR)
def test_solve_vs_truth(gpu_ctx, N, r, kind):
    from mav_trajectory_generation_cmake_amd import _native as nat
    flag = {"default": 0, "general": nat.MTG_FLAG_GENERAL_KERNEL, "split": nat.MTG_FLAG_SPLIT_KERNELS,
            "dl": nat.MTG_FLAG_DL_KERNEL, "column": nat.MTG_FLAG_COLUMN_KERNEL}
    worst = dict.fromkeys(C.PATHS, 0.0)
    kernels = {p: set() for p in C.PATHS}
    for K, D in C.shapes(N, r):
        vals, mask, times, tr = C.batch(N, r, K, D, kind, B)
        for path, kw in C.PATHS.items():
            where = (N, r, K, D, kind, path)
            want = C.expected_kernel(N, D, K, r, path)
            assert nat.solve_kernel(N, D, K, r, flag[path], B=B) == want, where
            if path == "default":
                assert nat.solve_kernel(N, D, K, r) == want, where
            kernels[path].add(want)
            out = gpu_ctx.solve_linear_batch(N, r, vals, mask, times, free=True, n_free=True, cost=True, status=True,
                                             **kw)
            worst[path] = max(worst[path], C.check_outputs(out, N, times, tr, where))
    assert kernels["general"] == {C.GENERAL} and kernels["split"] == {C.SPLIT} and C.COLUMN in kernels["column"]
    print("solve truth gpu N=%d r=%d %-7s " % (N, r, kind) + " ".join("%s %.1e" % (p, worst[p]) for p in C.PATHS))
