"""The ragged solve without a GPU: the plan (mtg_solve_ragged_plan), the host path
(mtg_host_solve_linear_ragged_batch) against mtg_host_solve_linear_batch called per trajectory, the
Python helpers, and the C++ solveRagged overloads (compiled and linked only: the class creates a context).

The contract under test (include/mtg.h): every output byte of trajectory b equals what the uniform
call writes for that trajectory alone, whatever the order of the batch and the other trajectories."""
import ctypes
import os

import numpy as np
import pytest

import mav_trajectory_generation_cmake_amd as mtg
from mav_trajectory_generation_cmake_amd import _native as nat
from _ragged_cases import order_of, per_k_batches, ragged_of, views_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plan(seg, N=10, D=3, r=4):
    p = mtg.solve_ragged_plan(N, D, r, seg)
    return p["n_groups"], p["n_in_place"], p["total_segments"]


def test_plan_counts():
    assert _plan([2, 2, 3, 5, 5, 7]) == (4, 6, 24)            # sorted: everything in place
    assert _plan([5, 2, 7, 2, 5, 3]) == (4, 2, 24)            # shuffled: only the single-member groups
    assert _plan([10] * 7) == (1, 7, 70)                       # one group
    assert _plan([2, 3, 3, 3, 2, 5, 2]) == (3, 4, 20)         # K = 3 is one run among groups that are not
    assert _plan([9, 4, 4, 9]) == (2, 2, 26)
    assert _plan([1]) == (1, 1, 1)
    assert _plan([]) == (0, 0, 0)                              # batch = 0
    # a descending batch is also one run per group
    assert _plan([7, 7, 5, 2, 2]) == (3, 5, 23)


def _plan_rc(N, D, r, seg, batch=None):
    lib = nat.load()
    a = None if seg is None else np.ascontiguousarray(seg, dtype=np.int32)
    g = ctypes.c_int64(-1)
    return lib.mtg_solve_ragged_plan(N, D, r, len(a) if batch is None else batch, None if a is None else a.ctypes.data,
                                     0, ctypes.byref(g), None, None)


def test_plan_errors():
    assert _plan_rc(10, 3, 4, [2, 0, 3]) == nat.MTG_ERR_SIZE_MISMATCH
    assert _plan_rc(10, 3, 4, [2, -1, 3]) == nat.MTG_ERR_SIZE_MISMATCH
    assert _plan_rc(10, 3, 4, None, batch=3) == nat.MTG_ERR_INVALID_ARGUMENT
    assert _plan_rc(10, 3, 4, None, batch=0) == nat.MTG_OK
    assert _plan_rc(14, 3, 4, [2, 3]) == nat.MTG_ERR_UNSUPPORTED_N
    assert _plan_rc(10, 3, 5, [2, 3]) == nat.MTG_ERR_BAD_DERIVATIVE
    assert _plan_rc(10, 0, 4, [2, 3]) == nat.MTG_ERR_SIZE_MISMATCH
    assert _plan_rc(10, 3, 4, [2], batch=-1) == nat.MTG_ERR_SIZE_MISMATCH
    # the uniform call's own limit, per K that is present (mtg_solve_kernel)
    big = 1 << 20
    assert nat.load().mtg_solve_kernel(10, 3, big, 4, 0) == nat.MTG_ERR_TOO_LARGE
    assert _plan_rc(10, 3, 4, [2, big]) == nat.MTG_ERR_TOO_LARGE
    # the host path reports the same argument errors (it has no size limit)
    lib = nat.load()
    z = np.zeros(64)
    m = np.zeros(64, np.uint8)
    seg = np.array([2, 0], np.int32)

    def host(N, D, r, B, segp):
        return lib.mtg_host_solve_linear_ragged_batch(N, D, r, B, segp, z.ctypes.data, m.ctypes.data, z.ctypes.data,
                                                      z.ctypes.data, None, None, None, None, 1)
    assert host(10, 1, 4, 2, seg.ctypes.data) == nat.MTG_ERR_SIZE_MISMATCH
    assert host(10, 1, 4, 2, None) == nat.MTG_ERR_INVALID_ARGUMENT
    assert host(14, 1, 4, 2, seg.ctypes.data) == nat.MTG_ERR_UNSUPPORTED_N
    assert host(10, 1, 4, 0, None) == nat.MTG_OK


# K = 1 is accepted by the generators (two vertices, both fixed to the highest derivative)
KS = (1, 2, 3, 5, 10, 11, 20, 37)


def _host_batches(N, D):
    counts = {K: 3 for K in KS}
    counts[3] = counts[10] = 4
    b = per_k_batches(N, D, counts, seed0=11 * N + D, kinds={3: "mixed", 10: "vel"})
    b = {K: tuple(a.copy() for a in v) for K, v in b.items()}
    b[5][2][1, 2] = -1.0          # a non-positive time: MTG_TRAJ_BAD_TIME
    b[11][2][0, 4] = 0.0
    b[2][1][2, 1] |= 0x80         # a mask bit >= h: MTG_TRAJ_WARN_DROPPED
    return b


def _per_trajectory_reference(N, r, batches):
    """reference[K][name][i]: mtg_host_solve_linear_batch with batch 1 on every trajectory."""
    ref = {}
    for K, (v, m, t) in batches.items():
        rows = [mtg.host_solve_linear_batch(N, r, v[i:i + 1], m[i:i + 1], t[i:i + 1], free=True, n_free=True, cost=True,
                                            status=True, threads=1) for i in range(v.shape[0])]
        ref[K] = {k: [row[k][0] for row in rows] for k in rows[0]}
    return ref


@pytest.fixture(scope="module")
def host_cases():
    cache = {}

    def get(N, D):
        if (N, D) not in cache:
            b = _host_batches(N, D)
            cache[(N, D)] = (b, _per_trajectory_reference(N, N // 2 - 1, b))
        return cache[(N, D)]
    return get


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("N", [4, 6, 10, 12])
def test_host_ragged_equals_uniform_per_trajectory(host_cases, N, D, threads):
    batches, ref = host_cases(N, D)
    order = order_of(batches, "shuffled", seed=N + D)
    values, mask, times, seg = ragged_of(batches, order)
    out = mtg.host_solve_linear_ragged_batch(N, N // 2 - 1, values, mask, times, seg, free=True, n_free=True, cost=True,
                                             status=True, threads=threads)
    got = views_of(out, seg, D)
    seen = 0
    for b, (K, i) in enumerate(order):
        for name in ("coeffs", "free", "n_free", "cost", "status"):
            np.testing.assert_array_equal(np.asarray(got[name][b]), np.asarray(ref[K][name][i]).reshape(np.shape(got[name][b])),
                                          err_msg="%s of trajectory %d (K = %d)" % (name, b, K))
        seen |= int(got["status"][b])
    # the special trajectories are in the batch and show their bits
    assert seen & nat.MTG_TRAJ_BAD_TIME and seen & nat.MTG_TRAJ_WARN_DROPPED


def test_order_independence(host_cases):
    N, D = 10, 3
    batches, _ = host_cases(N, D)
    res = {}
    for how, seed in (("shuffled", 1), ("shuffled", 2), ("sorted", 0)):
        order = order_of(batches, how, seed=seed)
        values, mask, times, seg = ragged_of(batches, order)
        out = mtg.host_solve_linear_ragged_batch(N, 4, values, mask, times, seg, free=True, n_free=True, cost=True,
                                                 status=True, threads=2)
        got = views_of(out, seg, D)
        res[(how, seed)] = {key: {k: np.asarray(got[k][b]).tobytes() for k in got} for b, key in enumerate(order)}
    first = res[("shuffled", 1)]
    assert res[("shuffled", 2)] == first and res[("sorted", 0)] == first


def test_free_out_blocks_and_every_element_written(host_cases):
    """Prefilled with NaN, every element of every requested output is written; in a free_out block the
    entries beyond n_free are +0.0 and the entries below it belong to that trajectory alone."""
    N, D, r = 10, 3, 4
    h = N // 2
    batches, ref = host_cases(N, D)
    order = order_of(batches, "shuffled", seed=5)
    values, mask, times, seg = ragged_of(batches, order)
    B, totS = len(seg), int(seg.sum())
    totV = totS + B
    coeffs = np.full((totS, D, N), np.nan)
    free = np.full((totV * h * D,), np.nan)
    cost = np.full((B,), np.nan)
    n_free = np.full((B,), -7, np.int32)
    status = np.full((B,), -7, np.int32)
    rc = nat.load().mtg_host_solve_linear_ragged_batch(N, D, r, B, seg.ctypes.data, values.ctypes.data, mask.ctypes.data,
                                                       times.ctypes.data, coeffs.ctypes.data, free.ctypes.data,
                                                       n_free.ctypes.data, cost.ctypes.data, status.ctypes.data, 3)
    assert rc == nat.MTG_OK
    assert (n_free != -7).all() and (status != -7).all()
    ok = (status & nat.MTG_TRAJ_ERROR_MASK) == 0
    fr = mtg.split_ragged(free, seg, "free", D=D)
    co = mtg.split_ragged(coeffs, seg, "coeffs")
    assert sum(f.size for f in fr) == free.size          # the blocks tile the array: no gap, no overlap
    for b, (K, i) in enumerate(order):
        assert fr[b].shape == (D, (K + 1) * h)
        if ok[b]:
            assert not np.isnan(fr[b]).any() and not np.isnan(co[b]).any() and not np.isnan(cost[b])
        tail = fr[b][:, n_free[b]:]
        assert (tail == 0.0).all() and not np.signbit(tail).any()
        # the block is this trajectory's, not a neighbour's
        np.testing.assert_array_equal(fr[b], ref[K]["free"][i])


def test_helpers_round_trip():
    rng = np.random.default_rng(0)
    seg = [3, 1, 4, 1, 5]
    vo, so = mtg.ragged_offsets(seg)
    np.testing.assert_array_equal(vo, [0, 4, 6, 11, 13, 19])
    np.testing.assert_array_equal(so, [0, 3, 4, 8, 9, 14])
    assert vo.dtype == np.int64 and so.dtype == np.int64
    h, D, N = 3, 2, 6
    problems = [(rng.normal(size=(K + 1, h, D)), rng.integers(0, 8, size=K + 1).astype(np.uint8), rng.random(K) + 0.5)
                for K in seg]
    values, mask, times, sc = mtg.pack_ragged(problems)
    assert sc.dtype == np.int32 and list(sc) == seg
    assert values.shape == (19, h, D) and mask.shape == (19,) and times.shape == (14,)
    for kind, arr, idx in (("values", values, 0), ("mask", mask, 1), ("times", times, 2)):
        parts = mtg.split_ragged(arr, sc, kind)
        for b, p in enumerate(parts):
            np.testing.assert_array_equal(p, problems[b][idx])
            assert np.shares_memory(p, arr)                 # views, not copies
    coeffs = rng.normal(size=(14, D, N))
    for b, p in enumerate(mtg.split_ragged(coeffs, sc, "coeffs")):
        assert p.shape == (seg[b], D, N) and np.shares_memory(p, coeffs)
    free = rng.normal(size=(19 * h * D,))
    parts = mtg.split_ragged(free, sc, "free", D=D)
    assert [p.shape for p in parts] == [(D, (K + 1) * h) for K in seg]
    np.testing.assert_array_equal(np.concatenate([p.reshape(-1) for p in parts]), free)
    assert mtg.split_ragged(np.arange(5), sc, "cost") == [0, 1, 2, 3, 4]
    # a run of equal K in the CSR arrays is a uniform array
    v2, m2, t2, s2 = mtg.pack_ragged([problems[1], problems[3]])
    np.testing.assert_array_equal(v2.reshape(2, 2, h, D)[1], problems[3][0])


def test_cpp_solve_ragged_compiles_and_links():
    """tests/cpp/test_ragged.cpp calls both solveRagged overloads; built against the library by the CMake
    project.  Not run here: BatchPolynomialOptimization creates a context (tests/test_gpu_ragged.py runs it)."""
    from test_cpp_api import _cmake_build
    _cmake_build()
    assert os.path.exists(os.path.join(ROOT, "build", "test_ragged"))
