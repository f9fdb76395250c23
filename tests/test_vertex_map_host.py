"""mtg_host_coefficients_from_vertices_batch, the host twin of the device's coefficient map, against the
60-digit truth of tests/_vertex_map_model.py on the shapes of test_gpu_vertex_map.py and under the same
two metrics; the empty batch, the argument errors and the threads argument.  No GPU."""
import numpy as np
import pytest

from mav_trajectory_generation_cmake_amd import _native as nat

import _vertex_map_model as M
from _util import scale_normalised_error
from test_vertex_map_model import oracle_coefficients

TOL = 1e-9


def host_map(N, x, T, threads=1):
    x = np.ascontiguousarray(x, dtype=np.float64)
    T = np.ascontiguousarray(T, dtype=np.float64)
    B, V, h, D = x.shape
    out = np.full((B, V - 1, D, N), np.nan)
    nat.check(nat.load().mtg_host_coefficients_from_vertices_batch(N, D, V - 1, B, x.ctypes.data, T.ctypes.data,
                                                                   out.ctypes.data, threads))
    return out


@pytest.mark.parametrize("shape", M.SHAPES, ids=M.shape_id)
def test_host_map_against_truth(shape):
    case = M.coefficient_case(*shape)
    c = host_map(case["N"], case["x"], case["T"])
    full = scale_normalised_error(c, case["truth64"], case["T"])
    shp = M.shape_error(c, case["truth64"], case["T"])
    print("host vs truth %s: full %.2e shape %.2e" % (M.shape_id(shape), full, shp))
    assert full <= TOL and shp <= TOL, (full, shp)


@pytest.mark.parametrize("shape", M.OFFSET_SHAPES, ids=M.shape_id)
def test_host_map_keeps_the_shape_at_position_offset_1e8(shape):
    """The start position is subtracted from the end position before anything is scaled, so c_j for
    j >= 1 does not see a common offset.  The reference's FP64 Schur inverse (the oracle) has no such
    step; its error is printed beside the host's (DESIGN.md records both)."""
    case = M.coefficient_case(*shape, offset=M.OFFSET)
    c = host_map(case["N"], case["x"], case["T"])
    shp = M.shape_error(c, case["truth64"], case["T"])
    oracle = M.shape_error(oracle_coefficients(case), case["truth64"], case["T"])
    msg = "offset 1e8 %s shape metric: host %.2e, oracle %.2e" % (M.shape_id(shape), shp, oracle)
    print(msg)
    assert shp <= TOL, msg
    assert scale_normalised_error(c, case["truth64"], case["T"]) <= TOL


def test_host_map_times_too_large_for_the_device():
    """The host map has no K limit: the first K the device's map refuses."""
    for shape in M.TOO_LARGE:
        N, D, K, B = shape
        x, T, _ = M.inputs(*shape)
        c = host_map(N, x, T)
        b, segs = B - 1, [0, K // 2, K - 1]  # truth on three segments of the last trajectory
        for i in segs:
            truth = M.to_float(M.truth_coefficients(N, x[b, i:i + 2, :, :1], T[b, i:i + 1]))
            assert scale_normalised_error(c[b:b + 1, i:i + 1, :1], truth[None], T[b:b + 1, i:i + 1]) <= TOL, (shape, i)


def test_host_map_empty_batch_and_errors():
    lib = nat.load()
    f = lib.mtg_host_coefficients_from_vertices_batch
    x, T, _ = M.inputs(10, 3, 3, 2)
    out = np.full((2, 3, 3, 10), -7.0)
    ptrs = (x.ctypes.data, T.ctypes.data, out.ctypes.data)
    assert f(10, 3, 3, 0, *ptrs, 1) == nat.MTG_OK
    assert f(10, 3, 3, 0, None, None, None, 1) == nat.MTG_OK
    for N in (0, 1, 3, 11, 13, 14, -2):
        assert f(N, 3, 3, 2, *ptrs, 1) == nat.MTG_ERR_UNSUPPORTED_N, N
    for D, K, B in ((0, 3, 2), (-1, 3, 2), (3, 0, 2), (3, -1, 2), (3, 3, -1)):
        assert f(10, D, K, B, *ptrs, 1) == nat.MTG_ERR_SIZE_MISMATCH, (D, K, B)
    for i in range(3):
        bad = list(ptrs)
        bad[i] = None
        assert f(10, 3, 3, 2, *bad, 1) == nat.MTG_ERR_INVALID_ARGUMENT, i
    assert np.all(out == -7.0)  # nothing above wrote the output


def test_host_map_threads_change_no_byte_and_inputs_stay():
    shape = (10, 3, 10, 37)
    x, T, _ = M.inputs(*shape)
    x0, T0 = x.copy(), T.copy()
    ref = host_map(10, x, T, threads=1)
    assert not np.isnan(ref).any()
    for threads in (0, 2, 5, 64):
        assert host_map(10, x, T, threads=threads).tobytes() == ref.tobytes(), threads
    assert x.tobytes() == x0.tobytes() and T.tobytes() == T0.tobytes()
    # a trajectory's bytes do not depend on its place in the batch
    for b in (0, 17, 36):
        assert host_map(10, x[b:b + 1], T[b:b + 1]).tobytes() == ref[b].tobytes(), b
