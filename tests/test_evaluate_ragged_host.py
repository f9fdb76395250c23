"""The ragged evaluate_at and min / max magnitude without a GPU: the host paths
(mtg_host_evaluate_at_ragged_batch, mtg_host_min_max_magnitude_ragged_batch) against the uniform host
entries run on every packed K-group, the call-level errors of the host and the device entries, and the
Python helpers.  CPU only.

The contract under test (include/mtg.h): every output byte of trajectory b equals what the uniform entry
writes for that trajectory alone, whatever the order of the batch and the other trajectories."""
import numpy as np
import pytest

import mav_trajectory_generation_cmake_amd as mtg
import _evaluate_at_model as model
from mav_trajectory_generation_cmake_amd import _native as nat
from _evaluate_ragged_cases import (assert_same_evaluation, assert_same_extrema, check_call_level_errors, csr_of,
                                    evaluate_reference,
                                    min_max_reference, query_rows, shared_row, solved_groups, with_bad_times)
from _ragged_cases import order_of

N, D = 10, 3
COUNTS = {1: 3, 2: 4, 5: 5, 10: 3}
M = 24  # >= K + 7 for every K: each row holds all of its trajectory's edge times
# one trajectory with T_i = 0 and one with a NaN time: (K, index in the K-batch, segment) -> value
BAD = {(5, 1, 3): 0.0, (10, 2, 0): np.nan}


@pytest.fixture(scope="module")
def groups():
    return solved_groups(N, D, COUNTS, seed0=77)


@pytest.mark.parametrize("how", ["sorted", "shuffled"])
@pytest.mark.parametrize("threads", [1, 4])
def test_evaluate_at_equals_the_uniform_host_entry(groups, how, threads):
    """Shared and per-trajectory query rows; nd = 1 and nd = 3 from order 0; queries at t < 0, at every
    prefix boundary exactly, at the total, beyond it, +inf and NaN (query_rows)."""
    order = order_of(groups, how, seed=3)
    coeffs, times, seg = csr_of(groups, order)
    for tq in (query_rows(groups, order, M, seed=5), shared_row(groups, order, M, seed=5)):
        for k0, nd in ((0, 1), (0, 3), (2, 1)):
            got = mtg.host_evaluate_at_ragged_batch(coeffs, times, seg, tq, k0, nd, threads=threads)
            want = evaluate_reference(mtg.host_evaluate_at_batch, groups, order, tq, k0, nd)
            assert_same_evaluation(got, want, (how, threads, tq.ndim, k0, nd))
            assert not got[2].any()
    # the edge times did their work: some rows out of range, some NaN, most in range
    assert 0.0 < got[1].mean() < 1.0 and np.isnan(got[0]).any()


@pytest.mark.parametrize("how", ["sorted", "shuffled"])
def test_bad_time_trajectories_and_their_neighbours(groups, how):
    order = order_of(groups, how, seed=4)
    bad_groups = with_bad_times(groups, BAD)
    tq = query_rows(groups, order, M, seed=6)
    coeffs, times, seg = csr_of(bad_groups, order)
    got = mtg.host_evaluate_at_ragged_batch(coeffs, times, seg, tq, 0, 3)
    assert_same_evaluation(got, evaluate_reference(mtg.host_evaluate_at_batch, bad_groups, order, tq, 0, 3), how)
    bad = [b for b, (K, i) in enumerate(order) if any((K, i) == key[:2] for key in BAD)]
    good = [b for b in range(len(order)) if b not in bad]
    assert len(bad) == 2
    assert (got[2][bad] == nat.MTG_TRAJ_BAD_TIME).all() and np.isnan(got[0][bad]).all() and not got[1][bad].any()
    assert not got[2][good].any()
    clean = mtg.host_evaluate_at_ragged_batch(*csr_of(groups, order), tq, 0, 3)
    assert_same_evaluation([x[good] for x in got], [x[good] for x in clean], "neighbours of the bad trajectories")


def test_evaluate_at_against_the_definition(groups):
    """The numpy model of the definition (tests/_evaluate_at_model.py) per trajectory: equality with the
    uniform entry is not the only pin."""
    order = order_of(groups, "shuffled", seed=8)
    coeffs, times, seg = csr_of(groups, order)
    tq = query_rows(groups, order, M, seed=9)
    got = mtg.host_evaluate_at_ragged_batch(coeffs, times, seg, tq, 0, 3)
    for b, (K, i) in enumerate(order):
        want = model.evaluate_at(groups[K][0][i:i + 1], groups[K][1][i:i + 1], tq[b:b + 1], 0, 3)
        model.assert_same_bits(got[0][b:b + 1], want[0], (b, K))
        assert np.array_equal(got[1][b:b + 1], want[1]) and got[2][b] == want[2][0]


@pytest.mark.parametrize("how", ["sorted", "shuffled"])
@pytest.mark.parametrize("derivative", [1, 2])
@pytest.mark.parametrize("dimensions", [None, (0, 2)])
def test_min_max_equals_the_uniform_host_entry(groups, how, derivative, dimensions):
    order = order_of(groups, how, seed=10)
    coeffs, times, seg = csr_of(groups, order)
    for threads in (1, 4):
        got = mtg.host_min_max_magnitude_ragged_batch(coeffs, times, seg, derivative, dimensions, threads=threads)
        want = min_max_reference(mtg.host_min_max_magnitude_batch, groups, order, derivative, dimensions)
        assert_same_extrema(got[0], want[0], ("minimum", how, derivative, dimensions, threads))
        assert_same_extrema(got[1], want[1], ("maximum", how, derivative, dimensions, threads))
    assert (got[1]["value"] > got[0]["value"]).all()


def test_python_helpers_accept_per_trajectory_blocks(groups):
    """What split_ragged(..., "coeffs") / (..., "times") yield goes back in as it is."""
    order = order_of(groups, "shuffled", seed=12)
    coeffs, times, seg = csr_of(groups, order)
    tq = query_rows(groups, order, 5, seed=13)
    blocks = mtg.split_ragged(coeffs, seg, "coeffs")
    tblocks = mtg.split_ragged(times, seg, "times")
    assert [x.shape for x in blocks] == [(K, D, N) for K, _ in order]
    assert_same_evaluation(mtg.host_evaluate_at_ragged_batch(blocks, tblocks, seg, tq, 0, 2),
                           mtg.host_evaluate_at_ragged_batch(coeffs, times, seg, tq, 0, 2))
    a = mtg.host_min_max_magnitude_ragged_batch(blocks, tblocks, seg, 1)
    b = mtg.host_min_max_magnitude_ragged_batch(coeffs, times, seg, 1)
    assert_same_extrema(a[0], b[0])
    assert_same_extrema(a[1], b[1])
    np.testing.assert_array_equal(mtg.join_ragged(blocks), coeffs)
    # a list in place of the int32 array, and the path helper
    assert_same_evaluation(mtg.host_evaluate_at_ragged_batch(coeffs, times, [int(k) for k in seg], tq, 0, 2),
                           mtg.host_evaluate_at_ragged_batch(coeffs, times, seg, tq, 0, 2))
    assert nat.evaluate_at_ragged_path(10, 3, 13, 40) == nat.evaluate_at_path(10, 3, 13, 40) == nat.MTG_EVALUATE_AT_STAGED
    assert nat.evaluate_at_ragged_path(10, 3, 50, 40) == nat.MTG_EVALUATE_AT_LANE


def test_call_level_errors():
    """The host entries; then what the device entries report without a context."""
    check_call_level_errors(None)
    lib = nat.load()
    z = np.zeros(8)
    seg = np.array([2], np.int32)
    assert lib.mtg_evaluate_at_ragged_batch(None, N, D, 1, seg.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, 1,
                                            1, 0, 1, z.ctypes.data, None, None, 0) == nat.MTG_ERR_INVALID_ARGUMENT
    assert lib.mtg_min_max_magnitude_ragged_batch(None, N, D, 1, seg.ctypes.data, z.ctypes.data, z.ctypes.data, 1, 0,
                                                  z.ctypes.data, None, 0) == nat.MTG_ERR_INVALID_ARGUMENT
    assert lib.mtg_evaluate_at_ragged_path(11, 3, 10, 1, 1) == nat.MTG_ERR_UNSUPPORTED_N
    assert lib.mtg_evaluate_at_ragged_path(10, 3, 0, 1, 1) == nat.MTG_ERR_SIZE_MISMATCH
    assert lib.mtg_evaluate_at_ragged_path(12, 11, 10, 1, 12) == nat.MTG_ERR_TOO_LARGE


def test_ragged_kernels_have_no_fma_and_no_scratch(tmp_path):
    """The gfx950 code of the ragged unit, as test_kernels_have_no_fma holds the uniform unit: both
    mappings for every N, no f64 FMA (no contracted Horner step), no scratch."""
    import os
    import re
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found: the library under test cannot have been built here"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "mav_trajectory_generation_cmake_amd", "csrc")
    out = tmp_path / "mtg_evaluate_at_ragged.s"
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-I",
                    os.path.join(root, "include"), "-I", csrc, os.path.join(csrc, "mtg_evaluate_at_ragged.hip"), "-o",
                    str(out)], check=True, capture_output=True)
    asm = out.read_text()
    kernels = re.findall(r"^(_ZN3mtg\w*evaluate_at_\w+_kernel\w*):", asm, flags=re.M)
    assert len(kernels) == 12 and all("Lb1E" in k for k in kernels), kernels  # (lane, staged) x N, Ragged = true
    assert "v_mul_f64" in asm and "v_add_f64" in asm
    assert not re.search(r"v_fmac?_f64", asm)
    assert re.findall(r"\.private_segment_fixed_size: (\d+)", asm) == ["0"] * 12


def test_empty_calls_write_nothing():
    lib = nat.load()
    out = np.full(64, 7.0)
    seg = np.array([2, 1], np.int32)
    z = np.zeros(3 * D * N)
    assert lib.mtg_host_evaluate_at_ragged_batch(N, D, 0, None, None, None, None, 0, 4, 0, 1, out.ctypes.data, None, None,
                                                 1) == nat.MTG_OK
    assert lib.mtg_host_evaluate_at_ragged_batch(N, D, 2, seg.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, 0,
                                                 0, 0, 1, out.ctypes.data, None, None, 1) == nat.MTG_OK
    assert lib.mtg_host_min_max_magnitude_ragged_batch(N, D, 0, None, None, None, 1, 0, out.ctypes.data, out.ctypes.data,
                                                       1) == nat.MTG_OK
    assert (out == 7.0).all()
    o, r, s = mtg.host_evaluate_at_ragged_batch(np.zeros((0, D, N)), np.zeros(0), [], np.zeros(4))
    assert o.shape == (0, 4, 1, D) and r.shape == (0, 4) and s.shape == (0,)
