"""The per-segment extremum entries without a GPU: mtg_host_segment_min_max_magnitude_batch and
mtg_host_segment_min_max_axis_batch (include/mtg.h) -- Segment::computeMinMaxMagnitudeCandidates +
selectMinMaxMagnitudeFromCandidates and Polynomial::computeMinMax on a window, with the candidate list.
The checks live in _segment_extrema_cases.py and run again on the device in test_gpu_segment_extrema.py.
CPU only."""
import numpy as np
import pytest

from mav_trajectory_generation_cmake_amd import _native as nat
import _segment_extrema_cases as cases
from _segment_extrema_cases import HostApi


@pytest.mark.parametrize("K", [1, 3, 10])
@pytest.mark.parametrize("explicit_windows", [False, True])
def test_reduced_segments_equal_the_uniform_host_entry(K, explicit_windows):
    """B = 7, N = 10, D = 3: S = 7, 21, 70 segments; derivatives 1 and 2; all dimensions, {0, 1} and {2}; bit
    equality of time, value and segment with mtg_host_min_max_magnitude_batch, with windows = NULL and with
    explicit [0, T] windows."""
    coeffs, times = cases.solved(K)
    for derivative in (1, 2):
        for dims in (None, [0, 1], [2]):
            cases.check_equals_uniform_entry(HostApi, coeffs, times, derivative, dims, explicit_windows,
                                             (K, derivative, dims))


def test_constructed_roots():
    """Exact counts, the ends first, ascending roots, a +0.0 tail, extremes within 1e-9 of the exact evaluation;
    root times within HOST_ROOT_TIME_ERR of the constructed roots (the value measured here, on this fixture:
    see _segment_extrema_cases.py)."""
    cases.check_constructed_roots(HostApi, cases.HOST_ROOT_TIME_ERR)


def test_magnitude_against_the_oracle_roots():
    from oracle import pyoracle
    cases.check_against_oracle(HostApi, pyoracle)


def test_windows():
    cases.check_windows(HostApi)


def test_ties_and_the_zero_polynomial():
    cases.check_ties_and_zero_polynomial(HostApi)


def test_independence_of_the_batch():
    cases.check_independence(HostApi)


def test_other_shapes_equal_the_uniform_host_entry():
    cases.check_shapes_against_uniform(HostApi)


def test_capacity_and_nullable_outputs():
    cases.check_capacity_and_nullable_outputs(HostApi)


def test_threads_do_not_change_the_bytes():
    coeffs, times, _ = cases.ragged_batch()
    one = HostApi.axis(coeffs, times, 1, candidate_capacity=6, threads=1)
    cases.assert_same_outputs(HostApi.axis(coeffs, times, 1, candidate_capacity=6, threads=4), one)


def test_argument_errors():
    lib = nat.load()
    cases.check_argument_errors(lambda *a: lib.mtg_host_segment_min_max_magnitude_batch(*a, 1),
                                lambda *a: lib.mtg_host_segment_min_max_axis_batch(*a, 1))
    # the device entries reject a NULL context before anything else
    z = np.zeros(64)
    a = z.ctypes.data
    assert lib.mtg_segment_min_max_magnitude_batch(None, 10, 3, 1, a, a, None, 1, 0, a, a, None, None, 0, None,
                                                   0) == nat.MTG_ERR_INVALID_ARGUMENT
    assert lib.mtg_segment_min_max_axis_batch(None, 10, 3, 1, a, a, None, 1, a, a, None, None, 0, None,
                                              0) == nat.MTG_ERR_INVALID_ARGUMENT
