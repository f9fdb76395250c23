"""The per-segment extremum kernel (csrc/mtg_segment_extrema.hip) through mtg_segment_min_max_magnitude_batch
and mtg_segment_min_max_axis_batch: the checks of _segment_extrema_cases.py on the device, the device
against the host path, and the device-pointer / async flags.

Bit equality with mtg_min_max_magnitude_batch holds because both kernels run mtg_extrema_common.h with
L = 8 lanes per segment and one staging pass: at K = 1, 3, 10 extrema_geometry gives L = 8 (K L <= 512)
and launch_extrema_nl keeps qd = min(ndim, 4) (the block's LDS is far below 64 KiB), which is the new
launcher's rule for every shape."""
import numpy as np
import pytest

import mav_trajectory_generation_cmake_amd as mtg
from mav_trajectory_generation_cmake_amd import _native as nat
from mav_trajectory_generation_cmake_amd.solver import EXTREMUM_DTYPE
import _segment_extrema_cases as cases

pytestmark = pytest.mark.gpu


class DeviceApi:
    def __init__(self, ctx):
        self.magnitude = ctx.segment_min_max_magnitude_batch
        self.axis = ctx.segment_min_max_axis_batch
        self.uniform = ctx.min_max_magnitude_batch


@pytest.fixture(scope="module")
def api(gpu_ctx):
    return DeviceApi(gpu_ctx)


@pytest.mark.parametrize("K", [1, 3, 10])
@pytest.mark.parametrize("explicit_windows", [False, True])
def test_reduced_segments_equal_the_uniform_kernel(api, K, explicit_windows):
    """B = 7: S = 7, 21 and 70 segments (70 leaves a partly filled tail wave: 8 full waves of 8 items and one
    of 6); derivatives 1 and 2; all dimensions, {0, 1} and {2}; time, value and segment bit for bit."""
    coeffs, times = cases.solved(K)
    for derivative in (1, 2):
        for dims in (None, [0, 1], [2]):
            cases.check_equals_uniform_entry(api, coeffs, times, derivative, dims, explicit_windows,
                                             (K, derivative, dims))


def test_constructed_roots(api):
    """Root times within 10 x the host path's measured worst error on this fixture (_segment_extrema_cases.py);
    counts equal to the host's."""
    dev = cases.check_constructed_roots(api, cases.DEVICE_ROOT_TIME_ERR)
    coeffs, windows, _ = cases.constructed()
    host = cases.HostApi.axis(coeffs, None, 1, windows, candidate_capacity=12)
    np.testing.assert_array_equal(dev["candidate_count"], host["candidate_count"])


def test_magnitude_against_the_oracle_roots(api):
    from oracle import pyoracle
    cases.check_against_oracle(api, pyoracle)


def test_windows(api):
    cases.check_windows(api)


def test_ties_and_the_zero_polynomial(api):
    cases.check_ties_and_zero_polynomial(api)


def test_independence_of_the_batch(api):
    cases.check_independence(api)


def test_other_shapes_equal_the_uniform_kernel(api):
    cases.check_shapes_against_uniform(api)


def test_capacity_and_nullable_outputs(api):
    cases.check_capacity_and_nullable_outputs(api)


def test_device_matches_host(api):
    """Values within 1e-11 of the host path (the bound of test_min_max_magnitude_gpu_matches_host: the kernel's
    Horner steps contract to FMA, the host's do not)."""
    coeffs, times, _ = cases.ragged_batch()
    w = np.stack([-0.05 * times, 0.9 * times], axis=1)
    for windows in (None, w):
        for name, args in (("magnitude", (coeffs, times, 1, None, windows)), ("magnitude", (coeffs, times, 2, [1], windows)),
                           ("axis", (coeffs, times, 0, windows)), ("axis", (coeffs, times, 2, windows))):
            g = getattr(api, name)(*args, candidate_capacity=10)
            h = getattr(cases.HostApi, name)(*args, candidate_capacity=10)
            scale = np.maximum(np.abs(h["maximum"]["value"]), np.abs(h["minimum"]["value"])).max()
            for key in ("minimum", "maximum"):
                assert np.max(np.abs(g[key]["value"] - h[key]["value"])) <= 1e-11 * scale, (name, key)
            np.testing.assert_array_equal(g["status"], h["status"])
            # (the counts are compared on the constructed fixture, whose roots are simple: a solved trajectory
            # rests at its ends, where the root polynomial has a multiple root that rounding may or may not show)
            assert (g["candidate_count"] >= 2).all()
            np.testing.assert_array_equal(g["candidate_times"][..., :2], h["candidate_times"][..., :2])


def test_argument_errors(gpu_ctx):
    lib = nat.load()
    cases.check_argument_errors(lambda *a: lib.mtg_segment_min_max_magnitude_batch(gpu_ctx.handle, *a, 0),
                                lambda *a: lib.mtg_segment_min_max_axis_batch(gpu_ctx.handle, *a, 0))


def test_device_pointers_and_async(gpu_ctx, api):
    """torch tensors on the device (MTG_FLAG_DEVICE_PTRS, the launch on torch's stream), waited for and with
    MTG_FLAG_ASYNC: the bytes of the host-pointer call."""
    import torch
    coeffs, times, _ = cases.ragged_batch()
    tc, tt = torch.from_numpy(coeffs).cuda(), torch.from_numpy(times).cuda()
    for name, args, targs in (("magnitude", (coeffs, times, 1, [0, 1]), (tc, tt, 1, [0, 1])),
                              ("axis", (coeffs, times, 2), (tc, tt, 2))):
        want = getattr(api, name)(*args, candidate_capacity=7)
        for asynchronous in (False, True):
            got = getattr(api, name)(*targs, candidate_capacity=7, asynchronous=asynchronous)
            torch.cuda.current_stream().synchronize()
            assert cases.same_bytes(mtg.extrema_from_bytes(got["minimum"]).reshape(want["minimum"].shape), want["minimum"])
            assert cases.same_bytes(mtg.extrema_from_bytes(got["maximum"]).reshape(want["maximum"].shape), want["maximum"])
            for key in ("candidate_times", "candidate_count", "status"):
                assert cases.same_bytes(got[key].cpu().numpy(), want[key]), (name, asynchronous, key)
    assert EXTREMUM_DTYPE.itemsize == 24
