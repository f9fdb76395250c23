"""mtg_evaluate_at_ragged_batch and mtg_min_max_magnitude_ragged_batch on the GPU against the uniform
device entries run on every packed K-group: every byte of every output (include/mtg.h: a trajectory's
outputs are what the uniform entry writes for it alone).  The inputs, the query set and the bad-time
trajectories are those of tests/test_evaluate_ragged_host.py."""
import numpy as np
import pytest

import mav_trajectory_generation_cmake_amd as mtg
from mav_trajectory_generation_cmake_amd import _native as nat
from _evaluate_ragged_cases import (assert_same_evaluation, assert_same_extrema, check_call_level_errors, csr_of,
                                    evaluate_reference, min_max_reference, query_rows, query_rows_of_times, shared_row,
                                    solved_groups,
                                    with_bad_times)
from _ragged_cases import order_of, per_k_batches, ragged_of
from test_evaluate_ragged_host import BAD

pytestmark = pytest.mark.gpu

LANE, STAGED = nat.MTG_EVALUATE_AT_LANE, nat.MTG_EVALUATE_AT_STAGED
COUNTS = {1: 3, 2: 4, 5: 5, 10: 3, 13: 3}


@pytest.fixture(scope="module")
def n10():
    return solved_groups(10, 3, COUNTS, seed0=77)


def _check_evaluate(ctx, groups, order, tq, k0, nd, what):
    coeffs, times, seg = csr_of(groups, order)
    got = ctx.evaluate_at_ragged_batch(coeffs, times, seg, tq, k0, nd)
    assert_same_evaluation(got, evaluate_reference(ctx.evaluate_at_batch, groups, order, tq, k0, nd), what)
    return got


# M = 1 and 5: a lane per query.  M = 40: staged for the ragged call (K_max = 13) and for every uniform
# group.  M = 1030: one more than a 1024-query chunk, a second block per trajectory with a tail of 6.
@pytest.mark.parametrize("how", ["sorted", "shuffled"])
@pytest.mark.parametrize("M,path", [(1, LANE), (5, LANE), (40, STAGED), (1030, STAGED)])
def test_evaluate_at_equals_the_uniform_device_call(gpu_ctx, n10, how, M, path):
    order = order_of(n10, how, seed=3)
    assert nat.evaluate_at_ragged_path(10, 3, 13, M, 1) == nat.evaluate_at_ragged_path(10, 3, 13, M, 3) == path
    assert {nat.evaluate_at_path(10, 3, K, M, 3) for K in COUNTS} == {path}
    for tq in (query_rows(n10, order, M, seed=5), shared_row(n10, order, M, seed=5)):
        for k0, nd in ((0, 1), (0, 3)):
            got = _check_evaluate(gpu_ctx, n10, order, tq, k0, nd, (how, M, tq.ndim, k0, nd))
            assert not got[2].any()


@pytest.mark.parametrize("how", ["sorted", "shuffled"])
def test_mixed_mappings_give_the_same_bytes(gpu_ctx, n10, how):
    """One K = 50 trajectory and M = 40: the ragged call takes the lane mapping (M < K_max) while the
    uniform K <= 13 groups take the staged one."""
    groups = dict(n10)
    groups.update(solved_groups(10, 3, {50: 1}, seed0=91))
    order = order_of(groups, how, seed=6)
    assert nat.evaluate_at_ragged_path(10, 3, 50, 40, 3) == LANE and nat.evaluate_at_path(10, 3, 5, 40, 3) == STAGED
    _check_evaluate(gpu_ctx, groups, order, query_rows(groups, order, 40, seed=7), 0, 3, how)


@pytest.mark.parametrize("N,D,counts", [(2, 1, {1: 3, 2: 3, 5: 4}), (12, 3, {1: 2, 3: 3, 10: 3, 13: 2})])
@pytest.mark.parametrize("M", [5, 40])
def test_other_orders_and_dimensions(gpu_ctx, N, D, counts, M):
    groups = solved_groups(N, D, counts, seed0=5 * N)
    order = order_of(groups, "shuffled", seed=N)
    for k0, nd in ((0, 1), (0, min(3, N)), (N - 1, 1)):
        _check_evaluate(gpu_ctx, groups, order, query_rows(groups, order, M, seed=8), k0, nd, (N, D, M, k0, nd))


@pytest.mark.parametrize("M", [5, 40])
def test_batch_of_one_and_single_segment_trajectories_at_the_ends(gpu_ctx, n10, M):
    for order in ([(10, 1)], [(1, 0)], [(1, 0), (13, 1), (5, 2), (13, 0), (1, 2)]):
        _check_evaluate(gpu_ctx, n10, order, query_rows(n10, order, M, seed=9), 0, 3, (M, order))
        _check_evaluate(gpu_ctx, n10, order, shared_row(n10, order, M, seed=9), 0, 1, (M, order, "shared"))


@pytest.mark.parametrize("M", [5, 40])
@pytest.mark.parametrize("how", ["sorted", "shuffled"])
def test_bad_time_trajectories_and_their_neighbours(gpu_ctx, n10, how, M):
    order = order_of(n10, how, seed=4)
    bad_groups = with_bad_times(n10, BAD)
    tq = query_rows(n10, order, M, seed=6)
    got = [x for x in _check_evaluate(gpu_ctx, bad_groups, order, tq, 0, 3, (how, M))]
    bad = [b for b, (K, i) in enumerate(order) if any((K, i) == key[:2] for key in BAD)]
    good = [b for b in range(len(order)) if b not in bad]
    assert len(bad) == 2
    assert (got[2][bad] == nat.MTG_TRAJ_BAD_TIME).all() and np.isnan(got[0][bad]).all() and not got[1][bad].any()
    clean = gpu_ctx.evaluate_at_ragged_batch(*csr_of(n10, order), tq, 0, 3)
    assert_same_evaluation([x[good] for x in got], [x[good] for x in clean], "neighbours of the bad trajectories")


def test_device_result_equals_the_host_path(gpu_ctx, n10):
    """An independent pin: the library's host path (held to the definition by the CPU tests)."""
    order = order_of(n10, "shuffled", seed=11)
    coeffs, times, seg = csr_of(n10, order)
    for M in (5, 40):
        tq = query_rows(n10, order, M, seed=12)
        assert_same_evaluation(gpu_ctx.evaluate_at_ragged_batch(coeffs, times, seg, tq, 0, 3),
                               mtg.host_evaluate_at_ragged_batch(coeffs, times, seg, tq, 0, 3), M)


def _device_solve(ctx, N, D, counts, how, seed, **kw):
    """(order, seg_count, the ragged device solve's result dict, times tensor) of per_k_batches problems."""
    import torch
    batches = per_k_batches(N, D, counts, seed0=seed)
    order = order_of(batches, how, seed=seed)
    values, mask, times, seg = ragged_of(batches, order)
    dev = [torch.from_numpy(x).to("cuda:0") for x in (values, mask, times)]
    return order, seg, ctx.solve_linear_ragged_batch(N, 4, *dev, seg, **kw), dev[2]


def test_device_pointers_end_to_end(gpu_ctx):
    """The device tensors of Context.solve_linear_ragged_batch go straight in (MTG_FLAG_DEVICE_PTRS); the
    result equals the host-array call on the same bytes."""
    order, seg, sol, times = _device_solve(gpu_ctx, 10, 3, COUNTS, "shuffled", 31)
    coeffs = sol["coeffs"]
    assert coeffs.is_cuda and tuple(coeffs.shape) == (int(seg.sum()), 3, 10)
    import torch
    tblocks = mtg.split_ragged(times.cpu().numpy(), seg, "times")
    for M in (5, 40):
        tq = query_rows_of_times(tblocks, M, seed=13)
        got = gpu_ctx.evaluate_at_ragged_batch(coeffs, times, seg, torch.from_numpy(tq).to("cuda:0"), 0, 3)
        assert got[0].is_cuda
        want = gpu_ctx.evaluate_at_ragged_batch(coeffs.cpu().numpy(), times.cpu().numpy(), seg, tq, 0, 3)
        assert_same_evaluation(got, want, M)
    mn, mx = gpu_ctx.min_max_magnitude_ragged_batch(coeffs, times, seg, 1)
    hmn, hmx = gpu_ctx.min_max_magnitude_ragged_batch(coeffs.cpu().numpy(), times.cpu().numpy(), seg, 1)
    assert_same_extrema(mtg.extrema_from_bytes(mn), hmn, "minimum")
    assert_same_extrema(mtg.extrema_from_bytes(mx), hmx, "maximum")
    gpu_ctx.reset_stream()


def test_two_async_evaluate_calls_with_different_seg_count(gpu_ctx, n10):
    """Back to back on one context and then one synchronise: the second call's offsets must not overwrite
    those the first call's kernel still reads."""
    import torch
    calls = []
    for seed, cut in ((21, None), (22, 11)):
        order = order_of(n10, "shuffled", seed=seed)[:cut]
        coeffs, times, seg = csr_of(n10, order)
        tq = query_rows(n10, order, 40, seed=seed)
        calls.append((order, seg, tq, [torch.from_numpy(x).to("cuda:0") for x in (coeffs, times, tq)]))
    torch.cuda.synchronize()
    outs = [gpu_ctx.evaluate_at_ragged_batch(d[0], d[1], seg, d[2], 0, 3, asynchronous=True) for _, seg, _, d in calls]
    mms = [gpu_ctx.min_max_magnitude_ragged_batch(d[0], d[1], seg, 1, asynchronous=True) for _, seg, _, d in calls]
    torch.cuda.synchronize()
    for (order, seg, tq, _), got, mm in zip(calls, outs, mms):
        assert_same_evaluation(got, evaluate_reference(gpu_ctx.evaluate_at_batch, n10, order, tq, 0, 3), len(order))
        want = min_max_reference(gpu_ctx.min_max_magnitude_batch, n10, order, 1, None)
        assert_same_extrema(mtg.extrema_from_bytes(mm[0]), want[0], len(order))
        assert_same_extrema(mtg.extrema_from_bytes(mm[1]), want[1], len(order))
    gpu_ctx.reset_stream()


def test_async_solve_then_evaluate_on_its_outputs(gpu_ctx):
    """A ragged solve (gathered groups: it uses the context's ragged buffer) and a ragged evaluate of its
    coefficients, both asynchronous, then one synchronise."""
    import torch
    batches = per_k_batches(10, 3, COUNTS, seed0=41)
    order = order_of(batches, "shuffled", seed=41)
    values, mask, times, seg = ragged_of(batches, order)
    tq = query_rows_of_times(mtg.split_ragged(times, seg, "times"), 40, seed=14)
    dev = [torch.from_numpy(x).to("cuda:0") for x in (values, mask, times, tq)]
    torch.cuda.synchronize()
    sol = gpu_ctx.solve_linear_ragged_batch(10, 4, dev[0], dev[1], dev[2], seg, asynchronous=True)
    got = gpu_ctx.evaluate_at_ragged_batch(sol["coeffs"], dev[2], seg, dev[3], 0, 3, asynchronous=True)
    torch.cuda.synchronize()
    want = mtg.host_evaluate_at_ragged_batch(sol["coeffs"].cpu().numpy(), times, seg, tq, 0, 3)
    assert_same_evaluation(got, want)
    assert not want[2].any() and want[1].any()
    gpu_ctx.reset_stream()


def _check_min_max(ctx, groups, order, derivative, dimensions, what, in_place=None):
    coeffs, times, seg = csr_of(groups, order)
    if in_place is not None:  # the plan is the ragged solve's: all in place, or all gathered
        assert mtg.solve_ragged_plan(10, 3, 4, seg)["n_in_place"] == (len(order) if in_place else 0)
    want = min_max_reference(ctx.min_max_magnitude_batch, groups, order, derivative, dimensions)
    got = ctx.min_max_magnitude_ragged_batch(coeffs, times, seg, derivative, dimensions)
    assert_same_extrema(got[0], want[0], ("minimum",) + what)
    assert_same_extrema(got[1], want[1], ("maximum",) + what)
    only_min = ctx.min_max_magnitude_ragged_batch(coeffs, times, seg, derivative, dimensions, maximum=False)
    only_max = ctx.min_max_magnitude_ragged_batch(coeffs, times, seg, derivative, dimensions, minimum=False)
    assert only_min[1] is None and only_max[0] is None
    assert_same_extrema(only_min[0], want[0], ("only minimum",) + what)
    assert_same_extrema(only_max[1], want[1], ("only maximum",) + what)


@pytest.mark.parametrize("how", ["sorted", "shuffled"])
@pytest.mark.parametrize("derivative", [1, 2])
@pytest.mark.parametrize("dimensions", [None, (0, 2)])
def test_min_max_equals_the_uniform_device_call(gpu_ctx, how, derivative, dimensions):
    groups = solved_groups(10, 3, {1: 4, 3: 5, 10: 4}, seed0=55)
    order = order_of(groups, how, seed=2)
    _check_min_max(gpu_ctx, groups, order, derivative, dimensions, (how, derivative, dimensions), in_place=how == "sorted")


@pytest.mark.parametrize("how", ["sorted", "shuffled"])
def test_min_max_where_the_staged_dimensions_differ_between_groups(gpu_ctx, how):
    """N = 12, D = 3: K = 20 runs 2 trajectories per block with 3 dimensions staged per pass, K = 21 runs 3
    with 2 (its root polynomial is summed in another order)."""
    groups = solved_groups(12, 3, {20: 4, 21: 5}, seed0=66)
    order = order_of(groups, how, seed=5)
    for derivative in (1, 2):
        _check_min_max(gpu_ctx, groups, order, derivative, None, (how, derivative))


def test_min_max_with_a_long_trajectory(gpu_ctx):
    """One K = 65 trajectory (4 lanes per segment in the uniform call, 8 for the others) inside the batch."""
    groups = solved_groups(10, 3, {1: 2, 3: 3, 10: 3}, seed0=55)
    groups.update(solved_groups(10, 3, {65: 1}, seed0=56))
    order = order_of(groups, "shuffled", seed=7)
    _check_min_max(gpu_ctx, groups, order, 1, None, ("K = 65",))
    _check_min_max(gpu_ctx, groups, order, 2, (0, 2), ("K = 65",))


@pytest.mark.parametrize("how", ["sorted", "shuffled"])
def test_min_max_with_more_dimensions_than_are_staged(gpu_ctx, how):
    groups = solved_groups(10, 5, {1: 3, 3: 4, 10: 3}, seed0=88)
    order = order_of(groups, how, seed=9)
    _check_min_max(gpu_ctx, groups, order, 1, None, (how, "D = 5"))
    _check_min_max(gpu_ctx, groups, order, 2, (0, 2), (how, "D = 5, mask 0b101"))


def test_min_max_device_result_against_the_host_path(gpu_ctx, n10):
    """An extra, independent pin on top of the byte-exact comparisons above, which it does not replace or
    loosen: the device and the host path are different algorithms' roundings (the kernel's lanes against
    a scalar loop), so they agree at the figure the uniform entries are held to in
    tests/test_gpu_parity.py -- the same segment, values to 1e-9 relative -- and not to the bit."""
    order = order_of(n10, "shuffled", seed=15)
    coeffs, times, seg = csr_of(n10, order)
    g = gpu_ctx.min_max_magnitude_ragged_batch(coeffs, times, seg, 1)
    h = mtg.host_min_max_magnitude_ragged_batch(coeffs, times, seg, 1)
    for a, b in zip(g, h):
        np.testing.assert_array_equal(a["segment"], b["segment"])
        np.testing.assert_allclose(a["value"], b["value"], rtol=1e-9)


def test_call_level_errors_of_the_device_entries(gpu_ctx):
    gpu_ctx.reset_stream()
    check_call_level_errors(gpu_ctx.handle)


def test_empty_calls(gpu_ctx):
    o, r, s = gpu_ctx.evaluate_at_ragged_batch(np.zeros((0, 3, 10)), np.zeros(0), [], np.zeros(4))
    assert o.shape == (0, 4, 1, 3) and r.shape == (0, 4) and s.shape == (0,)
    o, _, _ = gpu_ctx.evaluate_at_ragged_batch(np.zeros((3, 3, 10)), np.ones(3), [2, 1], np.zeros(0))
    assert o.shape == (2, 0, 1, 3)
    mn, mx = gpu_ctx.min_max_magnitude_ragged_batch(np.zeros((0, 3, 10)), np.zeros(0), [], 1)
    assert mn.shape == mx.shape == (0,)
