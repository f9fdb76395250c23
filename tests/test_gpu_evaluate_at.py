"""mtg_evaluate_at_batch on the GPU: both kernels (a lane per query; a block per trajectory with the
coefficients staged in LDS) against the host path, bit for bit (tests/test_evaluate_at_host.py pins the
host path to the definition)."""
import itertools

import numpy as np
import pytest

import _evaluate_at_model as model
from mav_trajectory_generation_cmake_amd import _native as nat
from mav_trajectory_generation_cmake_amd import host_evaluate_at_batch
from test_evaluate_at_host import STRIDES, strided_queries

pytestmark = pytest.mark.gpu

SHAPES = [(10, 3, 10), (12, 4, 20), (6, 1, 1), (10, 3, 37), (2, 5, 2), (10, 3, 100)]
BS, MS = (1, 7, 130), (1, 3, 64, 65, 300)
LANE, STAGED = nat.MTG_EVALUATE_AT_LANE, nat.MTG_EVALUATE_AT_STAGED


def same_results(got, want, what=""):
    model.assert_same_bits(got[0], want[0], what)
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(got[2], want[2]), what


def threshold(K):
    """The smallest M of the staged kernel for shapes whose staged block fits (the rule itself is
    mtg_evaluate_at_path; asserted where this is used)."""
    return max(32, K)


@pytest.mark.parametrize("N,D,K", SHAPES)
def test_kernels_vs_host_path(gpu_ctx, N, D, K):
    """Every B and M with every derivative pair; the strides cycle, and the first query times of every
    trajectory are a rotating window of its edge-case times (0, t < 0, every interior prefix value, the
    total and its neighbours, +-inf, NaN), so both kernels meet all of them."""
    rng = np.random.default_rng(100 * N + K)
    paths = set()
    n = 0
    for B, M in itertools.product(BS, MS):
        coeffs, times, tq = model.random_case(rng, N, D, K, B, M)
        for k0, nd in model.derivative_pairs(N):
            tq = tq.copy()
            for b in range(B):
                edge = model.edge_times(times[b])
                w = min(M, len(edge))
                tq[b, :w] = edge[(3 * n + np.arange(w)) % len(edge)]
            kind = STRIDES[n % len(STRIDES)]
            n += 1
            path = nat.evaluate_at_path(N, D, K, M, nd)
            assert path == (STAGED if M >= threshold(K) else LANE), (N, D, K, M, nd)
            paths.add(path)
            q = strided_queries(tq, kind)
            same_results(gpu_ctx.evaluate_at_batch(coeffs, times, q, k0, nd),
                         host_evaluate_at_batch(coeffs, times, q, k0, nd), (N, D, K, B, M, k0, nd, kind, path))
    assert paths == {LANE, STAGED}


@pytest.mark.parametrize("N,D,K", [(10, 3, 10), (12, 4, 20), (10, 3, 37)])
def test_both_kernels_give_the_same_bits(gpu_ctx, N, D, K):
    rng = np.random.default_rng(7 + K)
    M = threshold(K)
    coeffs, times, tq = model.random_case(rng, N, D, K, 7, M)
    w = min(M - 1, K + 7)
    tq[:, :w] = np.stack([model.edge_times(times[b]) for b in range(7)])[:, :w]
    for k0, nd in model.derivative_pairs(N):
        assert nat.evaluate_at_path(N, D, K, M, nd) == STAGED and nat.evaluate_at_path(N, D, K, M - 1, nd) == LANE
        staged = gpu_ctx.evaluate_at_batch(coeffs, times, tq, k0, nd)
        lane = gpu_ctx.evaluate_at_batch(coeffs, times, np.ascontiguousarray(tq[:, :M - 1]), k0, nd)
        model.assert_same_bits(staged[0][:, :M - 1], lane[0], (N, D, K, k0, nd))
        assert np.array_equal(staged[1][:, :M - 1], lane[1])


def test_more_queries_than_one_block_takes(gpu_ctx):
    """M = 1100: a staged block takes 4 passes of 256 queries, so each trajectory has a second, partial
    block; the output run of an odd row width starts off a 16-B boundary for odd trajectories."""
    rng = np.random.default_rng(9)
    coeffs, times, tq = model.random_case(rng, 10, 3, 10, 3, 1100)
    for k0, nd in ((0, 1), (0, 3)):
        same_results(gpu_ctx.evaluate_at_batch(coeffs, times, tq, k0, nd), host_evaluate_at_batch(coeffs, times, tq, k0, nd),
                     (k0, nd))


@pytest.mark.parametrize("M", [3, 65])
def test_independent_of_the_call(gpu_ctx, M):
    """Row b alone, inside the batch of 130 and inside the reversed batch: identical bits."""
    rng = np.random.default_rng(11 + M)
    coeffs, times, tq = model.random_case(rng, 10, 3, 10, 130, M)
    whole = gpu_ctx.evaluate_at_batch(coeffs, times, tq, 0, 3)
    rev = gpu_ctx.evaluate_at_batch(coeffs[::-1], times[::-1], np.ascontiguousarray(tq[::-1]), 0, 3)
    same_results([x[::-1] for x in rev], whole, "reversed")
    for b in (0, 63, 64, 129):
        alone = gpu_ctx.evaluate_at_batch(coeffs[b:b + 1], times[b:b + 1], tq[b:b + 1], 0, 3)
        same_results(alone, [x[b:b + 1] for x in whole], b)


@pytest.mark.parametrize("M", [3, 65])
@pytest.mark.parametrize("nd", [1, 2])
def test_output_alignment_and_null_outputs(gpu_ctx, M, nd):
    """Device pointers with `out` one double past a 16-B boundary, D * n_derivatives odd and even: the
    aligned call's bits, canaries before and after untouched; in_range_out and status NULL."""
    import torch
    rng = np.random.default_rng(13)
    N, D, K, B = 10, 3, 10, 7
    coeffs, times, tq = model.random_case(rng, N, D, K, B, M)
    want = host_evaluate_at_batch(coeffs, times, tq, 0, nd)[0]
    dev = dict(device="cuda:0")
    c, t, q = (torch.from_numpy(np.ascontiguousarray(x)).to(**dev) for x in (coeffs, times, tq))
    n = want.size
    gpu_ctx.reset_stream()
    for shift in (0, 1):
        buf = torch.full((n + 4,), -777.0, dtype=torch.float64, **dev)
        assert buf.data_ptr() % 16 == 0
        rc = gpu_ctx._lib.mtg_evaluate_at_batch(gpu_ctx.handle, N, D, K, B, c.data_ptr(), t.data_ptr(), q.data_ptr(), M, M,
                                                0, nd, buf.data_ptr() + 8 * (1 + shift), None, None,
                                                nat.MTG_FLAG_DEVICE_PTRS)
        nat.check(rc, gpu_ctx.handle)
        got = buf.cpu().numpy()
        model.assert_same_bits(got[1 + shift:1 + shift + n].reshape(want.shape), want, (M, nd, shift))
        assert (got[:1 + shift] == -777.0).all() and (got[1 + shift + n:] == -777.0).all()


def test_strided_view_does_not_read_the_padding(gpu_ctx):
    import torch
    rng = np.random.default_rng(17)
    for M in (3, 65):
        coeffs, times, tq = model.random_case(rng, 10, 3, 10, 7, M)
        want = gpu_ctx.evaluate_at_batch(coeffs, times, tq, 0, 3)
        view = strided_queries(tq, "padded")
        assert view.strides[0] == 8 * (M + 3) and np.isnan(view.base[:, M:]).all()
        same_results(gpu_ctx.evaluate_at_batch(coeffs, times, view, 0, 3), want, M)
        tview = torch.from_numpy(view.base).to("cuda:0")[:, :M]
        assert tview.stride() == (M + 3, 1)
        got = gpu_ctx.evaluate_at_batch(torch.from_numpy(coeffs).to("cuda:0"), torch.from_numpy(times).to("cuda:0"), tview,
                                        0, 3)
        same_results([x.cpu().numpy() for x in got], want, ("torch", M))


def test_torch_tensors_on_the_current_stream(gpu_ctx):
    import torch
    rng = np.random.default_rng(19)
    for M in (1, 65):
        coeffs, times, tq = model.random_case(rng, 10, 3, 10, 130, M)
        want = gpu_ctx.evaluate_at_batch(coeffs, times, tq, 0, 3)
        shared = gpu_ctx.evaluate_at_batch(coeffs, times, tq[0], 0, 3)
        s = torch.cuda.Stream(device="cuda:0")
        with torch.cuda.stream(s):
            c, t, q = (torch.from_numpy(x).to("cuda:0", non_blocking=False) for x in (coeffs, times, tq))
            got = gpu_ctx.evaluate_at_batch(c, t, q, 0, 3, asynchronous=True)
            got_shared = gpu_ctx.evaluate_at_batch(c, t, q[0], 0, 3, asynchronous=True)
        s.synchronize()
        assert got[0].is_cuda and tuple(got[0].shape) == (130, M, 3, 3)
        same_results([x.cpu().numpy() for x in got], want, M)
        same_results([x.cpu().numpy() for x in got_shared], shared, M)
        assert gpu_ctx.last_kernel_ms() > 0.0
    gpu_ctx.reset_stream()


@pytest.mark.parametrize("M", [3, 65])
def test_bad_time_trajectories(gpu_ctx, M):
    rng = np.random.default_rng(23)
    coeffs, times, tq = model.random_case(rng, 10, 3, 10, 8, M)
    bad = {1: 0.0, 4: -1.0, 6: np.nan}
    for b, v in bad.items():
        times[b, 3] = v
    got = gpu_ctx.evaluate_at_batch(coeffs, times, tq, 0, 3)
    same_results(got, host_evaluate_at_batch(coeffs, times, tq, 0, 3))
    good = [b for b in range(8) if b not in bad]
    for b in bad:
        assert got[2][b] == nat.MTG_TRAJ_BAD_TIME and np.isnan(got[0][b]).all() and not got[1][b].any()
    alone = gpu_ctx.evaluate_at_batch(coeffs[good], times[good], tq[good], 0, 3)
    same_results(alone, [x[good] for x in got])


def test_empty_calls_write_nothing(gpu_ctx):
    z = np.zeros((0, 10, 3, 10))
    out, in_range, status = gpu_ctx.evaluate_at_batch(z, np.zeros((0, 10)), np.zeros(4), 0, 1)
    assert out.shape == (0, 4, 1, 3)
    out, _, _ = gpu_ctx.evaluate_at_batch(np.zeros((2, 10, 3, 10)), np.ones((2, 10)), np.zeros(0), 0, 1)
    assert out.shape == (2, 0, 1, 3)


def test_full_size_config2(gpu_ctx):
    """1e4 config-2 coefficients from the default solve, M = 16, orders 0..2, every row against the host
    path (16 host threads: well under a second)."""
    import mav_trajectory_generation_cmake_amd as mtg
    B = 10000
    values, mask, times = mtg.random_vertices_path_batch(10, 3, 10, B, seed0=5)
    coeffs = gpu_ctx.solve_linear_batch(10, 4, values, mask, times)["coeffs"]
    rng = np.random.default_rng(29)
    tq = rng.uniform(0.0, 1.0, size=(B, 16)) * times.sum(axis=1)[:, None]
    got = gpu_ctx.evaluate_at_batch(coeffs, times, tq, 0, 3)
    same_results(got, host_evaluate_at_batch(coeffs, times, tq, 0, 3))
    assert got[1].mean() > 0.9 and not got[2].any()
