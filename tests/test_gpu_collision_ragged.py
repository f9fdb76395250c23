"""mtg_collision_cost_ragged_batch (csrc/mtg_collision_ragged.hip over csrc/mtg_collision.inc, DESIGN.md
3.18): cost, gradient, flag, count and status byte-equal to mtg_collision_cost_batch run on every packed
K-group, sorted and shuffled, with K = 1 and a segment of more than 64 clock samples in the batch; grad_out
NULL; device pointers with MTG_FLAG_ASYNC; two async calls with different seg_count; the LDS limit on K_max;
a BAD_TIME trajectory between its neighbours; and the pipeline ragged solve -> vertex derivatives ->
collision cost against the uniform chain per K-group."""
import numpy as np
import pytest

import mav_trajectory_generation_cmake_amd as mtg
from mav_trajectory_generation_cmake_amd import _native as nat

import _collision_model as CM
import _collision_ragged_cases as RC
from _ragged_cases import per_k_batches

pytestmark = pytest.mark.gpu

N = 10
COUNTS = ((1, 4), (2, 3), (3, 3), (5, 2), (8, 2))


@pytest.fixture(scope="module")
def case():
    groups = RC.collision_groups(N, COUNTS, seed0=11, long_segment=True)
    assert groups[2][2][0, 0] / 0.1 > 64  # more clock samples in a segment than a chunk holds
    grid, prm = RC.collision_params()
    g, p = CM.to_native(grid, prm)
    return dict(groups=groups, grid=grid, g=g, p=p)


def _uniform(gpu_ctx, c, grad=True):
    return lambda x, t, m: gpu_ctx.collision_cost_batch(N, x, t, c["g"], c["p"], mask=m if grad else None, grad=grad)


@pytest.mark.parametrize("how", ["sorted", "shuffled"])
def test_equals_the_uniform_device_entry_per_group(gpu_ctx, case, how):
    order = RC.collision_order(case["groups"], how, seed=6)
    x, mask, times, seg = RC.collision_csr(case["groups"], order)
    x0, m0, t0 = x.copy(), mask.copy(), times.copy()
    got = gpu_ctx.collision_cost_ragged_batch(N, x, times, seg, case["g"], case["p"], mask=mask, grad=True)
    assert x.tobytes() == x0.tobytes() and mask.tobytes() == m0.tobytes() and times.tobytes() == t0.tobytes()
    assert (got["status"] == 0).all() and got["n_evaluated"].min() > 0 and (got["cost"] > 0).sum() >= len(order) // 2
    assert np.abs(got["grad"]).max() > 0
    RC.assert_collision_equals_the_uniform(got, order, case["groups"], _uniform(gpu_ctx, case))
    # grad_out == NULL leaves the other outputs' bytes unchanged
    nograd = gpu_ctx.collision_cost_ragged_batch(N, x, times, seg, case["g"], case["p"])
    assert "grad" not in nograd
    for k in ("cost", "collision", "n_evaluated", "status"):
        assert nograd[k].tobytes() == got[k].tobytes(), k
    RC.assert_collision_equals_the_uniform(nograd, order, case["groups"], _uniform(gpu_ctx, case, grad=False), grad=False)


def test_device_pointers_async_and_two_calls_with_different_seg_count(gpu_ctx, case):
    import torch
    dv = torch.device("cuda", 0)
    tg = mtg.SdfGrid(torch.from_numpy(case["grid"].field).to(dv), case["grid"].origin, case["grid"].resolution,
                     case["grid"].oob)
    calls = []
    for how, seed in (("shuffled", 6), ("shuffled", 7), ("sorted", 0)):
        order = RC.collision_order(case["groups"], how, seed=seed)
        if seed == 7:
            order = order[3:]  # another batch size, another seg_count
        x, mask, times, seg = RC.collision_csr(case["groups"], order)
        calls.append((order, seg, [torch.from_numpy(a).to(dv) for a in (x, mask, times)]))
    torch.cuda.synchronize(dv)
    outs = [gpu_ctx.collision_cost_ragged_batch(N, x, times, seg, tg, case["p"], mask=mask, grad=True, asynchronous=True)
            for order, seg, (x, mask, times) in calls]  # back to back, no synchronisation between them
    torch.cuda.synchronize(dv)
    gpu_ctx.reset_stream()
    host_ptr = gpu_ctx.collision_cost_ragged_batch(N, *[a.cpu().numpy() for a in (calls[0][2][0], calls[0][2][2])],
                                                   calls[0][1], case["g"], case["p"], mask=calls[0][2][1].cpu().numpy(),
                                                   grad=True)
    for k in RC.OUTPUTS:  # device pointers with MTG_FLAG_ASYNC give the bytes of the host-pointer call
        assert outs[0][k].cpu().numpy().tobytes() == host_ptr[k].tobytes(), k
    for (order, seg, _), out in zip(calls, outs):
        RC.assert_collision_equals_the_uniform(out, order, case["groups"], _uniform(gpu_ctx, case))


def _lds_bytes(K, N=10):
    """collision_lds_bytes (csrc/mtg_collision.hip): coefficients, times, vertex values, one chunk."""
    return 8 * (K * 3 * N + K + (K + 1) * (N // 2) * 3 + 3 * 65 + 64)


def test_k_max_at_the_lds_limit(gpu_ctx, case):
    """K_max exactly at the 64 KiB limit runs, K_max + 1 gives MTG_ERR_TOO_LARGE with nothing written; at
    N = 10 the limit is that of collision_lds_bytes, which the uniform entry applies to its K."""
    K = 172
    assert _lds_bytes(K) <= 64 * 1024 < _lds_bytes(K + 1)
    rng = np.random.default_rng(172)
    times_long = rng.uniform(0.21, 0.39, size=K + 1)  # 3 or 4 clock samples per segment
    x_long, m_long = CM.random_trajectory(N, K + 1, 1720, times_long, extent=5.0)
    small = RC.collision_groups(N, ((2, 2), (3, 1)), seed0=11)
    lib = nat.load()
    for k_long, want in ((K, nat.MTG_OK), (K + 1, nat.MTG_ERR_TOO_LARGE)):
        xl, ml, tl = x_long[:k_long + 1], m_long[:k_long + 1].copy(), times_long[:k_long]
        ml[-1] = 31
        groups = dict(small)
        groups[k_long] = (xl[None], ml[None], tl[None])
        order = [(2, 0), (k_long, 0), (3, 0), (2, 1)]
        x, mask, times, seg = RC.collision_csr(groups, order)
        uni_cost = np.full(1, 7.0)
        gn, keep = case["g"].native()
        import ctypes
        rc_uniform = lib.mtg_collision_cost_batch(gpu_ctx.handle, N, 3, k_long, 1, np.ascontiguousarray(xl).ctypes.data, None,
                                                  np.ascontiguousarray(tl).ctypes.data, ctypes.byref(gn),
                                                  ctypes.byref(case["p"].native()), uni_cost.ctypes.data, None, None, None,
                                                  None, 0)
        assert rc_uniform == want
        if want == nat.MTG_OK:
            got = gpu_ctx.collision_cost_ragged_batch(N, x, times, seg, case["g"], case["p"], mask=mask, grad=True)
            assert (got["status"] == 0).all() and got["n_evaluated"][1] > K
            RC.assert_collision_equals_the_uniform(got, order, groups, _uniform(gpu_ctx, case))
        else:
            cost = np.full(len(order), 7.0)
            rc = lib.mtg_collision_cost_ragged_batch(gpu_ctx.handle, N, 3, len(order), seg.ctypes.data, x.ctypes.data, None,
                                                     times.ctypes.data, ctypes.byref(gn), ctypes.byref(case["p"].native()),
                                                     cost.ctypes.data, None, None, None, None, 0)
            assert rc == want and (cost == 7.0).all() and (uni_cost == 7.0).all()
            assert b"LDS" in lib.mtg_last_error(gpu_ctx.handle)
        del keep


def test_bad_time_trajectory_in_the_middle(gpu_ctx, case):
    from test_collision_ragged_host import bad_time_in_the_middle
    bad_time_in_the_middle(
        lambda x, t, seg, m: gpu_ctx.collision_cost_ragged_batch(N, x, t, seg, case["g"], case["p"], mask=m, grad=True),
        _uniform(gpu_ctx, case))


def test_device_result_against_the_host_path_and_the_model(gpu_ctx, case):
    """The ragged device result of one trajectory per K against the FP64 model (check_against's bounds);
    decisions (count, flag) as the host path's on the whole batch."""
    order = RC.collision_order(case["groups"], "shuffled", seed=6)
    x, mask, times, seg = RC.collision_csr(case["groups"], order)
    got = gpu_ctx.collision_cost_ragged_batch(N, x, times, seg, case["g"], case["p"], mask=mask, grad=True)
    host = mtg.host_collision_cost_ragged_batch(N, x, times, seg, case["g"], case["p"], mask=mask, grad=True)
    np.testing.assert_array_equal(got["n_evaluated"], host["n_evaluated"])
    np.testing.assert_array_equal(got["collision"], host["collision"])
    grads = mtg.split_ragged(got["grad"], seg, "grad", D=3)
    grid, prm = RC.collision_params()
    for b, (K, i) in enumerate(order):
        if i != 1 and not (K == 2 and i == 0):
            continue
        gr = case["groups"][K]
        model = CM.fp64_model(N, gr[0][i], gr[2][i], gr[1][i], grid, prm)
        assert model["margin"] >= 1e-9 and got["n_evaluated"][b] == model["n_eval"]
        CM.check_against("ragged device [%d] K=%d" % (b, K), got["cost"][b], grads[b], model)


def test_pipeline_solve_vertex_derivatives_collision(gpu_ctx, case):
    """solve_linear_ragged_batch -> vertex_derivatives_ragged_batch -> collision_cost_ragged_batch on a
    shuffled batch: every output byte equals the uniform chain (solve_linear_batch -> vertex_derivatives_batch
    -> collision_cost_batch) run on each packed K-group."""
    from _ragged_cases import order_of, ragged_of
    D, r = 3, 4
    batches = per_k_batches(N, D, {1: 3, 2: 3, 3: 2, 5: 2, 8: 2}, seed0=21)
    order = order_of(batches, "shuffled", seed=3)
    values, mask, times, seg = ragged_of(batches, order)
    solved = gpu_ctx.solve_linear_ragged_batch(N, r, values, mask, times, seg)
    vv = gpu_ctx.vertex_derivatives_ragged_batch(solved["coeffs"], times, seg)
    got = gpu_ctx.collision_cost_ragged_batch(N, vv, times, seg, case["g"], case["p"], mask=mask, grad=True)
    chain = {}
    for K in sorted(batches):
        idx = [i for k, i in order if k == K]
        v, m, t = (np.ascontiguousarray(a[idx]) for a in batches[K])
        co = gpu_ctx.solve_linear_batch(N, r, v, m, t)["coeffs"]
        xv = gpu_ctx.vertex_derivatives_batch(co, t)
        chain[K] = dict(coeffs=co, vertex_values=xv, **gpu_ctx.collision_cost_batch(N, xv, t, case["g"], case["p"], mask=m, grad=True))
    views = {"coeffs": mtg.split_ragged(solved["coeffs"], seg, "coeffs"), "vertex_values": mtg.split_ragged(vv, seg, "vertex_values")}
    views.update({n: mtg.split_ragged(got[n], seg, n, D=D) for n in RC.OUTPUTS})
    seen = {}
    for b, (K, _) in enumerate(order):
        at = seen.get(K, 0)
        seen[K] = at + 1
        for n, per in views.items():
            ref = np.asarray(chain[K][n][at])
            RC.same_bytes(np.asarray(per[b]).reshape(ref.shape), ref, "%s of trajectory %d (K = %d)" % (n, b, K))
    assert (got["status"] == 0).all() and got["n_evaluated"].sum() > 100
