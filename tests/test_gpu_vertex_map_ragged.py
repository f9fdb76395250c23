"""mtg_vertex_derivatives_ragged_batch and mtg_coefficients_from_vertices_ragged_batch
(csrc/mtg_vertex_ragged.hip): every trajectory's bytes against the uniform device entries run
on its packed K-group, at the smallest shapes at which a tile of TS packed segments can go wrong -- total
segments below one tile, exactly one tile, one tile plus one; a trajectory border on the first and on the last
segment of a tile; a trajectory over three tiles; a run of K = 1 trajectories filling a tile (the 2 TS + 1
vertex-row bound); every N; D = 1 and D = 4 --, a K = 100 chain the uniform entries refuse, device pointers
with MTG_FLAG_ASYNC, two async calls with different seg_count, and the call-level errors."""
import numpy as np
import pytest

import mav_trajectory_generation_cmake_amd as mtg
from mav_trajectory_generation_cmake_amd import _native as nat

import _collision_ragged_cases as RC
import _vertex_map_model as VM
from _util import scale_normalised_error
from test_collision_ragged_host import DERIV_TOL, TOL

pytestmark = pytest.mark.gpu

TS = 32  # packed segments per block at every (N, D) used here (asserted)

# segment counts per case; sums are in the ids.  The uniform entries take K <= 66 at N = 10, D = 3.
TILE_CASES = {
    "below-one-tile-9": [3, 1, 5],
    "one-tile-32": [8, 1, 5, 2, 3, 8, 5],
    "one-tile-plus-one-33": [8, 1, 5, 2, 3, 8, 5, 1],
    "last-trajectory-crosses-33": [8, 1, 5, 2, 3, 8, 6],
    "border-on-last-and-first-segment": [31, 1, 2, 29, 1, 1, 3],   # K = 1 at segments 31, 63 and 64; a start at 32
    "starts-on-the-last-segment": [31, 2, 30, 3, 2],               # 31..32 and 63..65 cross into the next tile
    "ends-on-the-first-segment": [30, 3, 5],                       # 30..32: its last segment opens tile 1
    "three-tiles": [5, 66, 3],                                     # segments 5..70: tiles 0, 1 and 2
    "k1-run-fills-a-tile": [3] + [1] * 40 + [5],                   # tile 1 is K = 1 throughout: 64 vertex rows
    "k1-run-from-segment-0": [1] * 33,
}


def _run(gpu_ctx, N, D, seg, seed=0, shuffle=None):
    groups, order = RC.groups_of_counts(N, D, seg, seed=seed)
    if shuffle is not None:
        order = RC.shuffled(order, seed=shuffle)
    x, T, c, sc = RC.vertex_csr(groups, order)
    x0, T0, c0 = x.copy(), T.copy(), c.copy()
    got_x = gpu_ctx.vertex_derivatives_ragged_batch(c, T, sc)
    got_c = gpu_ctx.coefficients_from_vertices_ragged_batch(N, x, T, sc)
    assert x.tobytes() == x0.tobytes() and T.tobytes() == T0.tobytes() and c.tobytes() == c0.tobytes()
    assert np.isfinite(got_x).all() and np.isfinite(got_c).all()
    return groups, order, (x, T, c, sc), got_x, got_c


@pytest.mark.parametrize("name", list(TILE_CASES))
def test_tiles_equal_the_uniform_device_entries(gpu_ctx, name):
    assert nat.load().mtg_vertex_ragged_tile(10, 3) == TS
    groups, order, _, got_x, got_c = _run(gpu_ctx, 10, 3, TILE_CASES[name])
    RC.assert_vertex_maps_equal_the_uniform(order, groups, got_x, got_c, gpu_ctx.vertex_derivatives_batch,
                                            gpu_ctx.coefficients_from_vertices_batch)


@pytest.mark.parametrize("N,D", [(N, 3) for N in (2, 4, 6, 8, 10, 12)] + [(10, 1), (8, 4)])
def test_every_order_and_other_dimensions(gpu_ctx, N, D):
    """A shuffled batch of every K of {1, 2, 3, 5, 8} over two tiles and a bit."""
    assert nat.load().mtg_vertex_ragged_tile(N, D) == TS
    seg = [3, 1, 8, 2, 5, 1, 3, 2, 8, 5, 1, 8, 8, 5, 3, 2, 1, 8]
    groups, order, _, got_x, got_c = _run(gpu_ctx, N, D, seg, seed=N + D, shuffle=1)
    assert sum(seg) > 2 * TS
    RC.assert_vertex_maps_equal_the_uniform(order, groups, got_x, got_c, gpu_ctx.vertex_derivatives_batch,
                                            gpu_ctx.coefficients_from_vertices_batch)


def test_a_chain_of_100_segments_in_a_mixed_batch(gpu_ctx):
    """The uniform device entries refuse K = 100 at N = 10, D = 3 (asserted), so the long chain is held to the
    host form and to the 60-digit truth within the bounds of the truth test; its neighbours are still
    byte-equal to the uniform entries."""
    N, D = 10, 3
    groups, order, (x, T, c, sc), got_x, got_c = _run(gpu_ctx, N, D, [3, 100, 2, 1], seed=9)
    with pytest.raises(mtg.MTGError) as e:
        gpu_ctx.vertex_derivatives_batch(groups[100][2], groups[100][1])
    assert e.value.code == nat.MTG_ERR_TOO_LARGE
    RC.assert_vertex_maps_equal_the_uniform(order, groups, got_x, got_c, gpu_ctx.vertex_derivatives_batch,
                                            gpu_ctx.coefficients_from_vertices_batch, skip=(100,))
    dev_x = mtg.split_ragged(got_x, sc, "vertex_values")[1]
    dev_c = mtg.split_ragged(got_c, sc, "coeffs")[1]
    host_x = mtg.host_vertex_derivatives_ragged_batch(c, T, sc)
    host_c = mtg.host_coefficients_from_vertices_ragged_batch(N, x, T, sc)
    truth, S = VM.truth_vertex_derivatives(N, groups[100][2][0], groups[100][1][0])
    err_t = VM.abs_err(dev_x, truth)
    err_h = np.abs(dev_x - mtg.split_ragged(host_x, sc, "vertex_values")[1])
    print("K = 100 derivatives: worst err / S vs truth %.2e, vs host %.2e" % ((err_t / S).max(), (err_h / S).max()))
    assert np.all(err_t <= DERIV_TOL * S) and np.all(err_h <= DERIV_TOL * S)
    Tl = groups[100][1][:1]
    e_c = scale_normalised_error(dev_c[None], mtg.split_ragged(host_c, sc, "coeffs")[1][None], Tl)
    e_t = scale_normalised_error(dev_c[None], VM.to_float(VM.truth_coefficients(N, groups[100][0][0], Tl[0]))[None], Tl)
    print("K = 100 coefficients: vs host %.2e, vs truth %.2e" % (e_c, e_t))
    assert e_c <= TOL and e_t <= TOL


def test_device_pointers_async_and_two_calls_with_different_seg_count(gpu_ctx):
    import torch
    dv = torch.device("cuda", 0)
    calls = []
    for seg, seed in (([31, 2, 30, 3, 2], 2), ([1] * 33 + [8, 5], 3)):
        groups, order = RC.groups_of_counts(10, 3, seg, seed=seed)
        x, T, c, sc = RC.vertex_csr(groups, order)
        calls.append((groups, order, sc, [torch.from_numpy(a).to(dv) for a in (x, T, c)]))
    torch.cuda.synchronize(dv)
    outs = []
    for groups, order, sc, (x, T, c) in calls:  # back to back, no synchronisation between them
        outs.append((gpu_ctx.vertex_derivatives_ragged_batch(c, T, sc, asynchronous=True),
                     gpu_ctx.coefficients_from_vertices_ragged_batch(10, x, T, sc, asynchronous=True)))
    torch.cuda.synchronize(dv)
    gpu_ctx.reset_stream()
    for (groups, order, sc, _), (gx, gc) in zip(calls, outs):
        RC.assert_vertex_maps_equal_the_uniform(order, groups, gx.cpu().numpy(), gc.cpu().numpy(),
                                                gpu_ctx.vertex_derivatives_batch, gpu_ctx.coefficients_from_vertices_batch)


def test_call_level_errors_of_the_device_entries(gpu_ctx):
    from test_collision_ragged_host import check_call_level_errors
    check_call_level_errors(gpu_ctx.handle)
    lib = nat.load()
    assert lib.mtg_vertex_ragged_tile(3, 3) == nat.MTG_ERR_UNSUPPORTED_N and lib.mtg_vertex_ragged_tile(10, 0) == nat.MTG_ERR_SIZE_MISMATCH
    # LDS use depends on N and D only: D = 40 still has a tile, a D in the hundreds has none
    assert 1 <= lib.mtg_vertex_ragged_tile(10, 40) < TS and lib.mtg_vertex_ragged_tile(12, 400) == nat.MTG_ERR_TOO_LARGE
    seg = np.array([1], np.int32)
    out = np.full((1, 12, 400), 7.0)
    rc = lib.mtg_vertex_derivatives_ragged_batch(gpu_ctx.handle, 12, 400, 1, seg.ctypes.data, np.zeros((1, 400, 12)).ctypes.data,
                                                 np.ones(1).ctypes.data, out.ctypes.data, 0)
    assert rc == nat.MTG_ERR_TOO_LARGE and (out == 7.0).all()


def test_a_small_tile_at_a_large_dimension(gpu_ctx):
    """D = 40 shrinks the tile (LDS is a function of TS, N and D only); the bytes still equal the uniform
    entries'."""
    N, D = 6, 40
    ts = nat.load().mtg_vertex_ragged_tile(N, D)
    assert ts == 11  # 8 * (12 * 240 + 12 + 23 * 120) + 4 * 24 = 45312 <= 48 KiB < the same at 12
    seg = [5, 8, 1, 8, 3, 2]  # (K <= 8: the uniform entries' limit at this D) 5..12 crosses a border, 14..21 ends on one
    groups, order, _, got_x, got_c = _run(gpu_ctx, N, D, seg, seed=4)
    RC.assert_vertex_maps_equal_the_uniform(order, groups, got_x, got_c, gpu_ctx.vertex_derivatives_batch,
                                            gpu_ctx.coefficients_from_vertices_batch)
