"""mtg_coefficients_from_vertices_batch and mtg_vertex_derivatives_batch (csrc/mtg_vertex.hip, with
coefficients_from_ends of mtg_vertex_common.h) against the 60-digit truth of tests/_vertex_map_model.py:
every N, K = 1, D != 3, every value the block-size rule takes (16, 12, 2 at the last K that fits, a
quotient of 3 rounded to 2) with tail blocks, the first K that does not fit, a position offset of 1e8,
discontinuous coefficients (the interior-vertex mean and its segment-time index), the round trip, the
independence of a trajectory's bytes from its place in the batch, and the two users of the maps,
set_free_constraints_batch and initial_solution_without_position_constraints.

The shapes and the arithmetic of the block-size rule are in _vertex_map_model.py.  test_vertex_map_model.py
pins the model to the reference algorithm; test_vertex_map_host.py runs the host twin on the same cases."""
import numpy as np
import pytest

import mav_trajectory_generation_cmake_amd as mtg
from mav_trajectory_generation_cmake_amd import _native as nat

import _vertex_map_model as M
from _util import scale_normalised_error
from test_vertex_map_host import host_map
from test_vertex_map_model import oracle_coefficients

pytestmark = pytest.mark.gpu

TOL = 1e-9          # the coefficient map, both metrics (README: the library's promise against truth)
DERIV_TOL = 1e-13   # times S: Horner's forward bound is 2 N u S = 2.7e-15 S at N = 12, the falling
#                     factorials are exact in FP64, the mean adds one rounding: a margin of about 40


@pytest.mark.parametrize("shape", M.SHAPES, ids=M.shape_id)
def test_coefficient_map_against_truth(gpu_ctx, shape):
    case = M.coefficient_case(*shape)
    c = gpu_ctx.coefficients_from_vertices_batch(case["N"], case["x"], case["T"])
    full = scale_normalised_error(c, case["truth64"], case["T"])
    shp = M.shape_error(c, case["truth64"], case["T"])
    print("device vs truth %s: full %.2e shape %.2e" % (M.shape_id(shape), full, shp))
    assert full <= TOL and shp <= TOL, (full, shp)


@pytest.mark.parametrize("shape", M.OFFSET_SHAPES, ids=M.shape_id)
def test_coefficient_map_keeps_the_shape_at_position_offset_1e8(gpu_ctx, shape):
    """"Start position subtracted first (only c_0 changes)": the two positions are subtracted exactly
    before anything is scaled, so c_j for j >= 1 does not see a common offset of the positions.  The
    reference's FP64 Schur inverse (the oracle) has no such step and misses the bound here; its figure
    and the host's are printed with the device's (DESIGN.md records the three)."""
    case = M.coefficient_case(*shape, offset=M.OFFSET)
    N, x, T, ref = case["N"], case["x"], case["T"], case["truth64"]
    c = gpu_ctx.coefficients_from_vertices_batch(N, x, T)
    dev = M.shape_error(c, ref, T)
    host = M.shape_error(host_map(N, x, T), ref, T)
    oracle = M.shape_error(oracle_coefficients(case), ref, T)
    msg = "offset 1e8 %s shape metric: device %.2e, host %.2e, oracle %.2e" % (M.shape_id(shape), dev, host, oracle)
    print(msg)
    assert dev <= TOL and host <= TOL, msg
    assert scale_normalised_error(c, ref, T) <= TOL


def _derivative_cases():
    return [(s, "mixed") for s in M.SHAPES] + list(M.TIME_MODE_SHAPES)


@pytest.mark.parametrize("shape,mode", _derivative_cases(), ids=lambda v: M.shape_id(v) if isinstance(v, tuple) else v)
def test_derivative_map_against_truth(gpu_ctx, shape, mode):
    """On coefficient blocks drawn independently per segment: the two ends that meet at an interior
    vertex differ by O(1), so one end for the mean, their sum, or another segment's time shows.
    "equal" (one time per trajectory) and "unequal" (0.05 next to 30) are the two layouts on which a
    wrong segment-time index behaves differently.  N = 2 (H = 1) and K = 1 (no interior vertex) are
    among the shapes."""
    case = M.derivative_case(*shape, mode=mode)
    got = gpu_ctx.vertex_derivatives_batch(case["c"], case["T"])
    err = M.abs_err(got, case["truth"])
    q = err / case["S"]
    print("device vs truth derivatives %s %s: worst err / S %.2e" % (M.shape_id(shape), mode, q.max()))
    assert np.all(err <= DERIV_TOL * case["S"]), (float(q.max()), np.unravel_index(np.argmax(q), q.shape))
    if shape[2] > 1:  # the input is discontinuous: the interior ends really differ
        c, T = case["c"], case["T"]
        start = c[:, 1:, :, 0]
        end = (c[:, :-1] * T[:, :-1, None, None] ** np.arange(shape[0])).sum(axis=-1)
        assert np.median(np.abs(start - end)) > 0.1


@pytest.mark.parametrize("shape", M.EVERY_N, ids=M.shape_id)
def test_round_trip_on_discontinuous_input(gpu_ctx, shape):
    """coefficients_from_vertices(vertex_derivatives(c)) of a discontinuous c is not c: it is the
    trajectory through the interior means.  Asserted against the truth of the composition."""
    case = M.round_trip_case(*shape)
    N, c, T = shape[0], case["c"], case["T"]
    back = gpu_ctx.coefficients_from_vertices_batch(N, gpu_ctx.vertex_derivatives_batch(c, T), T)
    full = scale_normalised_error(back, case["truth64"], T)
    shp = M.shape_error(back, case["truth64"], T)
    print("round trip %s: full %.2e shape %.2e" % (M.shape_id(shape), full, shp))
    assert full <= TOL and shp <= TOL, (full, shp)
    assert scale_normalised_error(back, c, T) > 1e-3  # the means moved the interior ends


@pytest.mark.parametrize("N,D,K,TB", [(10, 3, 10, 12), (10, 3, 66, 2)], ids=["K10-TB12", "K66-TB2"])
def test_placement_changes_no_byte(gpu_ctx, N, D, K, TB):
    """Trajectory j's bytes are the same alone (B = 1), as the last of a batch whose tail block holds
    only it (B = TB + 1), and as the first of a full block that is not the grid's first (B = 2 TB,
    place TB); both maps; the inputs are unchanged.  TB: 46 K + 15 doubles per trajectory in 6144,
    475 -> 12 and 3051 -> 2 (_vertex_map_model.py)."""
    B = 2 * TB
    x, T, c = M.inputs(N, D, K, B, seed=7)
    j = 1
    for inp, call in ((x, lambda a, t: gpu_ctx.coefficients_from_vertices_batch(N, a, t)),
                      (c, lambda a, t: gpu_ctx.vertex_derivatives_batch(a, t))):
        others = [b for b in range(B) if b != j]
        alone = call(inp[[j]], T[[j]])[0]
        assert np.isfinite(alone).all()
        for order, place in ((others[:TB] + [j], TB), (others[:TB] + [j] + others[TB:], TB)):
            a, t = np.ascontiguousarray(inp[order]), np.ascontiguousarray(T[order])
            a0, t0 = a.copy(), t.copy()
            out = call(a, t)
            assert out[place].tobytes() == alone.tobytes(), (len(order), place)
            assert a.tobytes() == a0.tobytes() and t.tobytes() == t0.tobytes()
            assert out[0].tobytes() == call(a[[0]], t[[0]])[0].tobytes()  # and so are the first's


@pytest.mark.parametrize("shape", M.TOO_LARGE, ids=M.shape_id)
def test_first_K_that_does_not_fit(gpu_ctx, shape):
    """MTG_ERR_TOO_LARGE from both maps at the first K whose per-trajectory arrays do not fit twice in
    48 KiB (N = 10: 46 * 67 + 15 = 3097 doubles, 6144 / 3097 = 1; N = 12: 55 * 56 + 18 = 3098); the
    output is not touched and the context goes on working."""
    N, D, K, B = shape
    x, T, c = M.inputs(*shape)
    lib = nat.load()
    SENTINEL = -12345.5
    for fn, inp, oshape in ((lib.mtg_coefficients_from_vertices_batch, x, c.shape),
                            (lib.mtg_vertex_derivatives_batch, c, x.shape)):
        out = np.full(oshape, SENTINEL)
        inp = np.ascontiguousarray(inp)
        rc = fn(gpu_ctx.handle, N, D, K, B, inp.ctypes.data, T.ctypes.data, out.ctypes.data, 0)
        assert rc == nat.MTG_ERR_TOO_LARGE, rc
        assert np.all(out == SENTINEL)
        assert b"LDS" in lib.mtg_last_error(gpu_ctx.handle)
    with pytest.raises(nat.MTGError) as e:
        gpu_ctx.coefficients_from_vertices_batch(N, x, T)
    assert e.value.code == nat.MTG_ERR_TOO_LARGE
    small = M.coefficient_case(N, 3, 3, 5)  # the context still works: one small call
    cs = gpu_ctx.coefficients_from_vertices_batch(N, small["x"], small["T"])
    assert scale_normalised_error(cs, small["truth64"], small["T"]) <= TOL


def test_objective_time_coeffs_out_at_a_K_that_does_not_fit(gpu_ctx):
    """mtg_objective_time_batch forms coeffs_out (objective 4) with the coefficient map, so it returns the
    same code at such a K -- and only when coeffs_out is asked for.  The inputs are the generator-made
    shapes of _objective_time_cases.py stretched to K = 67 (no fixture)."""
    import _objective_time_cases as TC
    N, D, K, B, r = 10, 3, 67, 2, 4
    values, mask, times = mtg.random_vertices_path_batch(N, D, K, B, seed0=9300, max_derivative=4)
    c = dict(N=N, D=D, K=K, B=B, r=r, values=values, mask=mask, times=times, w_c=0.0,
             n_free=mtg.number_of_free_constraints(mask, N))
    prm = TC.params(c, 4, soft=False)
    x = TC.x4(c, np.zeros((B, D, (K + 1) * (N // 2))))
    out = gpu_ctx.objective_time_batch(N, values, mask, x, prm)
    assert np.isfinite(out["cost"]).all() and out["coeffs"] is None
    with pytest.raises(nat.MTGError) as e:
        gpu_ctx.objective_time_batch(N, values, mask, x, prm, coeffs=True)
    assert e.value.code == nat.MTG_ERR_TOO_LARGE
    again = gpu_ctx.objective_time_batch(N, values, mask, x, prm)
    assert again["cost"].tobytes() == out["cost"].tobytes()


def _free_constraint_problem(N, D, K, B, seed0):
    """createRandomVertices per trajectory with its own max_derivative at the two ends (2 .. h - 1), so
    n_free differs within the batch (the generator alone gives every trajectory the same mask), and
    with a fixed velocity, drawn like the positions' scale, at about half of the interior vertices."""
    h = N // 2
    rng = np.random.default_rng(seed0)
    parts = [mtg.random_vertices_batch(N, D, K, 1, [-10.0] * D, [10.0] * D, seed0=seed0 + b, max_derivative=2 + b % (h - 2))
             for b in range(B)]
    values, mask, times = (np.concatenate([p[i] for p in parts]) for i in range(3))
    pin = rng.random((B, K + 1)) < 0.5
    pin[:, [0, K]] = False
    mask[pin] |= 2
    values[:, :, 1, :] = np.where(pin[:, :, None], rng.uniform(-2.0, 2.0, size=(B, K + 1, D)), values[:, :, 1, :])
    return values, mask, times


@pytest.mark.parametrize("N,r,K,D", [(10, 4, 1, 3), (10, 4, 2, 3), (8, 3, 5, 2)])
def test_set_free_constraints_and_initial_solution(gpu_ctx, N, r, K, D):
    B, h, V = 6, N // 2, K + 1
    values, mask, times = _free_constraint_problem(N, D, K, B, seed0=4100 + N + K)
    mask0 = mask.copy()
    out = gpu_ctx.initial_solution_without_position_constraints(N, r, values, mask, times)
    assert np.isfinite(out["coeffs"]).all() and mask.tobytes() == mask0.tobytes()
    # the new problem: interior positions freed, the ends (for K = 1 everything) unchanged
    assert np.all(out["mask"][:, [0, K]] == mask[:, [0, K]])
    assert np.all(out["mask"][:, 1:K] == mask[:, 1:K] & 0xFE)
    if K == 1:
        assert out["mask"].tobytes() == mask.tobytes()
    else:
        assert np.any(out["mask"][:, 1:K] & 2) and not np.all(out["mask"][:, 1:K] & 2)  # some interior velocities fixed
    assert len(set(out["n_free"].tolist())) > 1
    for b in range(B):
        slots = [(v, k) for v in range(V) for k in range(h) if not (int(out["mask"][b, v]) >> k) & 1]
        assert out["n_free"][b] == len(slots)
        assert np.all(out["free"][b, :, len(slots):] == 0.0)
        truth, S = M.truth_vertex_derivatives(N, out["coeffs"][b], times[b])
        want = np.array([[truth[v, k, d] for (v, k) in slots] for d in range(D)], dtype=object)
        bound = DERIV_TOL * np.array([[S[v, k, d] for (v, k) in slots] for d in range(D)])
        err = M.abs_err(out["free"][b, :, :len(slots)], want)
        assert np.all(err <= bound), (b, float(np.max(err / bound)))
    back = gpu_ctx.set_free_constraints_batch(N, out["values"], out["mask"], times, out["free"])
    e = scale_normalised_error(back, out["coeffs"], times)
    print("set_free_constraints(initial solution) N=%d K=%d D=%d: %.2e" % (N, K, D, e))
    assert e <= TOL
