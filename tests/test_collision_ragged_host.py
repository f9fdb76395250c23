"""The host paths of the ragged vertex maps and the ragged collision cost, no GPU:
mtg_host_vertex_derivatives_batch against the 60-digit truth of tests/_vertex_map_model.py with the measure
and bound tests/test_gpu_vertex_map.py applies to the device kernel; the ragged host maps byte-equal to the
uniform host forms per trajectory and their round trip; mtg_host_collision_cost_ragged_batch byte-equal to
mtg_host_collision_cost_batch with batch 1 per trajectory and held to the FP64 model; every call-level error
with the outputs untouched; a BAD_TIME trajectory between untouched neighbours; the wrong-offset and
wrong-K restatements of the CSR indexing (the sensitivity of these tests)."""
import numpy as np
import pytest

import mav_trajectory_generation_cmake_amd as mtg
from mav_trajectory_generation_cmake_amd import _native as nat

import _collision_model as CM
import _collision_ragged_cases as RC
import _vertex_map_model as VM
from _util import scale_normalised_error
from test_vertex_map_host import host_map

TOL = 1e-9          # the coefficient map and the round trip (tests/test_gpu_vertex_map.py)
DERIV_TOL = 1e-13   # times S (tests/test_gpu_vertex_map.py: Horner's forward bound 2 N u S with a margin of 40)
SEG = (3, 1, 8, 2, 5, 1, 3, 2, 8, 5, 1)   # every K of RC.KS, K = 1 at an end and in the middle
MIXED = ((1, 3), (2, 3), (3, 3), (5, 2), (8, 2))
MODEL_MIXED = ((1, 2), (2, 2), (3, 2), (5, 1), (8, 1))


@pytest.mark.parametrize("shape", VM.EVERY_N, ids=VM.shape_id)
def test_host_vertex_derivatives_against_truth(shape):
    case = VM.derivative_case(*shape)
    got = mtg.host_vertex_derivatives_batch(case["c"], case["T"])
    err = VM.abs_err(got, case["truth"])
    q = err / case["S"]
    print("host vs truth derivatives %s: worst err / S %.2e" % (VM.shape_id(shape), q.max()))
    assert np.all(err <= DERIV_TOL * case["S"]), (float(q.max()), np.unravel_index(np.argmax(q), q.shape))
    threaded = mtg.host_vertex_derivatives_batch(case["c"], case["T"], threads=3)
    assert threaded.tobytes() == got.tobytes()


@pytest.mark.parametrize("how", ["sorted", "shuffled"])
@pytest.mark.parametrize("N,D", [(10, 3), (6, 1), (12, 4), (2, 3)])
def test_host_ragged_maps_equal_the_uniform_host_forms(N, D, how):
    groups, order = RC.groups_of_counts(N, D, SEG, seed=3)
    order = sorted(order) if how == "sorted" else RC.shuffled(order, seed=5)
    x, T, c, seg = RC.vertex_csr(groups, order)
    x0, T0, c0 = x.copy(), T.copy(), c.copy()
    got_x = mtg.host_vertex_derivatives_ragged_batch(c, T, seg, threads=2)
    got_c = mtg.host_coefficients_from_vertices_ragged_batch(N, x, T, seg, threads=2)
    assert x.tobytes() == x0.tobytes() and T.tobytes() == T0.tobytes() and c.tobytes() == c0.tobytes()
    RC.assert_vertex_maps_equal_the_uniform(order, groups, got_x, got_c, mtg.host_vertex_derivatives_batch, host_map)
    # per trajectory alone, too: batch 1 of the uniform host forms
    for b, (K, i) in enumerate(order):
        alone = mtg.host_vertex_derivatives_batch(groups[K][2][[i]], groups[K][1][[i]])[0]
        RC.same_bytes(mtg.split_ragged(got_x, seg, "vertex_values")[b], alone, "trajectory %d alone" % b)


@pytest.mark.parametrize("shape", VM.EVERY_N, ids=VM.shape_id)
def test_host_ragged_round_trip(shape):
    """values -> coeffs -> values through the ragged host forms on continuous trajectories gives the values
    back; coeffs -> values -> coeffs on the discontinuous c of the round-trip case gives the truth of the
    composition, within the bound the existing round-trip case uses."""
    N, D, K, B = shape
    case = VM.round_trip_case(*shape)
    c, T = case["c"], case["T"]
    seg = np.full(B, K, np.int32)
    back = mtg.host_coefficients_from_vertices_ragged_batch(
        N, mtg.host_vertex_derivatives_ragged_batch(c.reshape(B * K, D, N), T.reshape(-1), seg), T.reshape(-1), seg)
    back = back.reshape(B, K, D, N)
    full = scale_normalised_error(back, case["truth64"], T)
    shp = VM.shape_error(back, case["truth64"], T)
    print("ragged host round trip %s: full %.2e shape %.2e" % (VM.shape_id(shape), full, shp))
    assert full <= TOL and shp <= TOL, (full, shp)
    assert scale_normalised_error(back, c, T) > 1e-3  # the means moved the interior ends


def _collision_case(counts, how, seed0=11):
    groups = RC.collision_groups(10, counts, seed0=seed0)
    order = RC.collision_order(groups, how, seed=4)
    grid, prm = RC.collision_params()
    g, p = CM.to_native(grid, prm)
    return groups, order, grid, prm, g, p


@pytest.mark.parametrize("how", ["sorted", "shuffled"])
def test_host_ragged_collision_equals_batch_one_per_trajectory(how):
    groups, order, _, _, g, p = _collision_case(MIXED, how)
    x, mask, times, seg = RC.collision_csr(groups, order)
    got = mtg.host_collision_cost_ragged_batch(10, x, times, seg, g, p, mask=mask, grad=True, threads=3)
    nograd = mtg.host_collision_cost_ragged_batch(10, x, times, seg, g, p)
    for k in ("cost", "collision", "n_evaluated", "status"):
        assert nograd[k].tobytes() == got[k].tobytes(), "grad_out = NULL changed %s" % k
    assert (got["status"] == 0).all() and got["n_evaluated"].min() > 0 and (got["cost"] > 0).sum() >= len(order) // 2
    grads = mtg.split_ragged(got["grad"], seg, "grad", D=3)
    for b, (K, i) in enumerate(order):
        one = mtg.host_collision_cost_batch(10, groups[K][0][[i]], groups[K][2][[i]], g, p, mask=groups[K][1][[i]], grad=True)
        for k in ("cost", "collision", "n_evaluated", "status"):
            RC.same_bytes(got[k][b], one[k][0], "%s of trajectory %d (K = %d)" % (k, b, K))
        RC.same_bytes(grads[b], one["grad"][0], "grad of trajectory %d (K = %d)" % (b, K))
    RC.assert_collision_equals_the_uniform(
        got, order, groups, lambda xx, tt, mm: mtg.host_collision_cost_batch(10, xx, tt, g, p, mask=mm, grad=True))


def test_host_ragged_collision_against_the_fp64_model():
    """One mixed batch, every trajectory: the seeds (collision_groups' seed0 = 11) were chosen on the CPU so
    that every trajectory's smallest margin is >= 1e-9; none is skipped."""
    groups, order, grid, prm, g, p = _collision_case(MODEL_MIXED, "shuffled")
    x, mask, times, seg = RC.collision_csr(groups, order)
    got = mtg.host_collision_cost_ragged_batch(10, x, times, seg, g, p, mask=mask, grad=True)
    grads = mtg.split_ragged(got["grad"], seg, "grad", D=3)
    for b, (K, i) in enumerate(order):
        model = CM.fp64_model(10, groups[K][0][i], groups[K][2][i], groups[K][1][i], grid, prm)
        print("trajectory %d (K = %d): margin %.3e" % (b, K, model["margin"]))
        assert model["margin"] >= 1e-9, "the seed puts a comparison on the edge"
        assert got["n_evaluated"][b] == model["n_eval"] and bool(got["collision"][b]) == model["flag"]
        CM.check_against("ragged[%d] K=%d" % (b, K), got["cost"][b], grads[b], model)


def check_call_level_errors(ctx):
    """Every call-level error of the three ragged entries, each returned with the outputs untouched: the
    host entries for ctx None, else the device entries on that context handle (host pointers)."""
    lib = nat.load()
    N, D, B, h = 10, 3, 3, 5
    seg = np.array([2, 1, 3], np.int32)
    totS, totV = 6, 9
    grid, prm = RC.collision_params()
    groups = RC.collision_groups(N, ((1, 1), (2, 1), (3, 1)), seed0=11)
    order = [(2, 0), (1, 0), (3, 0)]
    x, mask, t, _ = RC.collision_csr(groups, order)
    c = np.ascontiguousarray(np.concatenate([VM.inputs(N, D, K, 1, seed=1)[2][0] for K, _ in order]))
    out_x, out_c = np.full((totV, h, D), 7.0), np.full((totS, D, N), 7.0)
    cost, grad = np.full(B, 7.0), np.full(totV * h * D, 7.0)
    coll, nev, stat = np.full(B, 7, np.uint8), np.full(B, 7, np.int32), np.full(B, 7, np.int32)

    def p(a):
        return None if a is None else a.ctypes.data

    def dv(N=N, D=D, B=B, seg=seg, c=c, t=t, out=out_x):
        tail = (p(seg), p(c), p(t), p(out))
        if ctx is None:
            return lib.mtg_host_vertex_derivatives_ragged_batch(N, D, B, *tail, 1)
        return lib.mtg_vertex_derivatives_ragged_batch(ctx, N, D, B, *tail, 0)

    def cf(N=N, D=D, B=B, seg=seg, c=x, t=t, out=out_c):
        tail = (p(seg), p(c), p(t), p(out))
        if ctx is None:
            return lib.mtg_host_coefficients_from_vertices_ragged_batch(N, D, B, *tail, 1)
        return lib.mtg_coefficients_from_vertices_ragged_batch(ctx, N, D, B, *tail, 0)

    def cc(N=N, D=D, B=B, seg=seg, c=x, t=t, mask=mask, grid=grid, prm=prm, cost=cost, grad=grad, no_grid=False,
           no_prm=False):
        import ctypes
        g, q = CM.to_native(grid, prm)
        gn, keep = g.native()
        gp = None if no_grid else ctypes.byref(gn)
        qp = None if no_prm else ctypes.byref(q.native())
        tail = (p(seg), p(c), p(mask), p(t), gp, qp, p(cost), p(grad), p(coll), p(nev), p(stat))
        if ctx is None:
            return lib.mtg_host_collision_cost_ragged_batch(N, D, B, *tail, 1)
        return lib.mtg_collision_cost_ragged_batch(ctx, N, D, B, *tail, 0)

    E = nat
    for f in (dv, cf, cc):
        for bad_n in (0, 3, 14):
            assert f(N=bad_n) == E.MTG_ERR_UNSUPPORTED_N
        assert f(B=-1) == E.MTG_ERR_SIZE_MISMATCH
        assert f(seg=None) == E.MTG_ERR_INVALID_ARGUMENT
        assert f(seg=np.array([2, 0, 3], np.int32)) == E.MTG_ERR_SIZE_MISMATCH
        assert f(seg=np.array([2, 1, -3], np.int32)) == E.MTG_ERR_SIZE_MISMATCH
        assert f(c=None) == f(t=None) == E.MTG_ERR_INVALID_ARGUMENT
        assert f(B=0) == f(B=0, seg=None, c=None, t=None) == E.MTG_OK
    assert dv(D=0) == cf(D=0) == E.MTG_ERR_SIZE_MISMATCH
    assert dv(out=None) == cf(out=None) == E.MTG_ERR_INVALID_ARGUMENT
    assert cc(N=2) == cc(N=4) == E.MTG_ERR_UNSUPPORTED_N          # the collision term needs N >= 6
    assert cc(D=2) == cc(D=4) == E.MTG_ERR_INVALID_ARGUMENT       # and D == 3
    assert cc(no_grid=True) == cc(no_prm=True) == E.MTG_ERR_INVALID_ARGUMENT
    for bad in (dict(dt=0.0), dict(dt=-0.1), dict(map_resolution=-1e-3)):
        q = CM.Params(**{**dict(dt=prm.dt, map_resolution=prm.map_resolution, epsilon=prm.epsilon,
                                robot_radius=prm.robot_radius, multiplier=prm.multiplier, lo=prm.lo, hi=prm.hi,
                                continuous=prm.continuous), **bad})
        assert cc(prm=q) == E.MTG_ERR_INVALID_ARGUMENT, bad
    for res in (0.0, -0.25):
        assert cc(grid=CM.Grid(grid.field, grid.origin, res, grid.oob)) == E.MTG_ERR_INVALID_ARGUMENT
    assert cc(cost=None) == cc(mask=None) == E.MTG_ERR_INVALID_ARGUMENT   # grad_out needs fixed_mask
    # nothing written by any of them
    assert (out_x == 7.0).all() and (out_c == 7.0).all() and (cost == 7.0).all() and (grad == 7.0).all()
    assert (coll == 7).all() and (nev == 7).all() and (stat == 7).all()
    assert dv() == cf() == cc() == E.MTG_OK
    assert not (out_x == 7.0).any() and not (out_c == 7.0).any() and not (cost == 7.0).any()
    assert not (grad == 7.0).any() and (stat == 0).all()   # the gradient block is zeroed, then filled


def test_call_level_errors_of_the_host_entries():
    check_call_level_errors(None)


def bad_time_in_the_middle(call, uniform):
    """A BAD_TIME trajectory in the middle of a batch: NaN, a zero gradient and its status; its neighbours'
    bytes as they are without it.  call(x, times, seg, mask) is the ragged entry, uniform(x, times, mask) the
    uniform one (both with the gradient)."""
    groups = RC.collision_groups(10, MIXED, seed0=11)
    order = [(3, 0), (2, 0), (5, 0), (1, 0), (2, 1)]
    x, mask, times, seg = RC.collision_csr(groups, order)
    vo, so = mtg.ragged_offsets(seg)
    for b_bad, value in ((2, 0.0), (2, np.nan), (1, -1.0), (3, np.inf)):
        t = times.copy()
        t[so[b_bad] + seg[b_bad] - 1] = value
        got = RC.to_host(call(x, t, seg, mask))
        assert list(got["status"]) == [nat.MTG_TRAJ_BAD_TIME if b == b_bad else 0 for b in range(len(order))]
        assert np.isnan(got["cost"][b_bad]) and got["n_evaluated"][b_bad] == 0 and got["collision"][b_bad] == 0
        grads = mtg.split_ragged(got["grad"], seg, "grad", D=3)
        assert (grads[b_bad] == 0.0).all()
        keep = [b for b in range(len(order)) if b != b_bad]
        ref_order = [order[b] for b in keep]
        ref = {n: [mtg.split_ragged(got[n], seg, n, D=3)[b] for b in keep] for n in RC.OUTPUTS}
        want, place = RC.per_group(ref_order, lambda K, idx: RC.to_host(uniform(
            np.ascontiguousarray(groups[K][0][idx]), np.ascontiguousarray(groups[K][2][idx]),
            np.ascontiguousarray(groups[K][1][idx]))))
        for j, (K, at) in enumerate(place):
            for n in RC.OUTPUTS:
                w = np.asarray(want[K][n][at])
                RC.same_bytes(np.asarray(ref[n][j]).reshape(w.shape), w, "%s of neighbour %d" % (n, keep[j]))


def test_bad_time_trajectory_in_the_middle_on_the_host():
    grid, prm = RC.collision_params()
    g, p = CM.to_native(grid, prm)
    bad_time_in_the_middle(lambda x, t, seg, m: mtg.host_collision_cost_ragged_batch(10, x, t, seg, g, p, mask=m, grad=True),
                           lambda x, t, m: mtg.host_collision_cost_batch(10, x, t, g, p, mask=m, grad=True))


def test_wrong_csr_indexing_would_fail_these_tests():
    """The sensitivity of the byte comparisons, on the CPU: restating the host paths with so[b] in place of
    so[b] + b for the vertex base, or with K_max in place of K_b, changes bytes of the mixed batch -- so a
    host path that indexed that way would fail test_host_ragged_* above."""
    groups, order, _, _, g, p = _collision_case(MIXED, "shuffled")
    x, mask, times, seg = RC.collision_csr(groups, order)
    vo, so = mtg.ragged_offsets(seg)
    right = mtg.host_collision_cost_ragged_batch(10, x, times, seg, g, p, mask=mask, grad=True)
    h, kmax = 5, int(seg.max())
    wrong_base = wrong_k = 0
    for b, K in enumerate(seg):
        if b == 0:
            continue  # so[0] + 0 == so[0]
        xb = x[so[b]:so[b] + K + 1]          # the vertex base without + b
        one = mtg.host_collision_cost_batch(10, xb[None], times[None, so[b]:so[b + 1]], g, p, mask=mask[None, so[b]:so[b] + K + 1], grad=True)
        wrong_base += one["cost"][0].tobytes() != right["cost"][b].tobytes()
        if K < kmax and so[b] + kmax <= so[-1] and vo[b] + kmax + 1 <= vo[-1]:
            one = mtg.host_collision_cost_batch(10, x[None, vo[b]:vo[b] + kmax + 1], times[None, so[b]:so[b] + kmax], g, p,
                                                mask=mask[None, vo[b]:vo[b] + kmax + 1], grad=True)
            wrong_k += one["cost"][0].tobytes() != right["cost"][b].tobytes()
    assert wrong_base >= len(seg) - 2 and wrong_k >= 3, (wrong_base, wrong_k)
    vgroups, vorder = RC.groups_of_counts(10, 3, SEG, seed=3)
    vx, vT, vc, vseg = RC.vertex_csr(vgroups, vorder)
    vvo, vso = mtg.ragged_offsets(vseg)
    got_x = mtg.host_vertex_derivatives_ragged_batch(vc, vT, vseg)
    shifted = sum(got_x[vso[b]:vso[b] + vseg[b] + 1].tobytes() != got_x[vvo[b]:vvo[b + 1]].tobytes() for b in range(1, len(vseg)))
    assert shifted == len(vseg) - 1
