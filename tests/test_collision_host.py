"""Collision cost and gradient over a signed distance field: the host path
(mtg_host_collision_cost_batch) against a hand-computed answer, the FP64 restatement of the
reference loop and its 50-digit truth (tests/_collision_model.py), plus the model's own check of
paper eq. 14, the argument / status errors and the C++ wrapper.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import mav_trajectory_generation_cmake_amd as mtg
from mav_trajectory_generation_cmake_amd import _native as nat

import _collision_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1201  # of the eq. 14 self-check: chosen on the CPU so that its preconditions hold (asserted there)


def _known_answer_inputs(free_acceleration=True):
    """One N = 6 segment x0 + v t along x at height z0 = 0.375 and y = 0.125 (cell centres of the
    planar map), T = 1, dt = 0.125, map_resolution = 0."""
    x = np.zeros((1, 2, 3, 3))
    x[0, 0, 0] = [-1.0, 0.125, 0.375]
    x[0, 1, 0] = [1.0, 0.125, 0.375]
    x[0, :, 1, 0] = 2.0
    mask = np.array([[3, 3] if free_acceleration else [7, 7]], dtype=np.uint8)
    prm = M.Params(0.125, 0.0, 0.5, 0.125, 1.0, (-8.0,) * 3, (8.0,) * 3, False)
    return x, mask, np.array([[1.0]]), M.maps()["plane"], prm


@pytest.mark.parametrize("continuous", [False, True], ids=["nearest", "continuous"])
def test_known_answer(continuous):
    x, mask, times, grid, prm = _known_answer_inputs()
    prm.continuous = continuous
    g, p = M.to_native(grid, prm)
    out = mtg.host_collision_cost_batch(6, x, times, g, p, mask=mask, grad=True)
    # samples at t = 0, 0.125, .., 0.875 (exact); the first is skipped, the other seven each carry
    # time_sum = dt.  d = z0 - radius = 0.25 <= epsilon = 0.5: c = 0.5 / 0.5 * (0.25 - 0.5)^2.  (With the
    # continuous lookup the distance is z_c + (y - y_c) = z0 on this line.)
    c = 0.5 / 0.5 * (0.25 - 0.5) ** 2
    want = c * 2.0 * 0.125 * 7
    print("cost", out["cost"][0], "want", want)
    assert out["n_evaluated"][0] == 7 and out["collision"][0] == 0 and out["status"][0] == 0
    # the coefficients of x0 + v t are exact up to rounding of A(T)^-1 [x_i; x_{i+1}]: a few ulp
    assert abs(out["cost"][0] - want) <= 1e-12 * want
    model = M.fp64_model(6, x[0], times[0], mask[0], grid, prm)
    assert model["n_eval"] == 7 and not model["flag"]
    # map_resolution = 0: the central differences are 0 / 0, as in the reference; the NaN pattern must agree
    assert np.isnan(model["grad"][:, :2]).all() and not np.isnan(model["grad"][:, 2:]).any()
    M.check_against("known answer", out["cost"][0], out["grad"][0], model)


def test_model_gradient_is_the_derivative_of_the_model_cost():
    """Eq. 14 in the model, independent of the product: planar map, continuous distance.  The increment
    is small against the cell, so that every +-increment lookup stays in its sample's cell (asserted):
    the potential is then quadratic along each axis between the three lookups, its central difference
    is its derivative, and the model's gradient is the derivative of the model's cost at fixed gates."""
    N, K = 10, 2
    times = (1.44, 1.83)
    grid = M.maps()["plane"]
    inc = 1.0 / 1024
    prm = M.Params(0.1, inc, 3.0, 0.3, 2.0, (-7.0,) * 3, (7.0,) * 3, True)
    x, mask = M.random_trajectory(N, K, SEED, times, extent=1.0)
    x[:, 0, 2] += 1.5  # 0 < d < epsilon at every lookup (asserted): the quadratic branch, no kink
    base = M.fp64_model(N, x, times, mask, grid, prm)
    fd_step = 1e-6
    # the unshifted positions are further from their cell's faces than the increment and than any
    # displacement by the perturbation below (at most fd_step x T^q / q! <= 1e-5)
    assert base["margins"]["cell_unshifted"] * grid.resolution > inc + 1e-5, "a lookup leaves its sample's cell"
    assert base["band"] > 1e-3 and not base["flag"] and base["n_eval"] > 20
    h, V = N // 2, K + 1
    slots = [(v, q) for v in range(V) for q in range(h) if not (mask[v] >> q) & 1]
    worst = 0.0
    for k in range(3):
        for j, (v, q) in enumerate(slots):
            step = fd_step
            costs = []
            for s in (+1, -1):
                xp = x.copy()
                xp[v, q, k] += s * step
                m = M.fp64_model(N, xp, times, mask, grid, prm, want_grad=False)
                assert m["decisions"] == base["decisions"], "the gates moved under the perturbation"
                costs.append(m["cost"])
            fd = (costs[0] - costs[1]) / (2 * step)
            err = abs(fd - base["grad"][k, j])
            scale = np.max(np.abs(base["grad"][k]))
            worst = max(worst, err / scale)
            assert err <= 1e-6 * scale, (k, v, q, fd, base["grad"][k, j])
    print("worst relative difference %.3e" % worst)


@pytest.mark.parametrize("name", [c["name"] for c in M.CASES])
def test_host_against_model_and_truth(name):
    c = M.build_case(name)
    g, p = M.to_native(c["grid"], c["prm"])
    out = mtg.host_collision_cost_batch(c["N"], c["x"], c["times"], g, p, mask=c["mask"], grad=True)
    nograd = mtg.host_collision_cost_batch(c["N"], c["x"], c["times"], g, p)
    assert (out["status"] == 0).all()
    assert out["cost"].tobytes() == nograd["cost"].tobytes(), "grad_out = NULL changed the cost bits"
    for j, model in enumerate(c["models"]):
        print(name, j, "margin %.3e" % model["margin"], model["margins"])
        assert model["margin"] >= 1e-9, "the seed puts a comparison on the edge"
        assert out["n_evaluated"][j] == model["n_eval"]
        assert bool(out["collision"][j]) == model["flag"]
        M.check_against("%s[%d]" % (name, j), out["cost"][j], out["grad"][j], model, M.case_truth(name, j))


def test_clock_tie_counts_like_the_model():
    """T = 23 x 0.1: the accumulated clock passes 2.3 by an ulp-sized amount, so whether a 24th sample is
    taken is decided by the additions themselves; the host path makes them as the model does."""
    grid, prm = M.maps()["sphere"], M.Params(0.1, 0.0, 1.0, 0.3, 2.0, (-7.0,) * 3, (7.0,) * 3, False)
    x, mask = M.random_trajectory(10, 2, 77, (2.3, 0.7))
    model = M.fp64_model(10, x, (2.3, 0.7), mask, grid, prm, want_grad=False)
    g, p = M.to_native(grid, prm)
    out = mtg.host_collision_cost_batch(10, x[None], np.array([[2.3, 0.7]]), g, p)
    assert out["n_evaluated"][0] == model["n_eval"] == len(model["decisions"]) - model["decisions"].count(0)


def test_argument_and_status_errors():
    x, mask, times, grid, prm = _known_answer_inputs()

    def call(**kw):
        q = M.Params(prm.dt, prm.map_resolution, prm.epsilon, prm.robot_radius, prm.multiplier, prm.lo, prm.hi, False)
        gg = M.Grid(grid.field, grid.origin, grid.resolution, grid.oob)
        for k, v in kw.items():
            setattr(q if hasattr(q, k) else gg, k, v)
        g, p = M.to_native(gg, q)
        return mtg.host_collision_cost_batch(6, x, times, g, p, mask=mask, grad=True)

    for bad in (dict(dt=0.0), dict(dt=-0.1), dict(map_resolution=-1e-3), dict(resolution=0.0), dict(resolution=-0.25)):
        with pytest.raises(mtg.MTGError) as e:
            call(**bad)
        assert e.value.code == nat.MTG_ERR_INVALID_ARGUMENT, bad
    g, p = M.to_native(grid, prm)
    with pytest.raises(mtg.MTGError) as e:  # D != 3
        mtg.host_collision_cost_batch(6, np.zeros((1, 2, 3, 2)), times, g, p)
    assert e.value.code == nat.MTG_ERR_INVALID_ARGUMENT
    # a non-positive or non-finite T: BAD_TIME and a NaN cost for that trajectory only, no loop
    xs = np.repeat(x, 4, axis=0)
    ts = np.array([[1.0], [0.0], [np.inf], [np.nan]])
    out = mtg.host_collision_cost_batch(6, xs, ts, g, p, mask=np.repeat(mask, 4, axis=0), grad=True)
    assert list(out["status"]) == [0, nat.MTG_TRAJ_BAD_TIME, nat.MTG_TRAJ_BAD_TIME, nat.MTG_TRAJ_BAD_TIME]
    assert np.isfinite(out["cost"][0]) and np.isnan(out["cost"][1:]).all()
    assert (out["grad"][1:] == 0).all() and (out["n_evaluated"][1:] == 0).all()


def test_cpp_wrapper_known_answer():
    """tests/cpp/test_collision_api.cpp (built under MTG_BUILD_TESTS): collisionCost<N> on the host
    policy against the same hand-computed answer."""
    from test_cpp_api import _cmake_build
    _cmake_build()
    exe = os.path.join(ROOT, "build", "test_collision_api")
    assert os.path.exists(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
