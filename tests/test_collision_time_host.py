"""Segment-time gradient of the collision cost, the host path
(mtg_host_collision_time_gradient_batch): against the FP64 restatement of the reference's
getCostAndGradientTime walks and its 50-digit twin (tests/_collision_time_model.py), the edge rules
(the 0.1 clamp, the NaN rule, bad times) and the argument errors.  No GPU."""
import numpy as np
import pytest

import mav_trajectory_generation_cmake_amd as mtg
from mav_trajectory_generation_cmake_amd import _native as nat

import _collision_model as M
import _collision_time_model as TM


def _row(out, j):
    return {k: out[k][j] for k in ("grad_t", "side_cost", "side_evaluated")}


@pytest.mark.parametrize("name", [c["name"] for c in M.CASES])
def test_host_against_model_and_truth(name):
    c = M.build_case(name)
    g, p = M.to_native(c["grid"], c["prm"])
    out = mtg.host_collision_time_gradient_batch(c["N"], c["x"], c["times"], g, p, increment_time=TM.INC)
    assert (out["status"] == 0).all()
    for j, mdl in enumerate(TM.case_models(name)):
        print(name, j, "margin %.3e" % mdl["margin"])
        assert mdl["margin"] >= 1e-9, "the seed puts a comparison other than the clock on the edge"
        TM.check_sides("%s[%d]" % (name, j), _row(out, j), mdl, TM.INC)
    if name == "short-segment":  # T = 0.07 <= 0.1: both sides 0.1, the clock tie t == T' == 0.1
        assert (out["grad_t"][:, 1] == 0.0).all() and not np.signbit(out["grad_t"][:, 1]).any()
        assert (out["side_cost"][:, 1, 0] == out["side_cost"][:, 1, 1]).all()
        assert TM.case_models(name)[0]["sides"][1, 0]["margins"]["clock"] == 0.0


@pytest.mark.parametrize("map_resolution", [0.2, 1.5])
def test_early_stop_inputs_on_the_host(map_resolution):
    """The inputs of the device's early-stop test: what the model says about them (asserted here, without
    a GPU), and the host path on them."""
    c = TM.early_case(map_resolution)
    K = c["K"]
    for mdl in c["models"]:
        assert mdl["margin"] >= 1e-9
        if map_resolution == 0.2:
            assert all(s["walked"] == min(2, K - n) for (n, _), s in mdl["sides"].items())
            assert mdl["segments_walked"] == 4 * K - 2
    if map_resolution == 1.5:
        never = [(j, k) for j, mdl in enumerate(c["models"]) for k, s in mdl["sides"].items() if s["rejoined"] is False]
        later = [(j, k) for j, mdl in enumerate(c["models"]) for k, s in mdl["sides"].items()
                 if s["rejoined"] and s["walked"] > 2]
        print("never rejoin:", never, "rejoin after n+2:", later)
        assert any(n + 2 < K for _, (n, _) in never) and later
    g, p = M.to_native(c["grid"], c["prm"])
    out = mtg.host_collision_time_gradient_batch(c["N"], c["x"], c["times"], g, p, increment_time=TM.INC)
    for j, mdl in enumerate(c["models"]):
        TM.check_sides("early %.1f [%d]" % (map_resolution, j), _row(out, j), mdl, TM.INC)


@pytest.mark.parametrize("inc", [0.1, 0.005])
def test_more_samples_than_a_chunk_on_the_host(inc):
    c = TM.long_case(inc)
    mdl = c["model"]
    assert mdl["margin"] >= 1e-9
    g, p = M.to_native(c["grid"], c["prm"])
    out = mtg.host_collision_time_gradient_batch(c["N"], c["x"], c["times"], g, p, increment_time=inc)
    TM.check_sides("long inc %g" % inc, _row(out, 0), mdl, inc)
    assert out["side_evaluated"].min() > 2 * 64  # more evaluated samples than a chunk per segment
    if inc == 0.1:  # ten samples more or fewer in the perturbed segment
        assert (out["side_evaluated"][0, :, 1] > out["side_evaluated"][0, :, 0]).all()


def _edge_inputs():
    grid = M.maps()["sphere"]
    prm = M.Params(0.1, 0.2, 1.0, 0.3, 2.0, (-7.0,) * 3, (7.0,) * 3, True)
    times = (1.33, 0.17, 1.46)
    x, _ = M.random_trajectory(10, 3, 4242, times)
    return x, times, grid, prm


def check_edge_rules(call):
    """Shared with the device test: call(N, x [B][V][h][3], times [B][K], g, p, increment_time) -> dict."""
    x, times, grid, prm = _edge_inputs()
    g, p = M.to_native(grid, prm)
    # T[1] = 0.17 in (0.1, inc] with inc = 0.25: NaN for n = 1 only
    out = call(10, x[None], np.array([times]), g, p, 0.25)
    mdl = TM.model(10, x, times, grid, prm, 0.25, truth=False)
    assert mdl["sides"][1, 0] is None and mdl["sides"][1, 1] is None and mdl["margin"] >= 1e-9
    assert out["status"][0] == 0
    assert np.isnan(out["grad_t"][0, 1]) and np.isnan(out["side_cost"][0, 1]).all()
    assert (out["side_evaluated"][0, 1] == 0).all()
    assert np.isfinite(out["grad_t"][0, [0, 2]]).all() and np.isfinite(out["side_cost"][0, [0, 2]]).all()
    TM.check_sides("NaN rule", {k: out[k][0] for k in ("grad_t", "side_cost", "side_evaluated")}, mdl, 0.25)
    # a non-positive, infinite or NaN time: BAD_TIME, every output NaN, counts 0, for that trajectory only
    xs = np.repeat(x[None], 5, axis=0)
    ts = np.array([times, (1.33, 0.0, 1.46), (1.33, -1.0, 1.46), (np.nan, 0.17, 1.46), (1.33, 0.17, np.inf)])
    out = call(10, xs, ts, g, p, 0.1)
    assert list(out["status"]) == [0] + [nat.MTG_TRAJ_BAD_TIME] * 4
    assert np.isfinite(out["grad_t"][0]).all() and np.isnan(out["grad_t"][1:]).all()
    assert np.isnan(out["side_cost"][1:]).all() and (out["side_evaluated"][1:] == 0).all()
    # too many clock samples in a perturbed segment: (T + inc) / dt > 2^24
    tiny = M.Params(1e-7, 0.2, 1.0, 0.3, 2.0, (-7.0,) * 3, (7.0,) * 3, True)
    out = call(10, x[None], np.array([(1.33, 1.62, 1.46)]), *M.to_native(grid, tiny), 0.1)
    assert out["status"][0] == nat.MTG_TRAJ_BAD_TIME and np.isnan(out["grad_t"]).all()
    # increment_time must be > 0 and finite
    for bad in (0.0, -0.1, np.inf, np.nan):
        with pytest.raises(mtg.MTGError) as e:
            call(10, x[None], np.array([times]), g, p, bad)
        assert e.value.code == nat.MTG_ERR_INVALID_ARGUMENT, bad
    # the argument errors of the collision call
    with pytest.raises(mtg.MTGError) as e:  # D != 3
        call(10, np.zeros((1, 4, 5, 2)), np.array([times]), g, p, 0.1)
    assert e.value.code == nat.MTG_ERR_INVALID_ARGUMENT
    with pytest.raises(mtg.MTGError) as e:  # N = 4
        call(4, np.zeros((1, 4, 2, 3)), np.array([times]), g, p, 0.1)
    assert e.value.code == nat.MTG_ERR_UNSUPPORTED_N
    with pytest.raises(mtg.MTGError) as e:
        call(10, x[None], np.array([times]), *M.to_native(grid, M.Params(0.0, 0.2, 1.0, 0.3, 2.0, (-7.0,) * 3, (7.0,) * 3,
                                                                          True)), 0.1)
    assert e.value.code == nat.MTG_ERR_INVALID_ARGUMENT


def test_edge_rules_on_the_host():
    check_edge_rules(lambda N, x, t, g, p, inc: mtg.host_collision_time_gradient_batch(N, x, t, g, p, increment_time=inc))


def test_threads_and_null_outputs_do_not_change_the_bits():
    c = TM.early_case(0.2)
    g, p = M.to_native(c["grid"], c["prm"])
    one = mtg.host_collision_time_gradient_batch(c["N"], c["x"], c["times"], g, p, threads=1)
    three = mtg.host_collision_time_gradient_batch(c["N"], c["x"], c["times"], g, p, threads=3)
    for k in one:
        assert one[k].tobytes() == three[k].tobytes(), k
    lib = nat.load()
    import ctypes
    grad = np.empty_like(one["grad_t"])
    gn, keep = g.native()
    x, t = np.ascontiguousarray(c["x"]), np.ascontiguousarray(c["times"])
    nat.check(lib.mtg_host_collision_time_gradient_batch(c["N"], 3, c["K"], len(x), x.ctypes.data, t.ctypes.data,
                                                         ctypes.byref(gn), ctypes.byref(p.native()), 0.1,
                                                         grad.ctypes.data, None, None, None, 1))
    del keep
    assert grad.tobytes() == one["grad_t"].tobytes()
