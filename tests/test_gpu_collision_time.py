"""Segment-time gradient of the collision cost on the device (mtg_collision_time_gradient_batch,
csrc/mtg_collision_time.hip) against the FP64 restatement of the reference's getCostAndGradientTime
walks, its 50-digit twin and the early-stop rule (tests/_collision_time_model.py), and against the
library's host path."""
import numpy as np
import pytest

import mav_trajectory_generation_cmake_amd as mtg
from mav_trajectory_generation_cmake_amd import _native as nat

import _collision_model as M
import _collision_time_model as TM
from test_collision_time_host import _edge_inputs, _row, check_edge_rules

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [c["name"] for c in M.CASES])
def test_device_against_model_truth_and_host(gpu_ctx, name):
    c = M.build_case(name)
    g, p = M.to_native(c["grid"], c["prm"])
    dev = gpu_ctx.collision_time_gradient_batch(c["N"], c["x"], c["times"], g, p, increment_time=TM.INC)
    host = mtg.host_collision_time_gradient_batch(c["N"], c["x"], c["times"], g, p, increment_time=TM.INC)
    assert (dev["status"] == 0).all()
    for j, mdl in enumerate(TM.case_models(name)):
        assert mdl["margin"] >= 1e-9, "the seed puts a comparison other than the clock on the edge"
        TM.check_sides("%s[%d]" % (name, j), _row(dev, j), mdl, TM.INC)
        assert dev["segments_walked"][j] == mdl["segments_walked"]
    TM.compare_with_host(name, dev, host)
    if name == "short-segment":  # T = 0.07 <= 0.1: both sides 0.1, the clock tie t == T' == 0.1
        assert (dev["grad_t"][:, 1] == 0.0).all() and not np.signbit(dev["grad_t"][:, 1]).any()


@pytest.mark.parametrize("map_resolution", [0.2, 1.5])
def test_early_stop_both_ways(gpu_ctx, map_resolution):
    """segments_walked is the model's count: 4K - 2 where every perturbation rejoins at n+2 (0.2), more
    where some rejoin later or never (1.5; what the inputs contain is asserted in
    test_collision_time_host.py::test_early_stop_inputs_on_the_host)."""
    c = TM.early_case(map_resolution)
    K = c["K"]
    g, p = M.to_native(c["grid"], c["prm"])
    dev = gpu_ctx.collision_time_gradient_batch(c["N"], c["x"], c["times"], g, p, increment_time=TM.INC)
    host = mtg.host_collision_time_gradient_batch(c["N"], c["x"], c["times"], g, p, increment_time=TM.INC)
    want = [mdl["segments_walked"] for mdl in c["models"]]
    print("segments_walked", list(dev["segments_walked"]), "model", want)
    assert list(dev["segments_walked"]) == want
    if map_resolution == 0.2:
        assert all(mdl["margin"] >= 1e-9 for mdl in c["models"]) and want == [4 * K - 2] * len(want)
    else:
        assert any(s["rejoined"] is False and n + 2 < K for mdl in c["models"] for (n, _), s in mdl["sides"].items())
        assert max(want) > 4 * K - 2
    for j, mdl in enumerate(c["models"]):
        assert mdl["margin"] >= 1e-9
        TM.check_sides("early %.1f [%d]" % (map_resolution, j), _row(dev, j), mdl, TM.INC)
    TM.compare_with_host("early %.1f" % map_resolution, dev, host)


@pytest.mark.parametrize("inc", [0.1, 0.005])
def test_more_samples_than_a_chunk(gpu_ctx, inc):
    """Two segments of about 7 s at dt = 0.01: 700 samples per segment against chunks of 64; inc = 0.1 is
    ten samples more or fewer, inc = 0.005 less than one."""
    c = TM.long_case(inc)
    mdl = c["model"]
    assert mdl["margin"] >= 1e-9
    g, p = M.to_native(c["grid"], c["prm"])
    dev = gpu_ctx.collision_time_gradient_batch(c["N"], c["x"], c["times"], g, p, increment_time=inc)
    host = mtg.host_collision_time_gradient_batch(c["N"], c["x"], c["times"], g, p, increment_time=inc)
    TM.check_sides("long inc %g (host)" % inc, _row(host, 0), mdl, inc)
    TM.check_sides("long inc %g" % inc, _row(dev, 0), mdl, inc)
    TM.compare_with_host("long inc %g" % inc, dev, host)
    assert dev["segments_walked"][0] == mdl["segments_walked"]
    assert dev["side_evaluated"].min() > 2 * 64


def test_edge_rules_on_the_device(gpu_ctx):
    seen = []

    def call(N, x, t, g, p, inc):
        out = gpu_ctx.collision_time_gradient_batch(N, x, t, g, p, increment_time=inc)
        seen.append(out)
        return out

    check_edge_rules(call)
    # the NaN rule's perturbations walk nothing; a BAD_TIME trajectory walks nothing
    x, times, grid, prm = _edge_inputs()
    mdl = TM.model(10, x, times, grid, prm, 0.25, truth=False)
    assert seen[0]["segments_walked"][0] == mdl["segments_walked"]
    assert (seen[1]["segments_walked"][1:] == 0).all() and seen[1]["segments_walked"][0] > 0
    assert seen[2]["segments_walked"][0] == 0


def test_too_large_boundary(gpu_ctx):
    """include/mtg.h: one trajectory must fit 64 KiB of LDS, K <= 140 at N = 10.  K = 140 runs and agrees
    with the host path; K = 141 is MTG_ERR_TOO_LARGE."""
    N = 10
    grid = M.maps()["sphere"]
    prm = M.Params(0.1, 0.2, 1.0, 0.3, 2.0, (-7.0,) * 3, (7.0,) * 3, True)
    g, p = M.to_native(grid, prm)
    for K in (140, 141):
        times = tuple(0.23 + 0.01 * (i % 7) for i in range(K))
        x, _ = M.random_trajectory(N, K, 9000 + K, times)
        if K == 141:
            with pytest.raises(mtg.MTGError) as e:
                gpu_ctx.collision_time_gradient_batch(N, x[None], np.array([times]), g, p)
            assert e.value.code == nat.MTG_ERR_TOO_LARGE
            continue
        dev = gpu_ctx.collision_time_gradient_batch(N, x[None], np.array([times]), g, p)
        host = mtg.host_collision_time_gradient_batch(N, x[None], np.array([times]), g, p)
        mdl = TM.model(N, x, times, grid, prm, TM.INC, truth=False)
        assert mdl["margin"] >= 1e-9
        assert dev["status"][0] == 0 and np.isfinite(dev["grad_t"]).all()
        assert dev["segments_walked"][0] == mdl["segments_walked"]
        TM.check_sides("K = 140", _row(dev, 0), mdl, TM.INC)
        TM.compare_with_host("K = 140", dev, host)


@pytest.fixture(scope="module")
def batch67(gpu_ctx):
    """B = 67 trajectories of K = 8, N = 10 on the sphere map at the gate where some perturbations rejoin
    late or never."""
    N, K, B = 10, 8, 67
    xs = np.array([M.random_trajectory(N, K, 8200 + j, TM.EARLY_TIMES)[0] for j in range(B)])
    times = np.tile(np.array(TM.EARLY_TIMES), (B, 1)) * (1.0 + 0.003 * np.arange(B))[:, None]
    grid = M.maps()["sphere"]
    prm = M.Params(0.1, 1.5, 1.0, 0.3, 2.0, (-7.0,) * 3, (7.0,) * 3, True)
    g, p = M.to_native(grid, prm)
    dev = gpu_ctx.collision_time_gradient_batch(N, xs, times, g, p)
    models = [TM.model(N, xs[j], times[j], grid, prm, TM.INC, truth=False) for j in range(B)]
    return dict(N=N, K=K, B=B, x=xs, times=times, grid=grid, g=g, p=p, dev=dev, models=models)


KEYS = ("grad_t", "side_cost", "side_evaluated", "segments_walked", "status")


def test_bits_do_not_depend_on_batch_position_or_call(gpu_ctx, batch67):
    c = batch67
    x, times = c["x"].copy(), c["times"].copy()
    x[66], times[66] = x[0], times[0]
    moved = gpu_ctx.collision_time_gradient_batch(c["N"], x, times, c["g"], c["p"])
    alone = gpu_ctx.collision_time_gradient_batch(c["N"], x[:1], times[:1], c["g"], c["p"])
    for out, j in ((moved, 66), (moved, 0), (alone, 0)):
        for k in KEYS:
            assert out[k][j].tobytes() == c["dev"][k][0].tobytes(), k
    for k in KEYS:
        assert moved[k][1:66].tobytes() == c["dev"][k][1:66].tobytes(), k
    # the nullable outputs do not change grad_t
    bare = gpu_ctx.collision_time_gradient_batch(c["N"], c["x"], c["times"], c["g"], c["p"], diagnostics=False)
    assert bare["side_cost"] is None and bare["grad_t"].tobytes() == c["dev"]["grad_t"].tobytes()
    # and the batch agrees with the model and the host path
    for j, mdl in enumerate(c["models"]):
        assert mdl["margin"] >= 1e-9, j
        assert c["dev"]["segments_walked"][j] == mdl["segments_walked"], j
    TM.check_sides("B = 67 [33]", _row(c["dev"], 33), c["models"][33], TM.INC)
    host = mtg.host_collision_time_gradient_batch(c["N"], c["x"], c["times"], c["g"], c["p"], threads=0)
    TM.compare_with_host("B = 67", c["dev"], host)
    assert c["dev"]["segments_walked"].max() > 4 * c["K"] - 2  # some perturbation rejoins late or never


def test_device_pointers_async_same_bits(gpu_ctx, batch67):
    import torch
    c = batch67
    dv = torch.device("cuda", 0)
    tg = mtg.SdfGrid(torch.from_numpy(c["grid"].field).to(dv), c["grid"].origin, c["grid"].resolution, c["grid"].oob)
    out = gpu_ctx.collision_time_gradient_batch(c["N"], torch.from_numpy(c["x"]).to(dv),
                                                torch.from_numpy(c["times"]).to(dv), tg, c["p"], asynchronous=True)
    torch.cuda.synchronize(dv)
    gpu_ctx.reset_stream()
    for k in KEYS:
        assert out[k].cpu().numpy().tobytes() == c["dev"][k].tobytes(), k


def test_time_gradient_is_the_composition(gpu_ctx, batch67):
    c = batch67
    N, r, w = c["N"], 4, (0.1, 10.0, 1.0)
    x, times = c["x"][:5], c["times"][:5]
    out = gpu_ctx.time_gradient_batch(N, r, x, times, c["g"], c["p"], weights=w, increment_time=0.1)
    _, jd = gpu_ctx.time_jacobian_batch(N, r, x, times, np.ones((1, c["K"])), increment_time=0.1)
    jc = gpu_ctx.collision_time_gradient_batch(N, x, times, c["g"], c["p"], increment_time=0.1)["grad_t"]
    assert out["dJd_dt"].tobytes() == jd[:, 0, :].tobytes() and out["dJc_dt"].tobytes() == jc.tobytes()
    assert out["dJc_dt"].tobytes() == c["dev"]["grad_t"][:5].tobytes()
    assert out["grad_t"].tobytes() == ((w[0] * jd[:, 0, :] + w[1] * jc) + w[2]).tobytes()
    assert out["J_t"].tobytes() == times.sum(1).tobytes() and (out["status"] == 0).all()
    assert np.isfinite(out["grad_t"]).all() and np.abs(out["dJc_dt"]).max() > 0
