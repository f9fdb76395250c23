"""The nonlinear objective in the optimiser's variables on the device (mtg_objective_batch,
csrc/mtg_objective.hip around the component launchers): its parts against the existing device entry
points called separately on the same context (byte for byte), its outputs against the numpy
recombination (byte for byte), device against host within what the component tests allow, device
pointers with an asynchronous call, independence of batch position and size, and the raise rule and
state over two calls on a device-resident state."""
import numpy as np
import pytest

import mav_trajectory_generation_cmake_amd as mtg

import _collision_time_model as TM
import _objective_cases as OC
import _soft_constraint_model as SM
from _objective_cases import call_args, params, shape, x_of
from test_gpu_collision import _compare_with_host as compare_collision_with_host
from test_objective_host import OUT_KEYS, error_rule_checks, invalid_calls, raise_rule_checks, run_invalid

pytestmark = pytest.mark.gpu


def _device(ctx, c, objective, soft=True, prm=None, x=None, **kw):
    prm = prm or params(c, objective, soft)
    kw = {**dict(parts=True), **kw}
    return ctx.objective_batch(c["N"], c["values"], c["mask"], x_of(c, objective) if x is None else x, prm,
                               **call_args(c, objective, soft), **kw)


def _separate_calls(ctx, c, objective, soft):
    """The five existing entry points on the full vertex values, as a caller composes them today."""
    N, r, K = c["N"], c["r"], c["K"]
    full, times, mask = c["full"], c["times"], c["mask"]
    ones = np.ones((1, K))
    J, g = ctx.cost_at_times_batch(N, r, full, times, ones, mask=mask, grad=True)
    sep = {"J_d": J[:, 0], "grad_d": np.ascontiguousarray(g[:, 0])}
    if objective >= 1:
        sep["coll"] = ctx.collision_cost_batch(N, full, times, c["g"], c["p"], mask=mask, grad=True)
    if soft:
        sep["soft"] = ctx.soft_constraint_cost_batch(N, full, times, c["soft"].native(), mask=mask, grad=True)
    if objective == 2:
        sep["dJd_dt"] = np.ascontiguousarray(ctx.time_jacobian_batch(N, r, full, times, ones, increment_time=TM.INC)[1][:, 0])
        sep["ct"] = ctx.collision_time_gradient_batch(N, full, times, c["g"], c["p"], increment_time=TM.INC)
    return sep


def _same(a, b, what):
    assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), what


@pytest.mark.parametrize("name", OC.SHAPES)
@pytest.mark.parametrize("objective", [0, 1, 2])
def test_parts_recombination_and_host(gpu_ctx, name, objective):
    """GPU items 1 and 2 on every shape and objective (soft constraints on; also off on the small shapes)."""
    c = shape(name)
    for soft in ((True, False) if name in ("masks", "k1", "nofree") else (True,)):
        prm = params(c, objective, soft)
        out = _device(gpu_ctx, c, objective, soft, state=OC.zero_state(c["B"]))
        assert (out["status"] == 0).all()
        sep = _separate_calls(gpu_ctx, c, objective, soft)
        _same(out["J_d"], sep["J_d"], "J_d")
        _same(out["grad_d"], sep["grad_d"], "grad_d")
        if objective >= 1:
            _same(out["J_c"], sep["coll"]["cost"], "J_c")
            _same(out["grad_c"], sep["coll"]["grad"], "grad_c")
            _same(out["collision"], sep["coll"]["collision"], "collision")
        if soft:
            _same(out["J_sc"], sep["soft"]["cost"], "J_sc")
            if objective >= 1:
                _same(out["grad_sc"], sep["soft"]["grad"], "grad_sc")
            else:
                assert out["grad_sc"] is None
        if objective == 2:
            _same(out["dJd_dt"], sep["dJd_dt"], "dJd_dt")
            _same(out["dJc_dt"], sep["ct"]["grad_t"], "dJc_dt")
        OC.assert_recombination(c, prm, out, label=(name, objective, soft))
        bare = _device(gpu_ctx, c, objective, soft, grad=False, parts=False, state=OC.zero_state(c["B"]))
        for k in ("cost", "weighted_costs", "collision", "status", "state"):
            _same(out[k], bare[k], "grad_out = NULL changed " + k)
        if soft:
            _compare_device_with_host(gpu_ctx, c, objective, out, sep)


def _compare_device_with_host(ctx, c, objective, out, sep):
    """GPU item 2: each part within what the existing tests allow between device and host for that
    component.  The objective's device parts are the separate device calls' bytes (asserted above) and
    its host parts the separate host calls' (tests/test_objective_host.py), so the component tests'
    own comparisons run on those results: test_gpu_collision._compare_with_host, TM.compare_with_host,
    and the soft-constraint model's tolerances as SM.compare applies them with other = the host path.
    The derivative term: the bounds test_gpu_parity.py grants either side against the oracle, doubled."""
    N = c["N"]
    host = mtg.host_objective_batch(N, c["values"], c["mask"], x_of(c, objective), params(c, objective),
                                    **call_args(c, objective), parts=True, threads=0)
    assert (out["status"] == host["status"]).all() and (out["collision"] == host["collision"]).all()
    nt = c["K"] if objective == 2 else 0
    for b in range(c["B"]):  # the n_free-dependent padding
        n = nt + c["D"] * int(c["n_free"][b])
        assert (out["grad"][b, n:] == 0.0).all() and (host["grad"][b, n:] == 0.0).all()
        assert np.isfinite(out["grad"][b, :n]).all() and np.isfinite(host["grad"][b, :n]).all()
    jtol = 2e-6 if N == 12 else 2e-7
    assert (np.abs(out["J_d"] - host["J_d"]) <= jtol * np.abs(host["J_d"])).all()
    gmax = np.max(np.abs(host["grad_d"]), axis=(1, 2), keepdims=True)
    assert (np.abs(out["grad_d"] - host["grad_d"]) <= 2e-6 * gmax).all()
    if objective >= 1:
        hc = {"cost": host["J_c"], "grad": host["grad_c"], "collision": host["collision"], "status": host["status"],
              "n_evaluated": mtg.host_collision_cost_batch(N, c["full"], c["times"], c["g"], c["p"], threads=0)["n_evaluated"]}
        _same(hc["cost"], mtg.host_collision_cost_batch(N, c["full"], c["times"], c["g"], c["p"], threads=0)["cost"], "host J_c")
        compare_collision_with_host(c["name"], sep["coll"], hc)
    rows = range(c["B"]) if c["B"] <= 5 else (0, 33, 66)
    for b in rows:  # the soft-constraint model's tolerances (one model per trajectory: a few rows of the large batch)
        m = SM.model_one(N, c["full"][b], c["mask"][b] & ((1 << (N // 2)) - 1), c["times"][b], c["soft"],
                         grad=objective >= 1)
        assert abs(out["J_sc"][b] - host["J_sc"][b]) <= m["cost_tol"], (b, out["J_sc"][b], host["J_sc"][b], m["cost_tol"])
        if objective >= 1:
            assert (np.abs(out["grad_sc"][b] - host["grad_sc"][b]) <= m["grad_tol"]).all(), b
    if objective == 2:
        hct = mtg.host_collision_time_gradient_batch(N, c["full"], c["times"], c["g"], c["p"], increment_time=TM.INC,
                                                     threads=0)
        _same(hct["grad_t"], host["dJc_dt"], "host dJc_dt")
        TM.compare_with_host(c["name"], sep["ct"], hct)
        J = np.abs(host["J_d"])[:, None]
        tol = 2.0 * (2e-6 * J / TM.INC + 1e-7 * np.max(np.abs(host["dJd_dt"]), axis=1, keepdims=True))
        assert (np.abs(out["dJd_dt"] - host["dJd_dt"]) <= tol).all()


@pytest.fixture(scope="module")
def dev67(gpu_ctx):
    c = shape("batch67")
    return c, _device(gpu_ctx, c, 2, state=OC.zero_state(c["B"]))


def test_batch67_mixes_colliding_and_free_trajectories(dev67):
    c, out = dev67
    host = mtg.host_collision_cost_batch(c["N"], c["full"], c["times"], c["g"], c["p"], threads=0)
    assert host["collision"].any() and not host["collision"].all()
    assert (out["collision"] == host["collision"]).all()


def _to_device(c, objective, dv):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dv)  # noqa: E731
    tg = mtg.SdfGrid(t(c["grid"].field), c["grid"].origin, c["grid"].resolution, c["grid"].oob)
    kw = dict(times=None if objective == 2 else t(c["times"]), soft=c["soft"].native())
    if objective >= 1:
        kw.update(grid=tg, collision=c["p"])
    return t(c["values"]), t(c["mask"]), t(x_of(c, objective)), kw


def test_device_pointers_async_same_bits(gpu_ctx, dev67):
    """GPU item 3: x, values, mask, grad_out, the parts and the state are torch tensors, one
    torch.cuda.synchronize after the call; the bytes are the host-pointer call's."""
    import torch
    c, want = dev67
    dv = torch.device("cuda", 0)
    values, mask, x, kw = _to_device(c, 2, dv)
    state = torch.zeros((c["B"], 48), dtype=torch.uint8, device=dv)
    out = gpu_ctx.objective_batch(c["N"], values, mask, x, params(c, 2), state=state, parts=True, asynchronous=True, **kw)
    torch.cuda.synchronize(dv)
    gpu_ctx.reset_stream()
    for k in OUT_KEYS + mtg.solver.OBJECTIVE_PARTS:
        _same(out[k].cpu().numpy(), want[k], k)
    _same(state.cpu().numpy(), want["state"], "state")


def test_bits_do_not_depend_on_batch_position_or_size(gpu_ctx, dev67):
    """GPU item 4: row 0 alone, and moved to row 66."""
    c, want = dev67
    alone = gpu_ctx.objective_batch(c["N"], c["values"][:1], c["mask"][:1], c["x_time"][:1], params(c, 2),
                                    **call_args(c, 2), parts=True)
    values, mask, x = c["values"].copy(), c["mask"].copy(), c["x_time"].copy()
    values[66], mask[66], x[66] = values[0], mask[0], x[0]
    moved = gpu_ctx.objective_batch(c["N"], values, mask, x, params(c, 2), **call_args(c, 2), parts=True)
    for k in OUT_KEYS + mtg.solver.OBJECTIVE_PARTS:
        for res, j in ((alone, 0), (moved, 66), (moved, 0)):
            _same(res[k][j], want[k][0], (k, j))
        _same(moved[k][1:66], want[k][1:66], k)


def test_raise_rule_on_a_device_resident_state(gpu_ctx):
    """GPU item 5: two consecutive device-pointer calls on one device-resident state reproduce the host
    test's expectations (the numpy recombination of the parts)."""
    import torch
    c = shape("batch67")
    dv = torch.device("cuda", 0)
    values, mask, _, kw = _to_device(c, 2, dv)

    def call(prm, state, x):
        st = torch.from_numpy(state.view(np.uint8).reshape(c["B"], 48).copy()).to(dv)
        out = gpu_ctx.objective_batch(c["N"], values, mask, torch.from_numpy(np.ascontiguousarray(x)).to(dv), prm,
                                      state=st, parts=True, **kw)
        res = {k: (v.cpu().numpy() if v is not None and k != "state" else v) for k, v in out.items()}
        res["state"] = np.ascontiguousarray(st.cpu().numpy()).view(mtg.OBJECTIVE_STATE_DTYPE)[:, 0]
        return res

    try:
        raise_rule_checks(call, c)
    finally:
        gpu_ctx.reset_stream()


def test_bad_time_in_x_on_the_device(gpu_ctx):
    c = shape("masks")
    error_rule_checks(lambda x, state: _device(gpu_ctx, c, 2, x=x, state=state), c)


@pytest.mark.parametrize("which", range(10))
def test_invalid_arguments(gpu_ctx, which):
    c = shape("masks")
    label, objective, over = list(invalid_calls(c))[which]
    run_invalid(gpu_ctx.objective_batch, c, label, objective, over)


def test_row_too_short_with_device_pointers(gpu_ctx):
    """With device pointers the mask is not read on the host: a row longer than x_stride is found by
    the unpack kernel, its x is not read, and the trajectory gets MTG_TRAJ_ROW_TOO_SHORT and NaN outputs."""
    import torch
    from mav_trajectory_generation_cmake_amd import _native as nat
    c = shape("masks")
    dv = torch.device("cuda", 0)
    values, mask, x, kw = _to_device(c, 0, dv)
    good = gpu_ctx.objective_batch(c["N"], values, mask, x, params(c, 0), **kw)
    short = x[:, :26].contiguous()  # rows of 3 x (8, 9, 7, 10, 6) entries: the second and the fourth do not fit
    out = gpu_ctx.objective_batch(c["N"], values, mask, short, params(c, 0), **kw)
    gpu_ctx.reset_stream()
    assert list(out["status"].cpu().numpy()) == [0, nat.MTG_TRAJ_ROW_TOO_SHORT, 0, nat.MTG_TRAJ_ROW_TOO_SHORT, 0]
    cost, gcost = out["cost"].cpu().numpy(), good["cost"].cpu().numpy()
    assert np.isnan(cost[[1, 3]]).all() and cost[[0, 2, 4]].tobytes() == gcost[[0, 2, 4]].tobytes()
    assert np.isnan(out["grad"].cpu().numpy()[[1, 3]]).all()
