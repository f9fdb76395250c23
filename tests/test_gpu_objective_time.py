"""objectiveFunctionTime / objectiveFunctionTimeAndConstraints on the device (mtg_objective_time_batch,
csrc/mtg_objective.hip around the component launchers): the parts against the existing device entry
points called separately on the same context (byte for byte), the outputs against the numpy
recombination (byte for byte), device against host within what the component tests allow, the
stale-L_ collision term against the FP64 restatement of the reference loop, the hard-constraint
outputs, device pointers with an asynchronous call on a device-resident state, independence of batch
position and size, and the nullable outputs."""
import numpy as np
import pytest

import mav_trajectory_generation_cmake_amd as mtg
from mav_trajectory_generation_cmake_amd import _native as nat

import _objective_cases as OC
import _objective_time_cases as TC
import _soft_constraint_model as SM
from test_gpu_collision import _compare_with_host as compare_collision_with_host
from test_objective_time_host import ALL, check_stale

pytestmark = pytest.mark.gpu


def _same(a, b, what):
    assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), what


def _dev3(ctx, c, coeff_times=None, soft=True, x=None, **kw):
    prm = TC.params(c, 3, soft=soft)
    args = TC.call_args(c, prm, coeff_times, soft=soft or kw.get("constraint_values") or kw.get("maxima"))
    return prm, ctx.objective_time_batch(c["N"], c["values"], c["mask"], TC.x3(c) if x is None else x, prm, **args, **kw)


def _dev4(ctx, c, free_in, soft=True, **kw):
    prm = TC.params(c, 4, soft=soft)
    args = TC.call_args(c, prm, soft=soft or kw.get("constraint_values") or kw.get("maxima"))
    return prm, ctx.objective_time_batch(c["N"], c["values"], c["mask"], TC.x4(c, free_in), prm, **args, **kw)


@pytest.mark.parametrize("name", TC.SHAPES)
def test_parts_recombination_and_host(gpu_ctx, name):
    """GPU items 1 and 2 on every shape and both objectives."""
    c = TC.shape(name)
    N, r, T, mask = c["N"], c["r"], c["times"], c["mask"]
    assert nat.load().mtg_solve_kernel(N, c["D"], c["K"], r, 0) == c.get("kernel", nat.MTG_KERNEL_COLUMN)
    # ---- objective 3, coeff_times equal to the times
    prm, out = _dev3(gpu_ctx, c, state=OC.zero_state(c["B"]), **ALL)
    assert (out["status"] & nat.MTG_TRAJ_ERROR_MASK == 0).all()
    sol = gpu_ctx.solve_linear_batch(N, r, c["values"], mask, T, free=True, cost=True, status=True)
    _same(out["weighted_costs"][:, 0], sol["cost"], "ct")
    _same(out["free"], sol["free"], "free")
    _same(out["coeffs"], sol["coeffs"], "coeffs")
    assert (out["status"] == sol["status"]).all()
    full = mtg.full_vertex_values(c["values"], mask, sol["free"], N)
    sc = gpu_ctx.soft_constraint_cost_batch(N, full, T, c["soft"])
    _same(out["J_sc"], sc["cost"], "J_sc")
    _same(out["maxima"], sc["maxima"], "maxima")
    limits = np.array([v for _, v in c["soft"].constraints])
    _same(out["constraint_values"], sc["maxima"]["value"] - limits[None, :], "constraint_values")
    coll = None
    if prm.w_c > 0.0:
        coll = gpu_ctx.collision_cost_batch(N, full, T, c["g"], c["p"])
        _same(out["J_c"], coll["cost"], "J_c")
        _same(out["collision"], coll["collision"], "collision")
    else:
        assert out["J_c"] is None and (out["collision"] == 0).all()
    TC.assert_recombination(prm, out, sol["cost"], T, label=name + " 3")
    # ---- objective 4 at x4 = [T; the solve's free derivatives]
    prm4, o4 = _dev4(gpu_ctx, c, sol["free"], state=OC.zero_state(c["B"]), **ALL)
    assert (o4["status"] == 0).all()
    J = gpu_ctx.cost_at_times_batch(N, r, full, T, np.ones((1, c["K"])))
    _same(o4["J_d"], J[:, 0], "J_d")
    _same(o4["J_sc"], sc["cost"], "J_sc (4)")
    _same(o4["maxima"], sc["maxima"], "maxima (4)")
    _same(o4["constraint_values"], out["constraint_values"], "constraint_values (4)")
    _same(o4["free"], sol["free"], "free (4)")
    _same(o4["coeffs"], gpu_ctx.coefficients_from_vertices_batch(N, full, T), "coeffs (4)")
    TC.assert_recombination(prm4, o4, o4["J_d"], T, label=name + " 4")
    for k in (2, 3):  # ctime and cs are objective 3's bytes; ct within the bound J_d has between paths
        _same(o4["weighted_costs"][:, k], out["weighted_costs"][:, k], k)
    jtol = 2e-6 if N == 12 else 2e-7
    assert (np.abs(o4["weighted_costs"][:, 0] - sol["cost"]) <= jtol * np.abs(sol["cost"])).all()

    # ---- device against host: each part within what its component's tests allow between the two
    h3 = mtg.host_objective_time_batch(N, c["values"], mask, TC.x3(c), prm, **TC.call_args(c, prm), **ALL)
    assert (out["status"] == h3["status"]).all() and (out["collision"] == h3["collision"]).all()
    ct_d, ct_h = out["weighted_costs"][:, 0], h3["weighted_costs"][:, 0]
    print("%s: max |ct - host| / ct = %.3e" % (name, np.max(np.abs(ct_d - ct_h) / np.abs(ct_h))))
    assert (np.abs(ct_d - ct_h) <= 2e-9 * np.abs(ct_h)).all()  # test_gpu_parity.py: 1e-9 either side of the golden cost
    _same(out["weighted_costs"][:, 2], h3["weighted_costs"][:, 2], "ctime against host")
    if coll is not None:
        hfull = mtg.full_vertex_values(c["values"], mask, h3["free"], N)
        hc = mtg.host_collision_cost_batch(N, hfull, T, c["g"], c["p"], threads=0)
        _same(hc["cost"], h3["J_c"], "host J_c")
        compare_collision_with_host(name, coll, hc)
    h4 = mtg.host_objective_time_batch(N, c["values"], mask, TC.x4(c, sol["free"]), prm4, **TC.call_args(c, prm4),
                                       parts=True)
    assert (np.abs(o4["J_d"] - h4["J_d"]) <= jtol * np.abs(h4["J_d"])).all()
    rows = range(c["B"]) if c["B"] <= 5 else (0, 33, 66)
    hm = (1 << (N // 2)) - 1
    for b in rows:  # the soft-constraint model's cost tolerance (one model per trajectory)
        m = SM.model_one(N, full[b], mask[b] & hm, T[b], c["soft_model"], grad=False)
        for dev, host in ((out, h3), (o4, h4)):
            assert abs(dev["J_sc"][b] - host["J_sc"][b]) <= m["cost_tol"], (b, dev["J_sc"][b], host["J_sc"][b])


@pytest.mark.parametrize("name,rows", [("masks", range(5)), ("batch67", (0, 1, 33, 66))])
def test_stale_coefficients_on_the_device(gpu_ctx, name, rows):
    c = TC.shape(name)
    stale = 1.07 * c["times"]
    _, fresh = _dev3(gpu_ctx, c, parts=True)
    _, got = _dev3(gpu_ctx, c, coeff_times=stale, parts=True)
    assert (got["status"] & nat.MTG_TRAJ_ERROR_MASK == 0).all()
    check_stale(name + " device", c, got, stale, rows)
    assert (got["J_c"] != fresh["J_c"]).any(), "coeff_times is ignored"
    for k in (0, 2, 3):
        _same(got["weighted_costs"][:, k], fresh["weighted_costs"][:, k], k)
    host = mtg.host_objective_time_batch(c["N"], c["values"], c["mask"], TC.x3(c), TC.params(c, 3), parts=True,
                                         **TC.call_args(c, TC.params(c, 3), stale))
    assert (got["collision"] == host["collision"]).all()
    assert (np.abs(got["J_c"] - host["J_c"]) <= 1e-6 * host["J_c"]).all()  # test_gpu_collision._compare_with_host's bound


@pytest.mark.parametrize("name", ("masks", "dl67", "col_d2"))
def test_hard_constraint_outputs_and_nullable_outputs(gpu_ctx, name):
    """GPU items 3 and 5."""
    c = TC.shape(name)
    state_on = OC.zero_state(c["B"])
    prm_on, on = _dev3(gpu_ctx, c, state=state_on, **ALL)
    prm_off, off = _dev3(gpu_ctx, c, soft=False, constraint_values=True, maxima=True, parts=True)
    _same(off["constraint_values"], on["constraint_values"], "constraint_values")
    _same(off["maxima"], on["maxima"], "maxima")
    _same(off["weighted_costs"][:, 3], np.zeros(c["B"]), "cs")
    TC.assert_recombination(prm_off, off, off["weighted_costs"][:, 0], c["times"], label=name + " soft off")
    _, none_off = _dev3(gpu_ctx, c, soft=False)
    _same(none_off["cost"], off["cost"], "cost without the hard-constraint outputs")
    # nothing optional requested: the bytes of cost_out and state do not change
    state_bare = OC.zero_state(c["B"])
    _, bare = _dev3(gpu_ctx, c, state=state_bare)
    _same(bare["cost"], on["cost"], "cost")
    _same(state_bare, state_on, "state")
    for o in (bare,):
        assert o["free"] is None and o["coeffs"] is None and o["maxima"] is None and o["constraint_values"] is None
    prm4, o4 = _dev4(gpu_ctx, c, on["free"], state=OC.zero_state(c["B"]), **ALL)
    s4 = OC.zero_state(c["B"])
    _, b4 = _dev4(gpu_ctx, c, on["free"], state=s4)
    _same(b4["cost"], o4["cost"], "cost (4)")
    _same(s4, o4["state"], "state (4)")


@pytest.fixture(scope="module")
def dev67(gpu_ctx):
    c = TC.shape("batch67")
    stale = 1.03 * c["times"]
    state = OC.zero_state(c["B"])
    _, first = _dev3(gpu_ctx, c, coeff_times=stale, state=state, **ALL)
    first["state"] = state.copy()
    _, second = _dev3(gpu_ctx, c, coeff_times=stale, state=state, x=TC.x3(c, 1.1 * c["times"]), **ALL)
    second["state"] = state.copy()
    return c, stale, first, second


KEYS = ("cost", "weighted_costs", "collision", "status", "constraint_values", "maxima", "free", "coeffs", "J_c", "J_sc",
        "J_t")


def test_device_pointers_async_on_a_device_resident_state(gpu_ctx, dev67):
    """GPU item 4: every array is a torch tensor, the state stays on the device over two asynchronous
    calls; the bytes are the host-pointer calls'."""
    import torch
    c, stale, first, second = dev67
    dv = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dv)  # noqa: E731
    tg = mtg.SdfGrid(t(c["grid"].field), c["grid"].origin, c["grid"].resolution, c["grid"].oob)
    values, mask, ct = t(c["values"]), t(c["mask"]), t(stale)
    state = torch.zeros((c["B"], 48), dtype=torch.uint8, device=dv)
    prm = TC.params(c, 3)
    try:
        for want, times in ((first, c["times"]), (second, 1.1 * c["times"])):
            out = gpu_ctx.objective_time_batch(c["N"], values, mask, t(TC.x3(c, times)), prm, coeff_times=ct, grid=tg,
                                               collision=c["p"], constraints=c["soft"], state=state, asynchronous=True,
                                               **ALL)
            torch.cuda.synchronize(dv)
            for k in KEYS:
                got = out[k].cpu().numpy()
                if k == "maxima":
                    got = np.ascontiguousarray(got).view(mtg.solver.EXTREMUM_DTYPE)[..., 0]
                _same(got, want[k], k)
            _same(state.cpu().numpy(), want["state"], "state")
    finally:
        gpu_ctx.reset_stream()


def test_bits_do_not_depend_on_batch_position_or_size(gpu_ctx, dev67):
    c, stale, want, _ = dev67
    prm = TC.params(c, 3)
    for j in (0, 33, 66):
        alone = gpu_ctx.objective_time_batch(c["N"], c["values"][j:j + 1], c["mask"][j:j + 1], TC.x3(c)[j:j + 1], prm,
                                             coeff_times=stale[j:j + 1], grid=c["g"], collision=c["p"],
                                             constraints=c["soft"], **ALL)
        for k in KEYS:
            _same(alone[k][0], want[k][j], (k, j))
    # objective 4: row 33 alone against in the batch
    _, o4 = _dev4(gpu_ctx, c, want["free"], **ALL)
    prm4 = TC.params(c, 4)
    x = TC.x4(c, want["free"])
    alone = gpu_ctx.objective_time_batch(c["N"], c["values"][33:34], c["mask"][33:34], x[33:34], prm4,
                                         constraints=c["soft"], **ALL)
    for k in ("cost", "weighted_costs", "constraint_values", "maxima", "free", "coeffs", "J_d", "J_sc", "J_t"):
        _same(alone[k][0], o4[k][33], (k, 33))


def test_row_too_short_and_bad_times_on_the_device(gpu_ctx):
    """With device pointers the row length is checked on the device: MTG_TRAJ_ROW_TOO_SHORT, NaN outputs,
    an untouched state.  A time <= 0 in x and a non-finite coeff_times entry: BAD_TIME for that row only."""
    import torch
    c = TC.shape("masks")
    dv = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dv)  # noqa: E731
    _, sol = _dev3(gpu_ctx, c, free=True)
    prm4 = TC.params(c, 4)
    x = TC.x4(c, sol["free"])
    _, good = _dev4(gpu_ctx, c, sol["free"])
    values, mask = t(c["values"]), t(c["mask"])
    try:
        short = t(x[:, :c["K"] + 26].copy())  # rows of K + 3 x (8, 9, 7, 10, 6): the second and the fourth do not fit
        state = torch.full((c["B"], 48), 7, dtype=torch.uint8, device=dv)
        out = gpu_ctx.objective_time_batch(c["N"], values, mask, short, prm4, constraints=c["soft"], state=state, free=True)
        torch.cuda.synchronize(dv)
        status, cost = out["status"].cpu().numpy(), out["cost"].cpu().numpy()
        assert list(status) == [0, nat.MTG_TRAJ_ROW_TOO_SHORT, 0, nat.MTG_TRAJ_ROW_TOO_SHORT, 0]
        assert np.isnan(cost[[1, 3]]).all() and cost[[0, 2, 4]].tobytes() == good["cost"][[0, 2, 4]].tobytes()
        assert np.isnan(out["free"].cpu().numpy()[[1, 3]]).all()
        assert (state.cpu().numpy()[[1, 3]] == 7).all()
        out = gpu_ctx.objective_time_batch(c["N"], values, mask, t(TC.x3(c)[:, :c["K"] - 1].copy()), TC.params(c, 3, w_c=0.0),
                                           constraints=c["soft"])
        torch.cuda.synchronize(dv)
        status = out["status"].cpu().numpy()  # (row 2 also carries the solve's WARN_DROPPED)
        assert (status & nat.MTG_TRAJ_ERROR_MASK == nat.MTG_TRAJ_ROW_TOO_SHORT).all()
        assert np.isnan(out["cost"].cpu().numpy()).all()
    finally:
        gpu_ctx.reset_stream()
    xb = TC.x3(c)
    xb[1, 2] = -1.0
    ctb = c["times"].copy()
    ctb[3, 0] = np.nan
    _, ok = _dev3(gpu_ctx, c, **ALL)
    state = OC.zero_state(c["B"])
    _, out = _dev3(gpu_ctx, c, coeff_times=ctb, x=xb, state=state, **ALL)
    bad = np.array([False, True, False, True, False])
    assert (out["status"][bad] & nat.MTG_TRAJ_BAD_TIME != 0).all() and (out["status"][~bad] & 255 == 0).all()
    for k in ("cost", "weighted_costs", "constraint_values", "free", "coeffs"):
        assert np.isnan(out[k][bad]).all(), k
        _same(out[k][~bad], ok[k][~bad], k)
    assert np.isnan(out["maxima"]["value"][bad]).all() and (out["collision"][bad] == 0).all()
    assert (state["n_iterations"] == np.where(bad, 0, 1)).all()


def test_invalid_arguments_on_the_device(gpu_ctx):
    c = TC.shape("masks")
    good = dict(coeff_times=c["times"], grid=c["g"], collision=c["p"], constraints=c["soft"])

    def code(prm, **kw):
        with pytest.raises(mtg.MTGError) as e:
            gpu_ctx.objective_time_batch(c["N"], c["values"], c["mask"], TC.x3(c), prm, **kw)
        return e.value.code

    inv = nat.MTG_ERR_INVALID_ARGUMENT
    assert code(mtg.ObjectiveTimeParams(2, c["r"], w_c=10.0), **good) == inv
    assert code(mtg.ObjectiveTimeParams(3, c["r"], w_c=10.0, reserved=2), **good) == inv
    for missing in ("coeff_times", "grid", "collision", "constraints"):
        assert code(TC.params(c, 3), **{k: v for k, v in good.items() if k != missing}) == inv, missing
    for extra in ("coeff_times", "grid", "collision"):
        assert code(TC.params(c, 3, w_c=0.0), constraints=c["soft"], **{extra: good[extra]}) == inv, extra
    with pytest.raises(mtg.MTGError) as e:  # x_stride < K on a host-pointer call
        gpu_ctx.objective_time_batch(c["N"], c["values"], c["mask"], TC.x3(c)[:, :2].copy(), TC.params(c, 3), **good)
    assert e.value.code == inv
    d2 = TC.shape("col_d2")
    with pytest.raises(mtg.MTGError) as e:
        gpu_ctx.objective_time_batch(d2["N"], d2["values"], d2["mask"], TC.x3(d2), TC.params(d2, 3, w_c=10.0),
                                     coeff_times=d2["times"], grid=c["g"], collision=c["p"], constraints=d2["soft"])
    assert e.value.code == inv
