"""The host path of mtg_objective_time_batch (mtg_host_objective_time_batch: objectiveFunctionTime and
objectiveFunctionTimeAndConstraints, nl_impl:765-906) and mtg_host_objective_time_bounds_batch, without
a GPU: its parts against the separate host entry points byte for byte, the stale-L_ collision term
against the FP64 restatement of the reference loop, the combination against a numpy scalar restatement,
the two objectives against each other, the errors and the bounds."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mav_trajectory_generation_cmake_amd as mtg
from mav_trajectory_generation_cmake_amd import _native as nat

import _collision_model as M
import _objective_cases as OC
import _objective_time_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = dict(parts=True, constraint_values=True, maxima=True, free=True, coeffs=True)


def _host3(c, coeff_times=None, soft=True, **kw):
    prm = TC.params(c, 3, soft=soft)
    args = TC.call_args(c, prm, coeff_times, soft=soft or kw.get("constraint_values") or kw.get("maxima"))
    return prm, mtg.host_objective_time_batch(c["N"], c["values"], c["mask"], TC.x3(c), prm, **args, **kw)


def _host4(c, free_in, soft=True, **kw):
    prm = TC.params(c, 4, soft=soft)
    args = TC.call_args(c, prm, soft=soft or kw.get("constraint_values") or kw.get("maxima"))
    return prm, mtg.host_objective_time_batch(c["N"], c["values"], c["mask"], TC.x4(c, free_in), prm, **args, **kw)


def test_abi_version_is_5():
    assert nat.load().mtg_abi_version() == 5


def test_generated_shapes_select_their_solve_kernels():
    lib = nat.load()
    for name, (N, D, K, B, r, _, _, kernel) in TC.GENERATED.items():
        assert lib.mtg_solve_kernel(N, D, K, r, 0) == kernel, name


@pytest.mark.parametrize("name", TC.SHAPES)
def test_parts_byte_for_byte(name):
    """Objective 3 with coeff_times equal to the times: ct, free, coeffs, J_sc, maxima, J_c are the bytes of
    the separate host entry points composed by hand; objective 4 at the same trajectory likewise."""
    c = TC.shape(name)
    N, T = c["N"], c["times"]
    prm, out = _host3(c, **ALL)
    assert (out["status"] & nat.MTG_TRAJ_ERROR_MASK == 0).all()
    hs = mtg.host_solve_linear_batch(N, c["r"], c["values"], c["mask"], T, free=True, cost=True, status=True)
    assert out["weighted_costs"][:, 0].tobytes() == hs["cost"].tobytes()
    assert out["free"].tobytes() == hs["free"].tobytes() and out["coeffs"].tobytes() == hs["coeffs"].tobytes()
    assert (out["status"] == hs["status"]).all()
    full = mtg.full_vertex_values(c["values"], c["mask"], hs["free"], N)
    sc = mtg.host_soft_constraint_cost_batch(N, full, T, c["soft"])
    assert out["J_sc"].tobytes() == sc["cost"].tobytes() and out["maxima"].tobytes() == sc["maxima"].tobytes()
    limits = np.array([v for _, v in c["soft"].constraints])
    assert out["constraint_values"].tobytes() == (sc["maxima"]["value"] - limits[None, :]).tobytes()
    if prm.w_c > 0.0:
        cc = mtg.host_collision_cost_batch(N, full, T, c["g"], c["p"])
        assert out["J_c"].tobytes() == cc["cost"].tobytes() and (out["collision"] == cc["collision"]).all()
    else:
        assert out["J_c"] is None and (out["collision"] == 0).all() and (out["weighted_costs"][:, 1] == 0).all()
    assert out["J_d"] is None and out["grad"] is None
    # objective 4 at x4 = [T; the solve's free derivatives]
    prm4, o4 = _host4(c, hs["free"], **ALL)
    assert o4["J_sc"].tobytes() == sc["cost"].tobytes() and o4["maxima"].tobytes() == sc["maxima"].tobytes()
    assert o4["free"].tobytes() == hs["free"].tobytes()
    want = np.empty_like(o4["coeffs"])
    nat.check(nat.load().mtg_host_coefficients_from_vertices_batch(N, c["D"], c["K"], c["B"], full.ctypes.data,
                                                                   T.ctypes.data, want.ctypes.data, 1))
    assert o4["coeffs"].tobytes() == want.tobytes()
    # the host J_d of mtg_host_objective_batch (its objective 0 reads the same free blocks, without the times)
    o0 = mtg.host_objective_batch(N, c["values"], c["mask"], TC.x4(c, hs["free"])[:, c["K"]:].copy(),
                                  mtg.ObjectiveParams(0, c["r"], use_soft_constraints=False), times=T, grad=False,
                                  parts=True)
    assert o4["J_d"].tobytes() == o0["J_d"].tobytes()
    assert o4["weighted_costs"][:, 0].tobytes() == (np.float64(0.5) * o4["J_d"]).tobytes()
    assert o4["J_c"] is None and (o4["weighted_costs"][:, 1] == 0).all() and (o4["collision"] == 0).all()


def stale_model(c, coeff_times, rows):
    """The FP64 restatement of the reference loop with the coefficients formed at coeff_times and the clock
    bounds from the times, per row: dict(cost, S_J, flag, n_eval)."""
    hs = mtg.host_solve_linear_batch(c["N"], c["r"], c["values"], c["mask"], c["times"], free=True)
    full = mtg.full_vertex_values(c["values"], c["mask"], hs["free"], c["N"])
    out = {}
    for b in rows:
        co = M.host_coefficients(c["N"], full[b], coeff_times[b])
        coeffs = [[[float(v) for v in co[i, k]] for k in range(3)] for i in range(c["K"])]
        rec = M._Margins()
        r = M._loop(M._F64, c["N"], coeffs, [float(t) for t in c["times"][b]], c["grid"], c["prm"], False, rec=rec)
        out[b] = dict(cost=r["J"], S_J=r["S_J"], flag=r["flag"], n_eval=r["n_eval"], margin=rec.smallest())
    return out


def check_stale(label, c, got, coeff_times, rows):
    """J_c and the collision flag of a call with coeff_times against stale_model, with the tolerance
    _collision_model.check_against applies against the model (1e-6 S_J)."""
    model = stale_model(c, coeff_times, rows)
    for b in rows:
        assert model[b]["margin"] >= 1e-9, "the seed puts a comparison on the edge"
        M.check_against("%s[%d]" % (label, b), got["J_c"][b], None, model[b])
        assert bool(got["collision"][b]) == model[b]["flag"], (label, b)


@pytest.mark.parametrize("name,rows", [("masks", range(5)), ("batch67", (0, 1, 33, 66))])
def test_stale_coefficients(name, rows):
    """coeff_times = 1.07 x the times: the walk follows the polynomials of the stale times to the clock
    bounds of the new ones.  (The ABI has no evaluated-sample output; the count enters through J_c.)"""
    c = TC.shape(name)
    stale = 1.07 * c["times"]
    _, fresh = _host3(c, parts=True)
    _, got = _host3(c, coeff_times=stale, parts=True)
    check_stale(name, c, got, stale, rows)
    assert (got["J_c"] != fresh["J_c"]).any(), "coeff_times is ignored"
    # everything but the collision term is untouched by coeff_times
    for k in (0, 2, 3):
        assert got["weighted_costs"][:, k].tobytes() == fresh["weighted_costs"][:, k].tobytes()


@pytest.mark.parametrize("name", TC.SHAPES)
def test_recombination_and_state(name):
    c = TC.shape(name)
    T = c["times"]
    state = OC.zero_state(c["B"])
    prm, out = _host3(c, state=state, parts=True, free=True)
    first = TC.assert_recombination(prm, out, out["weighted_costs"][:, 0], T, label=name + " 3")
    assert (state["iter0_done"] == 1).all() and state["total_cost_iter0"].tobytes() == out["cost"].tobytes()
    free = out["free"]
    # a second call on the carried state with other times: total_cost_iter0 stays
    c2 = dict(c, times=1.1 * T)
    before = state.copy()
    prm = TC.params(c, 3)
    out2 = mtg.host_objective_time_batch(c["N"], c["values"], c["mask"], TC.x3(c2), prm, state=state, parts=True,
                                         **TC.call_args(c, prm))
    TC.assert_recombination(prm, out2, out2["weighted_costs"][:, 0], c2["times"], before, label=name + " 3 second")
    assert state["total_cost_iter0"].tobytes() == first["state"]["total_cost_iter0"].tobytes()
    assert (state["n_iterations"] == 2).all()
    # objective 4 on a state of sentinels: cost_collision and the iter0 fields are never touched
    sent = OC.zero_state(c["B"])
    sent["cost_collision"], sent["total_cost_iter0"], sent["iter0_done"], sent["n_iterations"] = -3.25, 77.5, 0, 40
    for _ in range(2):
        before = sent.copy()
        prm4, o4 = _host4(c, free, state=sent, parts=True)
        TC.assert_recombination(prm4, o4, o4["J_d"], T, before, label=name + " 4")
    assert (sent["cost_collision"] == -3.25).all() and (sent["total_cost_iter0"] == 77.5).all()
    assert (sent["iter0_done"] == 0).all() and (sent["n_iterations"] == 42).all()
    # soft constraints off: cs = +0.0, the hard-constraint outputs keep their bytes, nothing else moves
    _, on = _host3(c, constraint_values=True, maxima=True)
    prm_off, off = _host3(c, soft=False, constraint_values=True, maxima=True, parts=True)
    assert off["constraint_values"].tobytes() == on["constraint_values"].tobytes()
    assert off["maxima"].tobytes() == on["maxima"].tobytes()
    assert off["weighted_costs"][:, 3].tobytes() == np.zeros(c["B"]).tobytes()
    TC.assert_recombination(prm_off, off, off["weighted_costs"][:, 0], T, label=name + " soft off")
    _, bare = _host3(c, soft=False)
    assert bare["cost"].tobytes() == off["cost"].tobytes()


@pytest.mark.parametrize("name", TC.SHAPES)
def test_objectives_3_and_4_agree(name):
    """At x4 = [T; free_out of objective 3 at T] objective 4's ctime and cs are objective 3's bytes; its ct
    (0.5 d^T R d) agrees with the solve's cost within the bound test_gpu_objective.py grants J_d between
    paths (2e-7; N = 12: 2e-6)."""
    c = TC.shape(name)
    _, o3 = _host3(c, free=True)
    _, o4 = _host4(c, o3["free"])
    for k in (2, 3):
        assert o4["weighted_costs"][:, k].tobytes() == o3["weighted_costs"][:, k].tobytes()
    a, b = o3["weighted_costs"][:, 0], o4["weighted_costs"][:, 0]
    rel = np.max(np.abs(a - b) / np.abs(a))
    print("%s: max |ct4 - ct3| / ct3 = %.3e" % (name, rel))
    assert rel <= (2e-6 if c["N"] == 12 else 2e-7)


def test_both_costs_against_the_golden_cost():
    """tests/golden/cfg2_n10_k10.npz is the shape N = 10, K = 10, D = 3 with the oracle's cost: both ct
    values are within the project's 1e-9 of it."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "cfg2_n10_k10.npz"))
    N, r = int(g["N"]), int(g["r"])
    c = dict(N=N, r=r, B=g["values"].shape[0], K=g["times"].shape[1], D=3, values=g["values"],
             mask=g["mask"].astype(np.uint8), times=g["times"], w_c=0.0,
             n_free=mtg.number_of_free_constraints(g["mask"].astype(np.uint8), N))
    _, o3 = _host3(c, soft=False, free=True)
    _, o4 = _host4(c, o3["free"], soft=False)
    for o in (o3, o4):
        rel = np.max(np.abs(o["weighted_costs"][:, 0] - g["cost"]) / np.abs(g["cost"]))
        print("max |ct - golden| / golden = %.3e" % rel)
        assert rel <= 1e-9


def test_errors():
    c = TC.shape("masks")
    N, T, B, K = c["N"], c["times"], c["B"], c["K"]
    good = dict(coeff_times=T, grid=c["g"], collision=c["p"], constraints=c["soft"])

    def code(prm, x=None, **kw):
        with pytest.raises(mtg.MTGError) as e:
            mtg.host_objective_time_batch(N, c["values"], c["mask"], TC.x3(c) if x is None else x, prm, **kw)
        return e.value.code

    inv = nat.MTG_ERR_INVALID_ARGUMENT
    for objective in (0, 1, 2, 5, -1):
        assert code(mtg.ObjectiveTimeParams(objective, c["r"], w_c=10.0), **good) == inv
    assert code(mtg.ObjectiveTimeParams(3, c["r"], w_c=10.0, reserved=1), **good) == inv
    p3 = TC.params(c, 3)
    for missing in ("coeff_times", "grid", "collision", "constraints"):
        assert code(p3, **{k: v for k, v in good.items() if k != missing}) == inv, missing
    p3n = TC.params(c, 3, w_c=0.0)
    for extra in ("coeff_times", "grid", "collision"):  # w_c <= 0: no collision term, so none of its arguments
        assert code(p3n, constraints=c["soft"], **{extra: good[extra]}) == inv, extra
    p4 = TC.params(c, 4)
    _, o3 = _host3(c, free=True)
    for extra in ("coeff_times", "grid", "collision"):
        assert code(p4, x=TC.x4(c, o3["free"]), constraints=c["soft"], **{extra: good[extra]}) == inv, extra
    assert code(p3, x=TC.x3(c)[:, :K - 1].copy(), **good) == inv              # objective 3: x_stride < K
    assert code(p4, x=TC.x4(c, o3["free"])[:, :K + 3 * 10 - 1].copy(), constraints=c["soft"]) == inv  # row 3 is K + 30
    d2 = TC.shape("col_d2")  # D != 3 with w_c > 0
    with pytest.raises(mtg.MTGError) as e:
        mtg.host_objective_time_batch(d2["N"], d2["values"], d2["mask"], TC.x3(d2), TC.params(d2, 3, w_c=10.0),
                                      coeff_times=d2["times"], grid=c["g"], collision=c["p"], constraints=d2["soft"])
    assert e.value.code == inv
    # a gradient field of parts
    lib = nat.load()
    buf, cost = np.zeros(B * K), np.zeros(B)
    pp = nat.ObjectiveParts(None, None, None, None, buf.ctypes.data, None, None, None, None)
    pn = p3n.native()
    x = TC.x3(c)
    assert lib.mtg_host_objective_time_batch(N, 3, K, B, c["values"].ctypes.data, c["mask"].ctypes.data, x.ctypes.data,
                                             x.shape[1], ctypes.byref(pn), None, None, None, None, cost.ctypes.data, None,
                                             None, None, None, None, None, None, ctypes.byref(pp), None, 1) == inv


def test_bad_times_and_warning_rows():
    c = TC.shape("masks")
    T, B = c["times"], c["B"]
    prm = TC.params(c, 3)
    _, ok = _host3(c, **ALL)
    # a time <= 0 in x (row 1) and a non-finite coeff_times entry (row 3): BAD_TIME, NaN outputs and an
    # untouched state for those rows only
    x = TC.x3(c)
    x[1, 2] = 0.0
    ct = T.copy()
    ct[3, 0] = np.inf
    state = OC.zero_state(B)
    state["cost_time"], state["n_iterations"] = 4.5, 9
    before = state.copy()
    out = mtg.host_objective_time_batch(c["N"], c["values"], c["mask"], x, prm, state=state,
                                        **TC.call_args(c, prm, ct), **ALL)
    bad = np.array([False, True, False, True, False])
    assert (out["status"][bad] & nat.MTG_TRAJ_BAD_TIME != 0).all() and (out["status"][~bad] & 255 == 0).all()
    for k in ("cost", "weighted_costs", "constraint_values", "free", "coeffs"):
        assert np.isnan(out[k][bad]).all(), k
        assert out[k][~bad].tobytes() == ok[k][~bad].tobytes(), k
    assert np.isnan(out["maxima"]["value"][bad]).all() and np.isnan(out["maxima"]["time"][bad]).all()
    assert (out["collision"][bad] == 0).all()
    assert state[bad].tobytes() == before[bad].tobytes() and (state["n_iterations"][~bad] == 10).all()
    # row 2's mask carries bit 7: the solve reports WARN_DROPPED, the warning passes through, outputs are finite
    assert out["status"][2] == nat.MTG_TRAJ_WARN_DROPPED and ok["status"][2] == nat.MTG_TRAJ_WARN_DROPPED
    assert np.isfinite(ok["cost"]).all() and np.isfinite(ok["coeffs"]).all()


def test_bounds_utility():
    c = TC.shape("masks")
    N, D, K, B = c["N"], c["D"], c["K"], c["B"]
    f = np.float64
    rel = 0.1
    x = TC.x3(c)
    lo, up, step = mtg.host_objective_time_bounds_batch(N, D, K, c["mask"], x, 3, rel)
    want = np.zeros((3,) + x.shape)
    want[0, :, :K], want[1, :, :K], want[2, :, :K] = 0.1, x[:, :K] * f(2.0), f(rel) * x[:, :K]
    assert lo.tobytes() == want[0].tobytes() and up.tobytes() == want[1].tobytes() and step.tobytes() == want[2].tobytes()
    _, o3 = _host3(c, free=True)
    x = TC.x4(c, o3["free"])
    x[:, -1] = 5.0  # padding that must come out as +0.0
    assert (x[:, K:] < 0).any(), "the shape has no negative free derivative"
    lo, up, step = mtg.host_objective_time_bounds_batch(N, D, K, c["mask"], x, 4, rel)
    want = np.zeros((3,) + x.shape)
    for b in range(B):
        n = K + D * int(c["n_free"][b])
        a = np.abs(x[b, :n])
        want[0, b, :n], want[1, b, :n], want[2, b, :n] = -a * 2, a * 2, f(rel) * a
        want[0, b, :K] = 0.1
    assert lo.tobytes() == want[0].tobytes() and up.tobytes() == want[1].tobytes() and step.tobytes() == want[2].tobytes()
    for objective in (0, 2, 5):
        with pytest.raises(mtg.MTGError) as e:
            mtg.host_objective_time_bounds_batch(N, D, K, c["mask"], x, objective, rel)
        assert e.value.code == nat.MTG_ERR_INVALID_ARGUMENT
    with pytest.raises(mtg.MTGError) as e:
        mtg.host_objective_time_bounds_batch(N, D, K, c["mask"], x[:, :K + 3].copy(), 4, rel)
    assert e.value.code == nat.MTG_ERR_INVALID_ARGUMENT


def test_cpp_objective_time_on_the_host(tmp_path):
    """tests/cpp/test_objective_time_api.cpp: objectiveTime<N> of the C++ drop-in on the host policy, on the
    `k1` shape written to a file, against the Python host call byte for byte."""
    from test_cpp_api import _cmake_build
    _cmake_build()
    exe = os.path.join(ROOT, "build", "test_objective_time_api")
    assert os.path.exists(exe)
    c = TC.shape("k1")
    _, o3 = _host3(c, free=True)
    x4 = TC.x4(c, o3["free"])
    _, o4 = _host4(c, o3["free"])
    limits = [v for _, v in c["soft"].constraints]
    derivs = [k for k, _ in c["soft"].constraints]
    inp = np.concatenate([c["values"].ravel(), c["times"].ravel(), x4.ravel(),
                          [c["soft"].weight, c["soft"].maximum_cost, c["soft"].increment], limits])
    path = str(tmp_path / "in.f64")
    inp.astype("<f8").tofile(path)
    r = subprocess.run([exe, path, str(int(c["mask"][0, 0])), str(int(c["mask"][0, 1])), str(x4.shape[1]),
                        str(derivs[0]), str(derivs[1])], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.array([float.fromhex(t) for t in r.stdout.split()])
    # objective 3 without a collision term (the C++ test has no map), then objective 4
    prm = TC.params(c, 3, w_c=0.0)
    w3 = mtg.host_objective_time_batch(c["N"], c["values"], c["mask"], TC.x3(c), prm, constraints=c["soft"])
    assert got[:2].tobytes() == np.array([w3["cost"][0], o4["cost"][0]]).tobytes()
