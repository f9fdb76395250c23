"""The nonlinear objective in the optimiser's variables on the host (mtg_host_objective_batch,
csrc/mtg_host_objective.cpp): its parts against the library's existing host paths byte for byte, its
outputs against the numpy recombination of include/mtg.h's "Semantics" byte for byte, the new host
derivative term against the oracle, the raise rule and state over two calls, the gradient-off branch,
the padding and error rules, pack / unpack, and the bounds utility against a literal restatement."""
import ctypes

import numpy as np
import pytest

import mav_trajectory_generation_cmake_amd as mtg
from mav_trajectory_generation_cmake_amd import _native as nat

import _objective_cases as OC
from _objective_cases import call_args, params, shape, x_of

OUT_KEYS = ("cost", "grad", "weighted_costs", "collision", "status")


def _host(c, objective, soft=True, prm=None, x=None, **kw):
    prm = prm or params(c, objective, soft)
    kw = {**dict(parts=True, threads=0), **kw}
    return mtg.host_objective_batch(c["N"], c["values"], c["mask"], x_of(c, objective) if x is None else x, prm,
                                    **call_args(c, objective, soft), **kw)


@pytest.fixture(scope="module")
def full67():
    """Objective 2 with soft constraints on the B = 67 batch, computed once."""
    c = shape("batch67")
    return c, _host(c, 2, state=OC.zero_state(c["B"]))


def test_mask_rules_of_the_first_shape():
    c = shape("masks")
    nf = list(c["n_free"])
    assert len(set(nf)) == 5 and nf == [8, 9, 7, 10, 6]
    assert not c["mask"][1, 1] & 1                      # a free interior position
    assert c["mask"][2, 1] & 0x80                       # bit 7 set, and ignored by the count above
    assert c["mask"][3, 0] != c["mask"][0, 0]           # the first free slot of every block sits at vertex 0
    assert c["stride"] > c["K"] + 3 * max(nf)
    full = mtg.full_vertex_values(c["values"], c["mask"], c["free"], c["N"])
    assert full.tobytes() == c["full"].tobytes()


def test_batch67_has_colliding_and_free_trajectories():
    c = shape("batch67")
    out = mtg.host_collision_cost_batch(c["N"], c["full"], c["times"], c["g"], c["p"], threads=0)
    assert out["collision"].any() and not out["collision"].all()


@pytest.mark.parametrize("name", ["masks", "k1", "nofree", "n12"])
@pytest.mark.parametrize("soft", [True, False])
@pytest.mark.parametrize("objective", [0, 1, 2])
def test_parts_and_recombination(name, objective, soft):
    """Items 1 and 2: the parts are the existing host calls' bytes on full_vertex_values(values, mask,
    free-from-x); cost, grad, weighted costs and state are the numpy recombination's bytes."""
    c = shape(name)
    prm = params(c, objective, soft)
    out = _host(c, objective, soft, state=OC.zero_state(c["B"]))
    assert (out["status"] == 0).all()
    _check_parts_against_host_calls(c, objective, soft, out)
    OC.assert_recombination(c, prm, out, label=(name, objective, soft))
    assert (out["state"]["n_iterations"] == 1).all()
    assert (out["state"]["iter0_done"] == (0 if objective == 0 else 1)).all()


def _check_parts_against_host_calls(c, objective, soft, out):
    N = c["N"]
    _, free = mtg.unpack_optimization_variables(x_of(c, objective), c["n_free"], c["D"], c["K"] if objective == 2 else 0,
                                                width=c["free"].shape[2])
    full = mtg.full_vertex_values(c["values"], c["mask"], free, N)
    assert full.tobytes() == c["full"].tobytes()
    if objective >= 1:
        cc = mtg.host_collision_cost_batch(N, full, c["times"], c["g"], c["p"], mask=c["mask"], grad=True, threads=0)
        assert out["J_c"].tobytes() == cc["cost"].tobytes() and out["grad_c"].tobytes() == cc["grad"].tobytes()
        assert out["collision"].tobytes() == cc["collision"].tobytes()
    else:
        assert out["J_c"] is None and out["grad_c"] is None and not out["collision"].any()
    if soft:
        sc = mtg.host_soft_constraint_cost_batch(N, full, c["times"], c["soft"].native(), mask=c["mask"], grad=True,
                                                 threads=0)
        assert out["J_sc"].tobytes() == sc["cost"].tobytes()
        if objective >= 1:
            assert out["grad_sc"].tobytes() == sc["grad"].tobytes()
        else:
            assert out["grad_sc"] is None  # the reference does not add grad_sc in objective 0
    else:
        assert out["J_sc"] is None and out["grad_sc"] is None
    if objective == 2:
        ct = mtg.host_collision_time_gradient_batch(N, full, c["times"], c["g"], c["p"], increment_time=OC.TM.INC,
                                                    threads=0)
        assert out["dJc_dt"].tobytes() == ct["grad_t"].tobytes()
    else:
        assert out["dJd_dt"] is None and out["dJc_dt"] is None


def test_batch67_parts_and_recombination(full67):
    c, out = full67
    assert (out["status"] == 0).all() and out["collision"].any() and not out["collision"].all()
    _check_parts_against_host_calls(c, 2, True, out)
    OC.assert_recombination(c, params(c, 2), out, label="batch67")


@pytest.mark.parametrize("name", ["masks", "k1", "n12"])
def test_derivative_term_against_the_oracle(name):
    """Item 3: J_d, grad_d and dJd_dt of the new host evaluation against the oracle, with the tolerances
    the GPU tests grant the device kernels against the same oracle functions: J within 1e-7 |J|
    (tests/test_gpu_parity.py:358) and the gradient within 1e-6 of its largest entry (:362) for N <= 10;
    for N = 12 and for the central difference the bounds of test_time_jacobian_reference_difference
    (:413-416): J within 1e-6 |J|, dJd_dt within 2e-6 |J| / dt + 1e-7 max |G|."""
    from oracle import pyoracle as O
    from test_gpu_parity import _oracle_cost_grad
    c = shape(name)
    N, r, K = c["N"], c["r"], c["K"]
    out = _host(c, 2, False)
    dt = OC.TM.INC
    Jr, Gr = O.cost_time_jacobian_batch(N, r, c["full"], c["times"], np.ones((1, K)), dt)
    Jo = O.cost_at_times_batch(N, r, c["full"], c["times"], np.ones((1, K)))[:, 0]
    jtol = 1e-6 if N == 12 else 1e-7
    print("J_d rel err", np.max(np.abs(out["J_d"] - Jo) / np.abs(Jo)))
    assert (np.abs(out["J_d"] - Jo) <= jtol * np.abs(Jo)).all()
    assert (np.abs(out["J_d"] - Jr[:, 0]) <= 1e-6 * np.abs(Jr[:, 0])).all()
    tol = 2e-6 * np.abs(Jr)[..., None] / dt + 1e-7 * np.max(np.abs(Gr), axis=2, keepdims=True)
    print("dJd_dt err / tol", np.max(np.abs(out["dJd_dt"] - Gr[:, 0]) / tol[:, 0]))
    assert (np.abs(out["dJd_dt"] - Gr[:, 0]) <= tol[:, 0]).all()
    for b in range(c["B"]):
        Jb, gb = _oracle_cost_grad(N, r, c["full"][b], c["mask"][b] & ((1 << (N // 2)) - 1), c["times"][b])
        nf = gb.shape[1]
        assert nf == c["n_free"][b] and abs(out["J_d"][b] - Jb) <= jtol * abs(Jb)
        assert np.max(np.abs(out["grad_d"][b, :, :nf] - gb)) <= 1e-6 * np.max(np.abs(gb)), b
        assert (out["grad_d"][b, :, nf:] == 0).all()


def test_time_floor_and_nan_rule_of_the_derivative_term():
    """T <= 0.1: dJd_dt is exactly 0; 0.1 < T <= increment_time: NaN for that segment only."""
    c = shape("masks")
    x = c["x_time"].copy()
    x[0, 1] = 0.08
    x[1, 2] = 0.1
    out = _host(c, 2, False, x=x)
    assert out["dJd_dt"][0, 1] == 0.0 and out["dJd_dt"][1, 2] == 0.0 and np.count_nonzero(out["dJd_dt"] == 0.0) == 2
    prm = params(c, 2, False)
    prm.increment_time = 0.25
    x[2, 0] = 0.2
    out = _host(c, 2, False, x=x, prm=prm)
    assert np.isnan(out["dJd_dt"][2, 0]) and np.isnan(out["dJc_dt"][2, 0]) and np.isnan(out["grad"][2, 0])
    assert np.isfinite(out["dJd_dt"][2, 1:]).all() and out["status"][2] == 0 and np.isfinite(out["cost"][2])


def raise_rule_checks(call, c):
    """Item 4, shared with the device test: two consecutive calls on one state array, for the
    first-iteration raise, the last-iteration raise and is_collision_safe = 0; expected values from the
    numpy recombination of the parts.  call(prm, state, x) -> out (state updated in place or returned)."""
    B = c["B"]
    x0 = c["x_time"]
    seen = {"raised": 0, "not_raised_free": 0}
    for first, safe in ((True, True), (False, True), (True, False)):
        prm = params(c, 2, True, is_collision_safe=safe, is_coll_raise_first_iter=first, add_coll_raise=3.5)
        state = OC.zero_state(B)
        a = call(prm, state, x0)
        s_a = np.array(a["state"]).copy()
        want_a = OC.assert_recombination(c, prm, a, label=("first call", first, safe))
        assert (s_a["iter0_done"] == 1).all() and s_a["total_cost_iter0"].tobytes() == a["cost"].tobytes()
        assert (a["weighted_costs"][:, 1] == 10.0 * a["J_c"]).all()  # nothing to raise against a zero state
        # the second iterate is cheaper: the same x under a smaller time weight, so every total drops
        # below the first call's
        prm2 = params(c, 2, True, is_collision_safe=safe, is_coll_raise_first_iter=first, add_coll_raise=3.5)
        prm2.w_t = 0.25
        b = call(prm2, s_a.copy(), x0)
        want_b = OC.assert_recombination(c, prm2, b, state_in=s_a, label=("second call", first, safe))
        s_b = np.array(b["state"])
        assert (s_b["n_iterations"] == 2).all()
        assert s_b["total_cost_iter0"].tobytes() == s_a["total_cost_iter0"].tobytes()  # frozen by iter0_done
        unraised = (b["weighted_costs"][:, 1] == 10.0 * b["J_c"])
        coll = b["collision"].astype(bool)
        if safe:
            assert (~unraised[coll]).any(), "no colliding trajectory was raised: the inputs do not test the rule"
            seen["raised"] += int((~unraised).sum())
            # a raised cost is the reference cost plus add_coll_raise, up to the rounding of the three sums
            ref = s_a["total_cost_iter0"] if first else want_a["cost"]
            r = ~unraised
            assert np.allclose(b["cost"][r], ref[r] + 3.5, rtol=1e-12)
        else:
            assert unraised.all()
        assert unraised[~coll].all()  # a non-colliding trajectory is never raised
        seen["not_raised_free"] += int((~coll).sum())
        del want_b
    assert seen["raised"] > 0 and seen["not_raised_free"] > 0


def test_raise_rule_and_state_over_two_calls():
    c = shape("batch67")

    def call(prm, state, x):
        return _host(c, 2, True, prm=prm, x=x, state=state)

    raise_rule_checks(call, c)


def test_null_state_gives_the_bits_of_a_zero_state(full67):
    c, out = full67
    bare = _host(c, 2, state=None)
    for k in OUT_KEYS:
        assert bare[k].tobytes() == out[k].tobytes(), k
    assert bare["state"] is None


@pytest.mark.parametrize("objective", [0, 1, 2])
def test_gradient_off_leaves_the_other_bytes(objective):
    """Item 5."""
    c = shape("masks")
    a = _host(c, objective, state=OC.zero_state(c["B"]))
    b = _host(c, objective, state=OC.zero_state(c["B"]), grad=False)
    assert b["grad"] is None
    for k in ("cost", "weighted_costs", "collision", "status", "state", "J_d", "J_sc"):
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    for k in ("grad_d", "grad_c", "grad_sc", "dJd_dt", "dJc_dt"):
        assert b[k] is None, k
    # the library writes nothing through gradient part pointers when grad_out is NULL
    sentinel = np.full((c["B"], c["D"], (c["K"] + 1) * (c["N"] // 2)), 7.25)
    pp = nat.ObjectiveParts(None, None, None, None, None, None, sentinel.ctypes.data, sentinel.ctypes.data,
                            sentinel.ctypes.data)
    cost = np.zeros(c["B"])
    g, keep = c["g"].native()
    x = np.ascontiguousarray(x_of(c, objective))
    rc = nat.load().mtg_host_objective_batch(
        c["N"], c["D"], c["K"], c["B"], c["values"].ctypes.data, c["mask"].ctypes.data,
        None if objective == 2 else c["times"].ctypes.data, x.ctypes.data, c["stride"],
        ctypes.byref(params(c, objective).native()), ctypes.byref(g) if objective else None,
        ctypes.byref(c["p"].native()) if objective else None, ctypes.byref(c["soft"].native().native()), cost.ctypes.data,
        None, None, None, None, ctypes.byref(pp), None, 1)
    assert rc == 0 and (sentinel == 7.25).all() and cost.tobytes() == a["cost"].tobytes()


@pytest.mark.parametrize("objective", [0, 2])
def test_padding(objective):
    """Item 6: grad_out beyond each row is +0.0; x beyond each row is not read."""
    c = shape("masks")
    a = _host(c, objective)
    nt = c["K"] if objective == 2 else 0
    x = x_of(c, objective).copy()
    for b in range(c["B"]):
        n = nt + c["D"] * int(c["n_free"][b])
        pad = a["grad"][b, n:]
        assert len(pad) >= OC.PAD and (pad == 0.0).all() and not np.signbit(pad).any()
        assert np.isfinite(a["grad"][b, :n]).all() and np.abs(a["grad"][b, :n]).max() > 0
        x[b, n:] = np.nan
    b2 = _host(c, objective, x=x)
    for k in OUT_KEYS:
        assert a[k].tobytes() == b2[k].tobytes(), k


def error_rule_checks(call, c):
    """Item 7, shared with the device test: a time <= 0 in x."""
    good = call(c["x_time"], OC.zero_state(c["B"]))
    for badv in (0.0, -1.0, np.nan):
        x = c["x_time"].copy()
        x[1, 2] = badv
        state = OC.zero_state(c["B"])
        state["cost_time"] = 4.5
        before = state.copy()
        out = call(x, state)
        st = np.array(out["state"])
        assert list(out["status"]) == [0, nat.MTG_TRAJ_BAD_TIME, 0, 0, 0]
        n = c["K"] + c["D"] * int(c["n_free"][1])
        assert np.isnan(out["cost"][1]) and np.isnan(out["weighted_costs"][1]).all() and np.isnan(out["grad"][1, :n]).all()
        assert (out["grad"][1, n:] == 0.0).all() and not np.signbit(out["grad"][1, n:]).any()
        assert out["collision"][1] == 0 and st[1].tobytes() == before[1].tobytes()
        keep = [0, 2, 3, 4]
        for k in ("cost", "grad", "weighted_costs", "collision"):
            assert out[k][keep].tobytes() == good[k][keep].tobytes(), k
        assert (st["n_iterations"][keep] == 1).all()


def test_bad_time_in_x():
    c = shape("masks")
    error_rule_checks(lambda x, state: _host(c, 2, x=x, state=state), c)


def invalid_calls(c):
    """(label, objective, keyword overrides) of calls that must give MTG_ERR_INVALID_ARGUMENT."""
    p2 = params(c, 2)
    yield "use_numeric_grad", 2, dict(prm=params(c, 2, reserved=nat.MTG_OBJECTIVE_USE_NUMERIC_GRAD))
    yield "is_simple_numgrad_time", 2, dict(prm=params(c, 2, reserved=nat.MTG_OBJECTIVE_SIMPLE_NUMGRAD_TIME))
    yield "is_simple_numgrad_constraints", 2, dict(prm=params(c, 2, reserved=nat.MTG_OBJECTIVE_SIMPLE_NUMGRAD_CONSTRAINTS))
    for label, obj in (("objectiveFunctionTime", nat.MTG_OBJECTIVE_TIME),
                       ("objectiveFunctionTimeAndConstraints", nat.MTG_OBJECTIVE_TIME_AND_CONSTRAINTS)):
        q = params(c, 2)
        q.objective = obj
        yield label, 2, dict(prm=q)
    yield "short x_stride", 2, dict(x=np.ascontiguousarray(c["x_time"][:, :c["K"] + 3 * 10 - 1]))
    yield "NULL collision params", 2, dict(collision=None)
    yield "NULL grid", 1, dict(grid=None)
    yield "NULL soft params", 0, dict(soft=None)
    yield "soft params without use_soft_constraints", 0, dict(prm=params(c, 0, False))
    del p2


def run_invalid(call, c, label, objective, over):
    over = dict(over)
    prm = over.pop("prm", None) or params(c, objective)
    x = over.pop("x", x_of(c, objective))
    kw = {**call_args(c, objective), **over}
    with pytest.raises(mtg.MTGError) as e:
        call(c["N"], c["values"], c["mask"], x, prm, **kw)
    assert e.value.code == nat.MTG_ERR_INVALID_ARGUMENT, label


@pytest.mark.parametrize("which", range(10))
def test_invalid_arguments(which):
    c = shape("masks")
    label, objective, over = list(invalid_calls(c))[which]
    run_invalid(mtg.host_objective_batch, c, label, objective, over)


def test_collision_objective_needs_three_dimensions():
    c = shape("masks")
    v2 = np.ascontiguousarray(c["values"][..., :2])
    x = np.zeros((c["B"], c["K"] + 2 * 10))
    x[:, :c["K"]] = c["times"]
    for objective in (1, 2):
        with pytest.raises(mtg.MTGError) as e:
            mtg.host_objective_batch(c["N"], v2, c["mask"], x, params(c, objective), **call_args(c, objective))
        assert e.value.code == nat.MTG_ERR_INVALID_ARGUMENT
    # objective 0 takes D = 2
    out = mtg.host_objective_batch(c["N"], v2, c["mask"], x[:, c["K"]:], params(c, 0, False), times=c["times"])
    assert (out["status"] == 0).all() and np.isfinite(out["cost"]).all()
    with pytest.raises(mtg.MTGError) as e:
        mtg.host_objective_batch(c["N"], np.zeros(c["values"].shape[:3] + (5,)), c["mask"], np.zeros((c["B"], 60)),
                                 params(c, 0, False), times=c["times"])
    assert e.value.code == nat.MTG_ERR_INVALID_ARGUMENT


def test_pack_unpack_round_trip():
    """Item 8."""
    c = shape("masks")
    for times in (None, c["times"]):
        x = mtg.pack_optimization_variables(times, c["free"], c["n_free"], c["stride"])
        nt = 0 if times is None else c["K"]
        t2, f2 = mtg.unpack_optimization_variables(x, c["n_free"], c["D"], nt, width=c["free"].shape[2])
        assert f2.tobytes() == c["free"].tobytes() and (t2 is None if times is None else t2.tobytes() == times.tobytes())
        assert mtg.pack_optimization_variables(t2, f2, c["n_free"], c["stride"]).tobytes() == x.tobytes()
        tight = mtg.pack_optimization_variables(times, c["free"], c["n_free"])
        assert tight.shape[1] == nt + c["D"] * int(c["n_free"].max())
        for b in range(c["B"]):  # row b: times, then D blocks of n_free[b]
            nf = int(c["n_free"][b])
            assert (x[b, nt:nt + 3 * nf].reshape(3, nf) == c["free"][b, :, :nf]).all() and (x[b, nt + 3 * nf:] == 0).all()
    assert list(mtg.number_of_free_constraints(c["mask"], c["N"])) == [8, 9, 7, 10, 6]


def _bounds_restated(n_free, D, K, r, with_pos, constraints, lo_b, hi_b, x, nt, rel):
    """setFreeEndpointDerivativeHardConstraints (nl_impl:2518-2564) and nl_impl:646-692 in Python, the index
    arithmetic as written (unsigned int wraps); IndexError where .at() throws."""
    lower, upper = [-np.inf] * (D * n_free), [np.inf] * (D * n_free)

    def at(seq, i):
        if not 0 <= i < len(seq):
            raise IndexError(i)
        return i
    for k in range(D):
        for n in range(K - 1):
            if with_pos:
                start = (k * n_free + n * r) & 0xFFFFFFFF
            else:
                start = (k * n_free + n * (r + 1)) & 0xFFFFFFFF
                lower[at(lower, start)] = lo_b[k]
                upper[at(upper, start)] = hi_b[k]
            for der, val in constraints:
                idx = (start + ((der - 1) if with_pos else der)) & 0xFFFFFFFF
                lower[at(lower, idx)] = -abs(val)
                upper[at(upper, idx)] = abs(val)
    row = len(lower) + nt
    return (np.array([0.1] * nt + lower), np.array([np.inf] * nt + upper), rel * np.abs(x[:row]))


@pytest.mark.parametrize("with_pos", [True, False])
def test_bounds_against_the_restatement(with_pos):
    """Item 9, on the generators' pattern: with the position constraint the interior vertices free
    derivatives 1..4 (n r slots per vertex); without it also the position (r + 1)."""
    N, D, K, B, r = 10, 3, 6, 4, 4
    _, mask, times = mtg.random_vertices_path_batch(N, D, K, B, seed0=5)
    mask = mask.copy()
    if not with_pos:
        mask[:, 1:-1] = 0
    n_free = mtg.number_of_free_constraints(mask, N)
    assert (n_free == (K - 1) * (r if with_pos else r + 1)).all()
    rng = np.random.default_rng(3)
    free = rng.normal(size=(B, D, (K + 1) * 5))
    cons = mtg.SoftConstraintParams([(1, 2.5), (2, -4.0)])
    lo_b, hi_b = (-7.0, -6.0, 0.5), (7.0, 6.0, 3.5)
    for nt, t in ((K, times), (0, None)):
        x = mtg.pack_optimization_variables(t, free, n_free, nt + D * int(n_free.max()) + 2)
        lo, up, step = mtg.host_objective_bounds_batch(N, D, K, mask, x, r, bool(nt), with_pos, cons, lo_b, hi_b, 0.1)
        for b in range(B):
            wl, wu, ws = _bounds_restated(int(n_free[b]), D, K, r, with_pos, cons.constraints, lo_b, hi_b, x[b], nt, 0.1)
            n = len(wl)
            assert lo[b, :n].tobytes() == wl.tobytes() and up[b, :n].tobytes() == wu.tobytes()
            assert step[b, :n].tobytes() == ws.tobytes()
            for a in (lo, up, step):
                assert (a[b, n:] == 0.0).all()
        assert np.isinf(lo).any() and (lo == -2.5).any() and (up == 4.0).any() and (with_pos or (lo == 0.5).any())


def test_bounds_index_past_the_end_is_an_error():
    """A mask on which the reference's index runs past the end: the interior vertices also fix their
    velocity, so n_free < (K - 1) r and .at() throws for the last vertices; and derivative 0 with the
    position constraint, whose unsigned index wraps."""
    N, D, K, r = 10, 3, 6, 4
    _, mask, times = mtg.random_vertices_path_batch(N, D, K, 1, seed0=5)
    x = np.ones((1, 200))
    with pytest.raises(IndexError):
        _bounds_restated(15, D, K, r, True, [(1, 2.0)], None, None, x[0], 0, 0.1)
    m2 = mask.copy()
    m2[:, 1:-1] |= 2
    assert mtg.number_of_free_constraints(m2, N)[0] == 15
    cons = mtg.SoftConstraintParams([(1, 2.0)])
    with pytest.raises(mtg.MTGError) as e:
        mtg.host_objective_bounds_batch(N, D, K, m2, x, r, False, True, cons)
    assert e.value.code == nat.MTG_ERR_INVALID_ARGUMENT
    with pytest.raises(IndexError):
        _bounds_restated(20, D, K, r, True, [(0, 2.0)], None, None, x[0], 0, 0.1)
    with pytest.raises(mtg.MTGError) as e:
        mtg.host_objective_bounds_batch(N, D, K, mask, x, r, False, True, mtg.SoftConstraintParams([(0, 2.0)]))
    assert e.value.code == nat.MTG_ERR_INVALID_ARGUMENT
    lo, up, step = mtg.host_objective_bounds_batch(N, D, K, mask, x, r, False, True, mtg.SoftConstraintParams([(1, 2.0)]))
    assert (lo == -2.0).sum() == D * (K - 1)
