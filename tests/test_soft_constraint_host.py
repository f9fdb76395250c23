"""Soft-constraint cost and gradient of the magnitude limits: the host path
(mtg_host_soft_constraint_cost_batch, the reference loop written literally) against the independent
FP64 model (tests/_soft_constraint_model.py) on the shared cases, the conditions the cases must meet
(asserted from the model alone), the error paths and the C++ wrapper.  No GPU."""
import numpy as np
import pytest

import mav_trajectory_generation_cmake_amd as mtg
from mav_trajectory_generation_cmake_amd import _native as nat

import _soft_constraint_model as M


def _host(name, **kw):
    N, x, mask, times, prm = M.case(name)
    return mtg.host_soft_constraint_cost_batch(N, x, times, prm.native(), mask=mask, grad=True, threads=8, **kw)


@pytest.mark.parametrize("name", M.ALL_CASES)
def test_host_matches_model(name):
    M.compare("host vs model", _host(name), name)


@pytest.mark.parametrize("name", M.GRADIENT_CASES)
def test_cases_are_not_trivial(name):
    """From the model alone: every constraint is violated, and per trajectory at least n_free / 4
    gradient entries exceed 100 x their tolerance."""
    N, x, mask, times, prm = M.case(name)
    counts = []
    for b, m in enumerate(M.model(name)):
        assert all(mx[1] > limit for mx, (_, limit) in zip(m["maxima"], prm.constraints))
        g, t = m["grad"][:, :m["n_free"]], m["grad_tol"][:, :m["n_free"]]
        big = int(np.count_nonzero(np.abs(g) > 100.0 * t))
        counts.append(big)
        assert m["n_free"] > 0 and big >= m["n_free"] / 4.0, (name, b, big, m["n_free"])
    print(name, "n_free", m["n_free"], "entries above 100 x tolerance per trajectory: min", min(counts))


def test_comparator_rejects_nan_and_errors_above_the_tolerance():
    """The gate itself: a NaN cost or gradient entry on either side, or an entry off by 1e-3, fails."""
    out = _host("k2")
    M.compare("host vs model", out, "k2")

    def changed(key, idx, value):
        o = {k: (v.copy() if v is not None else None) for k, v in out.items()}
        o[key][idx] = value
        return o

    for o in (changed("cost", (1,), np.nan), changed("grad", (2, 1, 0), np.nan),
              changed("grad", (0, 0, 0), out["grad"][0, 0, 0] * 1.001)):
        with pytest.raises(AssertionError):
            M.compare("changed vs model", o, "k2")
        with pytest.raises(AssertionError):
            M.compare("host vs changed", out, "k2", other=o)


def test_locality():
    """One segment dominates the velocity maximum: a free derivative of a vertex that is not an end
    of that segment has a gradient of exactly 0.0, in the model and on the host path; the others match
    the model (test_host_matches_model)."""
    N, x, mask, times, prm = M.case("locality")
    out = _host("locality")
    h = N // 2
    for b, m in enumerate(M.model("locality")):
        s = m["maxima"][0][2]
        slots = [(v, k) for v in range(x.shape[1]) for k in range(h) if not (int(mask[b, v]) >> k) & 1]
        far = [n for n, (v, k) in enumerate(slots) if v not in (s, s + 1)]
        near = [n for n, (v, k) in enumerate(slots) if v in (s, s + 1)]
        assert len(far) >= 24 and len(near) >= 4
        assert (m["grad"][:, far] == 0.0).all() and (out["grad"][b][:, far] == 0.0).all()
        assert (np.abs(m["grad"][:, near]) > 0).any()


def test_argmax_switches_in_the_model():
    """Case 7 is only a test of the argmax switch if some perturbation moves the maximum to another
    segment: the model counts them."""
    total = sum(m["switches"] for m in M.model("switch"))
    print("perturbed evaluations whose maximum changed segment:", total)
    assert total >= 1


def test_saturation_is_exact():
    N, x, mask, times, prm = M.case("saturated")
    out = _host("saturated")
    assert (out["cost"] == len(prm.constraints) * 1e12).all()
    assert (out["grad"] == 0.0).all()


def test_gradient_off_leaves_the_cost_bits():
    N, x, mask, times, prm = M.case("k2")
    a = mtg.host_soft_constraint_cost_batch(N, x, times, prm.native(), mask=mask, grad=True)
    b = mtg.host_soft_constraint_cost_batch(N, x, times, prm.native())
    assert b["grad"] is None
    np.testing.assert_array_equal(a["cost"], b["cost"])
    np.testing.assert_array_equal(a["maxima"], b["maxima"])


def test_zero_increment_and_bad_times():
    N, x, mask, times, prm = M.case("k2")
    p0 = M.Params(prm.constraints, prm.weight, prm.maximum_cost, 0.0)
    out = mtg.host_soft_constraint_cost_batch(N, x, times, p0.native(), mask=mask, grad=True)
    n_free = M.model("k2")[0]["n_free"]
    assert np.isfinite(out["cost"]).all() and np.isnan(out["grad"][:, :, :n_free]).all()  # 0 / 0, as the reference
    assert (out["grad"][:, :, n_free:] == 0).all()
    good = mtg.host_soft_constraint_cost_batch(N, x, times, prm.native(), mask=mask, grad=True)
    for badv in (0.0, -1.0, np.inf, np.nan):
        t2 = times.copy()
        t2[1, 1] = badv
        out = mtg.host_soft_constraint_cost_batch(N, x, t2, prm.native(), mask=mask, grad=True)
        assert list(out["status"]) == [0, nat.MTG_TRAJ_BAD_TIME, 0, 0, 0]
        assert np.isnan(out["cost"][1]) and (out["grad"][1] == 0).all()
        keep = [0, 2, 3, 4]
        np.testing.assert_array_equal(out["cost"][keep], good["cost"][keep])
        np.testing.assert_array_equal(out["grad"][keep], good["grad"][keep])


def _invalid_calls():
    N, x, mask, times, prm = M.case("k2")
    ok = prm.constraints
    yield "n_constraints = 0", N, x, times, M.Params([])
    yield "n_constraints = 9", N, x, times, M.Params([ok[0]] * 9)
    yield "derivative < 0", N, x, times, M.Params([(-1, 1.0)])
    yield "derivative > 4", N, x, times, M.Params([(5, 1.0)])
    yield "limit = 0", N, x, times, M.Params([(1, 0.0)])
    yield "limit < 0", N, x, times, M.Params([(1, -1.0)])
    yield "limit NaN", N, x, times, M.Params([(1, float("nan"))])
    yield "D = 5", 10, np.zeros((1, 2, 5, 5)), np.ones((1, 1)), prm
    yield "N = 4", 4, np.zeros((1, 2, 2, 3)), np.ones((1, 1)), prm
    yield "N = 14", 14, np.zeros((1, 2, 7, 3)), np.ones((1, 1)), prm


def invalid_calls():
    """(N - 2 >= 4 for every supported N, so min(4, N - 2) is 4: a derivative above 4 is the range error.)"""
    return _invalid_calls()


@pytest.mark.parametrize("call", list(invalid_calls()), ids=lambda c: c[0])
def test_invalid_arguments(call):
    label, N, x, times, prm = call
    with pytest.raises(mtg.MTGError) as e:
        mtg.host_soft_constraint_cost_batch(N, x, times, prm.native())
    assert e.value.code == nat.MTG_ERR_INVALID_ARGUMENT, label
