"""Shared inputs and the numpy recombination for the tests of mtg_objective_time_batch
(tests/test_objective_time_host.py, tests/test_gpu_objective_time.py): the shapes of _objective_cases
plus generator-made ones that reach every default solve kernel, the optimiser's vectors for objectives
3 and 4, and the reference's rules for objectiveFunctionTime / objectiveFunctionTimeAndConstraints
restated in numpy float64 scalars in the order include/mtg.h writes them."""
import functools

import numpy as np

import mav_trajectory_generation_cmake_amd as mtg
from mav_trajectory_generation_cmake_amd import _native as nat

import _collision_model as M
import _objective_cases as OC
import _soft_constraint_model as SM

TIME_PENALTY = 500.0  # the reference's default
W_C = 10.0
PAD = 3               # x_stride = the longest row + PAD

# name -> (N, D, K, B, r, seed0, max_derivative, the default solve kernel of the shape)
GENERATED = {
    "dl67": (10, 3, 10, 67, 4, 9100, 4, nat.MTG_KERNEL_DL),      # the dimension-lane kernel, with a wave tail
    "dlx13": (10, 3, 13, 3, 4, 9200, 4, nat.MTG_KERNEL_DLX),     # the long-chain kernel
    "col_d2": (8, 2, 2, 3, 3, 9300, 3, nat.MTG_KERNEL_COLUMN),   # the column kernel; D != 3: legal only with w_c = 0
    "d4": (10, 4, 3, 3, 4, 9400, 4, nat.MTG_KERNEL_COLUMN),      # D = 4 (objective 4's extra shape)
}
SHAPES = OC.SHAPES + tuple(GENERATED)


@functools.lru_cache(maxsize=None)
def shape(name):
    """dict(N, K, B, D, r, values, mask, times, n_free, soft (mtg.SoftConstraintParams; soft_model: the
    _soft_constraint_model.Params it came from), grid / prm (the models' objects) and g / p (their native
    forms), w_c: 10 where the shape can carry a collision term)."""
    if name in OC.SHAPES:
        c = dict(OC.shape(name))
        c["soft_model"], c["soft"] = c["soft"], c["soft"].native()
        c["w_c"] = W_C
        return c
    N, D, K, B, r, seed0, max_derivative, kernel = GENERATED[name]
    values, mask, times = mtg.random_vertices_path_batch(N, D, K, B, seed0=seed0, max_derivative=max_derivative)
    grid = M.maps()["sphere"]
    prm = M.Params(0.1, 0.2, 1.0, 0.3, 2.0, (-7.0,) * 3, (7.0,) * 3, True)
    g, p = M.to_native(grid, prm)
    # the generators drive v_max = a_max = 2: limits of that size keep the cost neither saturated nor negligible
    soft = SM.Params([(1, 2.0), (2, 2.0)], weight=5.0)
    return dict(name=name, N=N, K=K, B=B, D=D, r=r, values=values, mask=mask, times=times,
                n_free=mtg.number_of_free_constraints(mask, N), soft_model=soft, soft=soft.native(), grid=grid,
                prm=prm, g=g, p=p, w_c=W_C if D == 3 else 0.0, kernel=kernel)


def params(c, objective, soft=True, w_c=None):
    w = (c["w_c"] if w_c is None else w_c) if objective == 3 else 0.0
    return mtg.ObjectiveTimeParams(objective, c["r"], time_penalty=TIME_PENALTY, w_c=w, use_soft_constraints=soft)


def call_args(c, prm, coeff_times=None, soft=True):
    """Keyword arguments of objective_time_batch / host_objective_time_batch for a shape and its params;
    coeff_times defaults to the shape's times (a refreshed L_)."""
    kw = {}
    if prm.objective == 3 and prm.w_c > 0.0:
        kw.update(coeff_times=c["times"] if coeff_times is None else coeff_times, grid=c["g"], collision=c["p"])
    if soft:
        kw.update(constraints=c["soft"])
    return kw


def x3(c, times=None):
    """Objective 3's vector: the K times, then padding that must not be read."""
    T = c["times"] if times is None else times
    x = np.full((c["B"], c["K"] + PAD), -7.5)
    x[:, :c["K"]] = T
    return x


def x4(c, free, times=None):
    """Objective 4's vector: the K times, then D blocks of n_free free derivatives from free [B][D][V*h]."""
    T = c["times"] if times is None else times
    stride = c["K"] + c["D"] * int(c["n_free"].max()) + PAD
    return mtg.pack_optimization_variables(T, free, c["n_free"], stride)


def recombine(prm, out, times, state_in=None):
    """cost, weighted_costs, state of include/mtg.h's "Semantics" of mtg_objective_time_batch from the parts
    in `out` (J_d / the solve's cost as out["ct_in"], J_c, J_sc), one float64 scalar operation at a time."""
    f = np.float64
    B, K = times.shape
    state = OC.zero_state(B) if state_in is None else state_in.copy()
    cost, weighted = np.zeros(B), np.zeros((B, 4))
    zero = f(0.0)
    for b in range(B):
        J_t = f(0.0)
        for i in range(K):  # the sequential sum
            J_t = J_t + f(times[b, i])
        if out.get("J_t") is not None:
            assert f(out["J_t"][b]).tobytes() == J_t.tobytes()
        ctime = (J_t * J_t) * f(prm.time_penalty)
        cs = f(out["J_sc"][b]) if prm.use_soft_constraints else zero
        s = state[b]
        if prm.objective == 3:
            ct = f(out["ct_in"][b])
            cc = f(prm.w_c) * f(out["J_c"][b]) if prm.w_c > 0.0 else zero
            total = ((ct + cc) + ctime) + cs
            s["n_iterations"] += 1
            s["cost_trajectory"], s["cost_collision"], s["cost_time"], s["cost_soft_constraints"] = ct, cc, ctime, cs
            if not s["iter0_done"]:
                s["total_cost_iter0"], s["iter0_done"] = total, 1
        else:
            ct, cc = f(0.5) * f(out["ct_in"][b]), zero
            total = (ct + ctime) + cs
            s["n_iterations"] += 1
            s["cost_trajectory"], s["cost_time"], s["cost_soft_constraints"] = ct, ctime, cs
        cost[b] = total
        weighted[b] = (ct, cc, ctime, cs)
    return dict(cost=cost, weighted_costs=weighted, state=state)


def assert_recombination(prm, out, ct_in, times, state_in=None, label=""):
    """out: the dict of a call with parts=True; ct_in: the solve's cost (objective 3) or J_d (objective 4)."""
    want = recombine(prm, dict(ct_in=ct_in, J_c=out["J_c"], J_sc=out["J_sc"], J_t=out["J_t"]), times, state_in)
    for k in ("cost", "weighted_costs"):
        assert np.asarray(out[k]).tobytes() == want[k].tobytes(), (label, k)
    if out.get("state") is not None:
        assert np.asarray(out["state"]).tobytes() == want["state"].tobytes(), (label, "state")
    return want
