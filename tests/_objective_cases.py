"""Shared inputs and the numpy recombination for the tests of mtg_objective_batch
(tests/test_objective_host.py, tests/test_gpu_objective.py): the shapes, the optimiser's vector x
built from them, and the reference's weighting / raise / state rules restated in numpy scalars in the
order include/mtg.h writes them (every product and sum rounds on its own in IEEE double, as numpy
float64 scalars do)."""
import functools

import numpy as np

import mav_trajectory_generation_cmake_amd as mtg
from mav_trajectory_generation_cmake_amd import _native as nat

import _collision_model as M
import _collision_time_model as TM
import _soft_constraint_model as SM

R = {6: 2, 10: 4, 12: 4}  # derivative_to_optimize per N (N = 6: acceleration, the highest it has)
PAD = 5                   # x_stride = the longest row + PAD


def _finish(name, N, xs, masks, times, prm):
    """values = the trajectories' own vertex values; free = their free slots; x_free / x_time = the
    optimiser's vectors without / with the leading times."""
    B, V, h, D = xs.shape
    n_free = mtg.number_of_free_constraints(masks, N)
    free = np.zeros((B, D, V * h))
    for b in range(B):
        slots = [(v, k) for v in range(V) for k in range(h) if not (int(masks[b, v]) >> k) & 1]
        assert len(slots) == n_free[b]
        for d in range(D):
            free[b, d, :len(slots)] = [xs[b, v, k, d] for v, k in slots]
    K = V - 1
    stride = K + D * int(n_free.max()) + PAD
    grid = M.maps()["sphere"]
    g, p = M.to_native(grid, prm)
    # soft limits: 0.9 x the batch's median maximum of velocity and acceleration, a mild weight, so the
    # cost is neither saturated nor negligible
    mx = SM._maxima(N, xs, masks, times, (1, 2))
    soft = SM.Params([(1, 0.9 * float(np.median(mx[:, 0]))), (2, 0.9 * float(np.median(mx[:, 1])))], weight=5.0)
    rng = np.random.default_rng(len(name))
    values = xs.copy()
    fixed = ((masks[:, :, None] >> np.arange(h)[None, None, :]) & 1).astype(bool)
    values[~fixed] = rng.normal(size=values[~fixed].shape)  # a free slot's entry of `values` must not be read
    return dict(name=name, N=N, K=K, B=B, D=D, r=R[N], values=values, mask=masks, times=times, n_free=n_free, free=free,
                stride=stride, x_free=mtg.pack_optimization_variables(None, free, n_free, stride),
                x_time=mtg.pack_optimization_variables(times, free, n_free, stride), grid=grid, prm=prm, g=g, p=p,
                soft=soft, full=xs)


@functools.lru_cache(maxsize=None)
def shape(name):
    prm = M.Params(0.1, 0.2, 1.0, 0.3, 2.0, (-7.0,) * 3, (7.0,) * 3, True)
    if name == "masks":  # N = 10, K = 3, B = 5: a different mask, and a different n_free, per trajectory
        N, K, t = 10, 3, (1.37, 2.13, 1.74)
        masks = np.array([[31, 1, 1, 31],            # the generators' pattern: 8 free
                          [31, 0, 1, 31],            # a free interior position: 9
                          [31, 1 | 0x80, 3, 31],     # bit 7 set (ignored): 7
                          [7, 1, 1, 31],             # vertex 0 frees jerk and snap: the first slot of every block moves: 10
                          [31, 3, 3, 31]], np.uint8)  # 6
        xs = np.array([M.random_trajectory(N, K, 7100 + j, t)[0] for j in range(5)])
        times = np.tile(np.array(t), (5, 1)) * (1.0 + 0.01 * np.arange(5))[:, None]
        return _finish(name, N, xs, masks, times, prm)
    if name == "k1":  # N = 6, K = 1, B = 1: no interior vertex; the end vertex frees its acceleration
        N, t = 6, (2.33,)
        xs = np.array([M.random_trajectory(N, 1, 7200, t)[0]])
        return _finish(name, N, xs, np.array([[7, 3]], np.uint8), np.array([t]), prm)
    if name == "nofree":  # N = 6, K = 1, B = 2: n_free = 0 (an empty row for objectives 0 and 1) beside n_free = 1
        N, t = 6, (1.91,)
        xs = np.array([M.random_trajectory(N, 1, 7250 + j, t)[0] for j in range(2)])
        return _finish(name, N, xs, np.array([[7, 7], [7, 3]], np.uint8), np.tile(np.array(t), (2, 1)), prm)
    if name == "n12":  # N = 12, K = 8, B = 3
        N, K = 12, 8
        xs = np.array([M.random_trajectory(N, K, 7300 + j, TM.EARLY_TIMES)[0] for j in range(3)])
        masks = np.tile(M.random_trajectory(N, K, 0, TM.EARLY_TIMES)[1], (3, 1))
        return _finish(name, N, xs, masks, np.tile(np.array(TM.EARLY_TIMES), (3, 1)), prm)
    if name == "batch67":  # as test_gpu_collision_time.py's batch67: the grid tail, colliding and free trajectories
        N, K, B = 10, 8, 67
        xs = np.array([M.random_trajectory(N, K, 8200 + j, TM.EARLY_TIMES)[0] for j in range(B)])
        masks = np.tile(M.random_trajectory(N, K, 0, TM.EARLY_TIMES)[1], (B, 1))
        times = np.tile(np.array(TM.EARLY_TIMES), (B, 1)) * (1.0 + 0.003 * np.arange(B))[:, None]
        return _finish(name, N, xs, masks, times, M.Params(0.1, 1.5, 1.0, 0.3, 2.0, (-7.0,) * 3, (7.0,) * 3, True))
    raise KeyError(name)


SHAPES = ("masks", "k1", "nofree", "n12", "batch67")


def params(c, objective, soft=True, **kw):
    return mtg.ObjectiveParams(objective, c["r"], w_d=0.1, w_c=10.0, w_t=1.0, w_sc=1.0, increment_time=TM.INC,
                               use_soft_constraints=soft, **kw)


def call_args(c, objective, soft=True):
    """Keyword arguments of objective_batch / host_objective_batch for a shape and an objective."""
    kw = dict(times=None if objective == 2 else c["times"])
    if objective >= 1:
        kw.update(grid=c["g"], collision=c["p"])
    if soft:
        kw.update(soft=c["soft"].native())
    return kw


def x_of(c, objective):
    return c["x_time"] if objective == 2 else c["x_free"]


def zero_state(B):
    return np.zeros(B, dtype=mtg.OBJECTIVE_STATE_DTYPE)


def recombine(c, prm, out, state_in=None):
    """cost, grad, weighted_costs, state of include/mtg.h's "Semantics" from the parts in `out`, one
    numpy float64 scalar operation at a time.  prm: the mtg.ObjectiveParams of the call."""
    B, K, D, stride = c["B"], c["K"], c["D"], c["stride"]
    f = np.float64
    w_d, w_c, w_t, w_sc = f(prm.w_d), f(prm.w_c), f(prm.w_t), f(prm.w_sc)
    obj, with_soft = prm.objective, prm.use_soft_constraints
    state = zero_state(B) if state_in is None else state_in.copy()
    cost, weighted = np.zeros(B), np.zeros((B, 4))
    grad = np.zeros((B, stride)) if out.get("grad") is not None else None
    zero = f(0.0)
    for b in range(B):
        J_d = f(out["J_d"][b])
        J_c = f(out["J_c"][b]) if obj >= 1 else zero
        J_sc = f(out["J_sc"][b]) if with_soft else zero
        s = state[b]
        if obj == 0:
            ct, cc, ctime, cs = J_d, zero, zero, J_sc
            cost[b] = J_d + J_sc
            s["n_iterations"] += 1
            s["cost_trajectory"], s["cost_soft_constraints"] = ct, cs
        else:
            ct, cc, cs = w_d * J_d, w_c * J_c, w_sc * J_sc
            ctime = zero
            if obj == 1:
                total = (ct + cc) + cs
            else:
                T = c["times"][b]
                J_t = f(0.0)
                for i in range(K):  # the sequential sum (np.sum's order differs)
                    J_t = J_t + f(T[i])
                assert out["J_t"] is None or f(out["J_t"][b]).tobytes() == J_t.tobytes()
                ctime = w_t * J_t
                total = ((ct + cc) + ctime) + cs
                if prm.is_collision_safe and out["collision"][b]:
                    if prm.is_coll_raise_first_iter:
                        ref = f(s["total_cost_iter0"])
                    else:
                        ref = ((f(s["cost_trajectory"]) + f(s["cost_collision"])) + f(s["cost_time"])) + \
                            f(s["cost_soft_constraints"])
                    if total < ref:
                        cc = (ref - (total - cc)) + f(prm.add_coll_raise)
                total = ((ct + cc) + ctime) + cs
                s["cost_time"] = ctime
            cost[b] = total
            s["n_iterations"] += 1
            s["cost_trajectory"], s["cost_collision"], s["cost_soft_constraints"] = ct, cc, cs
            if not s["iter0_done"]:
                s["total_cost_iter0"], s["iter0_done"] = total, 1
        weighted[b] = (ct, cc, ctime, cs)
        if grad is not None:
            nf = int(c["n_free"][b])
            nt = K if obj == 2 else 0
            for i in range(nt):
                grad[b, i] = ((w_d * f(out["dJd_dt"][b, i]) + w_c * f(out["dJc_dt"][b, i])) + w_sc * zero) + w_t
            for d in range(D):
                for i in range(nf):
                    g_d = f(out["grad_d"][b, d, i])
                    if obj == 0:
                        grad[b, nt + d * nf + i] = g_d
                    else:
                        g_sc = f(out["grad_sc"][b, d, i]) if with_soft else zero
                        grad[b, nt + d * nf + i] = (w_d * g_d + w_c * f(out["grad_c"][b, d, i])) + w_sc * g_sc
    return dict(cost=cost, grad=grad, weighted_costs=weighted, state=state)


def assert_recombination(c, prm, out, state_in=None, label=""):
    want = recombine(c, prm, out, state_in)
    for k in ("cost", "grad", "weighted_costs"):
        if want[k] is None:
            assert out[k] is None
            continue
        assert np.asarray(out[k]).tobytes() == want[k].tobytes(), (label, k)
    if out.get("state") is not None:
        assert np.asarray(out["state"]).tobytes() == want["state"].tobytes(), (label, "state")
    return want
