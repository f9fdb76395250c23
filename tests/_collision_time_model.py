"""Stand-in for the collision part of the reference's getCostAndGradientTime
(polynomial_optimization_nonlinear_impl.h:2155-2243), built on tests/_collision_model.py: the
coefficients come from the UNPERTURBED times (the reference's L_ is not recomputed by
updateSegmentTimes), and each (segment n, side) is one walk of M._loop over the perturbed times.

* fp64_side: the literal FP64 restatement of one walk: J, S_J (sum of |cost terms|), n_eval, the gate
  decisions and the smallest margin of every comparison, by kind.
* truth_side: the same walk at 50 digits (coefficients by a 50-digit solve with A(T) at the unperturbed
  times), with the FP64 walk's decisions forced.
* segments_walked: the early-stop rule of include/mtg.h restated -- an own, gradient-free copy of the
  loop's state recurrence gives (time_sum, dist_sum) at every segment entry; a perturbed walk stops at
  the first segment m >= n+2 whose entry state equals the unperturbed walk's bit for bit.
"""
import functools
import math
import struct

import numpy as np

import _collision_model as M

try:
    import mpmath
except ImportError:
    mpmath = None

CLAMP = 0.1  # the reference's literal


def perturbed_times(times, n, side, inc):
    """T' of (n, side), or None where the reference CHECK-fails (T[n] > 0.1 and T[n] - inc <= 0)."""
    T = [float(t) for t in times]
    if T[n] <= CLAMP:
        T[n] = CLAMP
    elif T[n] - inc <= 0.0:
        return None
    else:
        T[n] = T[n] + inc if side else T[n] - inc
    return T


def _coeff_lists(N, x, times):
    co = M.host_coefficients(N, x, times)
    return [[[float(v) for v in co[i, k]] for k in range(3)] for i in range(len(times))]


def fp64_side(N, coeffs, tp, grid, prm):
    rec = M._Margins()
    r = M._loop(M._F64, N, coeffs, tp, grid, prm, False, rec=rec)
    return {"J": r["J"], "S_J": r["S_J"], "n_eval": r["n_eval"], "decisions": tuple(r["decisions"]),
            "margins": dict(rec.by_kind)}


def mp_coefficients(N, x, times):
    """[K][3][N] at 50 digits from the vertex values and the unperturbed times (call inside workdps)."""
    h = N // 2
    out = []
    for i, T in enumerate(times):
        A = M._mp_mapping(N, mpmath.mpf(float(T)))
        rows = []
        for k in range(3):
            rhs = mpmath.matrix([mpmath.mpf(float(x[i, q, k])) for q in range(h)] +
                                [mpmath.mpf(float(x[i + 1, q, k])) for q in range(h)])
            sol = mpmath.lu_solve(A, rhs)
            rows.append([sol[j] for j in range(N)])
        out.append(rows)
    return out


def truth_side(N, mp_coeffs, tp, grid, prm, decisions):
    M._MP.nan = mpmath.nan
    r = M._loop(M._MP, N, mp_coeffs, tp, grid, prm, False, forced=decisions)
    assert tuple(r["decisions"]) == tuple(decisions)
    return r["J"]


def _bits(v):
    return struct.pack("<d", v)


def entry_states(N, coeffs, tp, prm):
    """(time_sum, dist_sum) at the entry of every segment, and the decisions, of the loop's state
    recurrence alone (positions, step lengths, the gate; no potential): plain FP64, the loop's order."""
    dt, gate = prm.dt, prm.map_resolution
    states, decisions = [], []
    prev = [0.0, 0.0, 0.0]
    time_sum, dist_sum = -1.0, 0.0
    for i, T in enumerate(tp):
        states.append((time_sum, dist_sum))
        t = 0.0
        while t < T:
            pos = []
            for k in range(3):
                c = coeffs[i][k]
                p = c[N - 1]
                for n in range(N - 2, -1, -1):
                    p = p * t + c[n]
                pos.append(p)
            if time_sum < 0:
                time_sum = 0.0
                prev = pos
                decisions.append(0)
                t += dt
                continue
            time_sum = time_sum + dt
            dx, dy, dz = pos[0] - prev[0], pos[1] - prev[1], pos[2] - prev[2]
            dist_sum = dist_sum + math.sqrt(dx * dx + dy * dy + dz * dz)
            prev = pos
            if dist_sum < gate:
                decisions.append(1)
            else:
                decisions.append(2)
                dist_sum = 0.0
                time_sum = 0.0
            t += dt
        time_sum = time_sum + (-dt + (T - t))
    return states, tuple(decisions)


def walked_segments(n, K, unperturbed_states, states):
    """Segments the walk of a perturbation of segment n does under the early-stop rule; and whether it
    rejoined (None where there is no segment n+2 to rejoin at)."""
    for m in range(n + 2, K):
        if all(_bits(a) == _bits(b) for a, b in zip(states[m], unperturbed_states[m])):
            return m - n, True
    return K - n, (False if n + 2 < K else None)


def model(N, x, times, grid, prm, inc, truth=True):
    """Everything the tests compare against, for one trajectory: per (n, side) the FP64 walk (None under
    the NaN rule) with its 50-digit cost `truth`, walked / rejoined of the early-stop rule, and the sums
    grad_t [K], segments_walked, margin (the smallest margin of a kind other than the clock, over all
    perturbed walks and the unperturbed one)."""
    x = np.asarray(x, dtype=np.float64)
    times = [float(t) for t in times]
    K = len(times)
    coeffs = _coeff_lists(N, x, times)
    base = fp64_side(N, coeffs, times, grid, prm)
    u_states, u_dec = entry_states(N, coeffs, times, prm)
    assert u_dec == base["decisions"], "the state recurrence and M._loop disagree"
    margin = min([v for k, v in base["margins"].items() if k != "clock"] + [np.inf])
    sides, grad, total = {}, [], 0
    want_truth = truth and mpmath is not None
    with (mpmath.workdps(50) if want_truth else _Null()):
        mpc = mp_coefficients(N, x, times) if want_truth else None
        for n in range(K):
            for s in (0, 1):
                tp = perturbed_times(times, n, s, inc)
                if tp is None:
                    sides[n, s] = None
                    continue
                r = fp64_side(N, coeffs, tp, grid, prm)
                states, dec = entry_states(N, coeffs, tp, prm)
                assert dec == r["decisions"], "the state recurrence and M._loop disagree"
                r["walked"], r["rejoined"] = walked_segments(n, K, u_states, states)
                r["rejoined_at"] = n + r["walked"] if r["rejoined"] else None
                total += r["walked"]
                margin = min([margin] + [v for k, v in r["margins"].items() if k != "clock"])
                if want_truth:
                    r["truth"] = truth_side(N, mpc, tp, grid, prm, r["decisions"])
                sides[n, s] = r
            a, b = sides[n, 0], sides[n, 1]
            grad.append(float("nan") if a is None or b is None else (b["J"] - a["J"]) / (2.0 * inc))
    return {"sides": sides, "grad_t": grad, "segments_walked": total, "margin": margin, "base": base}


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def check_sides(name, got, mdl, inc, model_tol=1e-6, truth_tol=1e-9):
    """The acceptance measures of one trajectory, got = dict(grad_t [K], side_cost [K][2], side_evaluated
    [K][2]): counts exact; each side cost within 1e-6 S_J of the FP64 model and within max(4 x the
    model's own error, 1e-9 S_J) of the 50-digit value (the bounds of M.check_against); grad_t within
    1e-6 (S_J(n,0) + S_J(n,1)) / (2 inc) of the model's quotient.  Prints the worst ratios, then asserts."""
    K = len(mdl["grad_t"])
    fails, worst = [], {"side_model": 0.0, "side_truth": 0.0, "grad_model": 0.0}
    for n in range(K):
        if mdl["sides"][n, 0] is None:
            if not (np.isnan(got["grad_t"][n]) and np.isnan(got["side_cost"][n]).all() and
                    (got["side_evaluated"][n] == 0).all()):
                fails.append("NaN rule at n = %d" % n)
            continue
        S = 0.0
        for s in (0, 1):
            m = mdl["sides"][n, s]
            S += m["S_J"]
            if got["side_evaluated"][n, s] != m["n_eval"]:
                fails.append("side_evaluated[%d][%d] = %d, model %d" % (n, s, got["side_evaluated"][n, s], m["n_eval"]))
            e = abs(got["side_cost"][n, s] - m["J"])
            if not e <= model_tol * m["S_J"]:
                fails.append("side cost (%d, %d) vs model: %.3e > %.3e" % (n, s, e, model_tol * m["S_J"]))
            if m["S_J"] > 0:
                worst["side_model"] = max(worst["side_model"], e / (model_tol * m["S_J"]))
            if "truth" in m:
                with mpmath.workdps(50):
                    et = float(abs(mpmath.mpf(float(got["side_cost"][n, s])) - m["truth"]))
                    em = float(abs(mpmath.mpf(float(m["J"])) - m["truth"]))
                bound = max(4.0 * em, truth_tol * m["S_J"])
                if not et <= bound:
                    fails.append("side cost (%d, %d) vs truth: %.3e > %.3e" % (n, s, et, bound))
                if bound > 0:
                    worst["side_truth"] = max(worst["side_truth"], et / bound)
        e = abs(got["grad_t"][n] - mdl["grad_t"][n])
        bound = model_tol * S / (2.0 * inc)
        if not e <= bound:
            fails.append("grad_t[%d] vs model: %.3e > %.3e" % (n, e, bound))
        if bound > 0:
            worst["grad_model"] = max(worst["grad_model"], e / bound)
    print("%s worst ratios: %s" % (name, {k: "%.3g" % v for k, v in worst.items()}))
    assert not fails, (name, fails)
    return worst


def compare_with_host(name, dev, host):
    """Device against host: counts and status exact, the NaN pattern equal, side costs within 1e-6 of the
    host's (every cost term is >= 0, so a side cost is its own S_J)."""
    assert (dev["status"] == host["status"]).all()
    assert (dev["side_evaluated"] == host["side_evaluated"]).all()
    for k in ("side_cost", "grad_t"):
        assert (np.isnan(dev[k]) == np.isnan(host[k])).all(), k
    e = np.nan_to_num(np.abs(dev["side_cost"] - host["side_cost"]))
    scale = np.nan_to_num(np.abs(host["side_cost"]))
    print("%s: max |side cost - host| / host = %.3e" % (name, np.max(e / np.maximum(scale, 1e-300))))
    assert (e <= 1e-6 * scale).all()


# ----------------------------------------------------------------------------- shared cases
INC = 0.1


@functools.lru_cache(maxsize=None)
def case_models(name):
    """The models of the four trajectories of M.build_case(name) at increment_time = 0.1 (computed once
    per session, shared by the host and device tests)."""
    c = M.build_case(name)
    return [model(c["N"], c["x"][j], c["case"]["times"], c["grid"], c["prm"], INC) for j in range(len(c["x"]))]


# Early stop (test 2): K = 8, N = 10, the sphere map, dt = 0.1; segment times with irregular hundredths
# in [1.2, 2.6], so that no T +- 0.1 lands on the clock.  The seeds were chosen on the CPU so that the
# model says what the tests assert: at map_resolution 0.2 every perturbation rejoins at n+2, at 1.5 some
# perturbation with n+2 < K never rejoins, and no margin other than the clock's is below 1e-9.
EARLY_TIMES = (1.37, 2.13, 1.74, 2.56, 1.23, 1.91, 2.38, 1.62)
EARLY_SEEDS = {0.2: (8101, 8102, 8104), 1.5: (8101, 8103, 8104)}


@functools.lru_cache(maxsize=None)
def early_case(map_resolution):
    N, K = 10, 8
    grid = M.maps()["sphere"]
    prm = M.Params(0.1, map_resolution, 1.0, 0.3, 2.0, (-7.0,) * 3, (7.0,) * 3, True)
    xs = np.array([M.random_trajectory(N, K, seed, EARLY_TIMES)[0] for seed in EARLY_SEEDS[map_resolution]])
    times = np.tile(np.array(EARLY_TIMES), (len(xs), 1))
    models = [model(N, x, EARLY_TIMES, grid, prm, INC) for x in xs]
    return dict(N=N, K=K, x=xs, times=times, grid=grid, prm=prm, models=models)


# More samples than a chunk (test 3): two segments of about 7 s at dt = 0.01
LONG_TIMES = (7.013, 6.987)


@functools.lru_cache(maxsize=None)
def long_case(inc):
    N, K = 10, 2
    grid = M.maps()["sphere"]
    prm = M.Params(0.01, 0.05, 1.0, 0.3, 2.0, (-7.0,) * 3, (7.0,) * 3, True)
    x, _ = M.random_trajectory(N, K, 5151, LONG_TIMES)
    return dict(N=N, K=K, x=x[None], times=np.array([LONG_TIMES]), grid=grid, prm=prm,
                model=model(N, x, LONG_TIMES, grid, prm, inc, truth=False))
