"""Independent FP64 model of the soft-constraint term (mtg_soft_constraint_cost_batch), in numpy, and
the test cases shared by test_soft_constraint_host.py and test_gpu_soft_constraint.py.

The model restates getCostAndGradientSoftConstraints (nl_impl:2025-2091) over
evaluateMaximumMagnitudeAsSoftConstraint (:2396-2425) and computeMaximumOfMagnitude
(lin_impl:470-503):
* coefficients c_i = A(T_i)^-1 [x_i; x_{i+1}] with the oracle's mapping matrix and its Schur inverse
  (oracle.pyoracle.setup_mapping_matrix / invert_mapping_matrix, as its coefficients_from_vertices);
* candidates per segment, in order: t = 0, then the real roots in [0, T_i] of
  sum_d conv(p_d^(k), p_d^(k+1)) (D = 1: of p^(k+1)) as the oracle's root finder selects them
  (_real_roots_in: companion-matrix eigenvalues from LAPACK, nothing in common with the product's
  256-sample bracket search); after the last segment t = T_K; a candidate replaces the best only when strictly larger;
* the gradient by the literal central difference: for every (dimension, free index, side) the vertex
  values are perturbed, ALL coefficients re-formed and ALL segments evaluated.  The evaluation of one
  segment is a pure function of (its coefficients, T_i, k); all perturbed copies of a trajectory are
  evaluated together, and segments whose re-formed coefficients are equal value for value share one
  eigenvalue problem (numpy, in one LAPACK call per segment and constraint: this is what keeps the
  model to a few seconds).

Tolerances (derived, not chosen): the project's gate on an extremum value is EPS = 1e-9 of the maximum
(test_min_max_magnitude_vs_oracle).  An unsaturated constraint's cost exp(w (max - l) / l) may then
differ by a_c = cost_c * expm1(w EPS max_c / l_c); a saturated one (the cost is maximum_cost itself)
by nothing.  Cost: sum_c a_c.  Gradient entry: (sum_c a_c(x+) + sum_c a_c(x-)) / (2 increment), from
the model's own perturbed evaluations."""
import functools
from math import factorial

import numpy as np

import mav_trajectory_generation_cmake_amd as mtg
from oracle import pyoracle as O

EPS = 1e-9
TIE = 1e-9   # maxima: segment / time are compared only where the best segment leads by this (relative)


class Params:
    def __init__(self, constraints, weight=100.0, maximum_cost=1e12, increment=0.05):
        self.constraints = [(int(k), float(v)) for k, v in constraints]
        self.weight, self.maximum_cost, self.increment = float(weight), float(maximum_cost), float(increment)

    def native(self):
        return mtg.SoftConstraintParams(self.constraints, self.weight, self.maximum_cost, self.increment)


def _segment_maxima(N, blocks, T, k, with_end):
    """Best candidate (t, value) of derivative k for each of U coefficient blocks [U][D][N] of one
    segment of time T: t = 0, the real roots in [0, T] ascending, then t = T if with_end; the first of
    equal maxima.  The roots are the eigenvalues of the companion matrix with the selection of the
    oracle's _real_roots_in (|imag| <= eps, 0 <= real <= T), all blocks in one LAPACK call; a block whose
    root polynomial has a zero leading coefficient goes through _real_roots_in itself."""
    U, D, _ = blocks.shape
    nd, ndd = N - k, N - k - 1
    ff0 = np.array([factorial(j + k) / factorial(j) for j in range(nd)])
    ff1 = np.array([factorial(j + k + 1) / factorial(j) for j in range(ndd)])
    q, q1 = blocks[:, :, k:] * ff0, blocks[:, :, k + 1:] * ff1
    if D > 1:
        f = np.zeros((U, nd + ndd - 1))
        for d in range(D):
            for a in range(nd):
                f[:, a:a + ndd] += q[:, d, a, None] * q1[:, d, :]
    else:
        f = q1[:, 0, :].copy()
    n = f.shape[1] - 1  # degree
    roots = np.full((U, max(n, 1)), np.inf)
    regular = f[:, n] != 0.0 if n >= 1 else np.zeros(U, bool)
    if n >= 1 and regular.any():
        fr = f[regular]
        comp = np.zeros((fr.shape[0], n, n))
        comp[:, np.arange(1, n), np.arange(0, n - 1)] = 1.0
        comp[:, 0, :] = -fr[:, n - 1::-1] / fr[:, n, None]
        z = np.linalg.eigvals(comp)
        ok = (np.abs(z.imag) <= np.finfo(float).eps) & (z.real >= 0.0) & (z.real <= T)
        roots[regular] = np.where(ok, z.real, np.inf)
    for u in np.flatnonzero(~regular):
        r = O._real_roots_in(f[u], 0.0, T)
        roots[u, :len(r)] = r
    roots.sort(axis=1)  # ascending, the rejected ones (inf) last
    cands = np.concatenate([np.zeros((U, 1)), roots] + ([np.full((U, 1), T)] if with_end else []), axis=1)
    valid = np.isfinite(cands)
    t = np.where(valid, cands, 0.0)
    ssq = np.zeros_like(t)
    for d in range(D):
        acc = np.zeros_like(t)
        for j in range(nd - 1, -1, -1):
            acc = acc * t + q[:, d, j, None]
        ssq += acc * acc
    v = np.where(valid, np.sqrt(ssq), -1.0)
    j = np.argmax(v, axis=1)  # the first of equal maxima
    rows = np.arange(U)
    return t[rows, j], v[rows, j]


def _evaluate_all(N, X, times, prm):
    """X [P][V][h][D]: P sets of vertex values of one trajectory.  For each, ALL coefficients are formed
    and ALL segments evaluated; a segment's evaluation is a pure function of its coefficients, and
    equal coefficient blocks (found by their exact values) are factorised once.  Returns cost [P],
    tolerance [P], best (t, value, segment) [P][C] and the segment values [P][C][K]."""
    P, V, h, D = X.shape
    K = V - 1
    Ainv = np.stack([O.invert_mapping_matrix(O.setup_mapping_matrix(N, float(T))) for T in times])
    ends = np.concatenate([X[:, :-1], X[:, 1:]], axis=2)          # [P][K][N][D]
    coeffs = np.einsum("kab,pkbd->pkda", Ainv, ends)              # [P][K][D][N]
    C = len(prm.constraints)
    seg_t, seg_v = np.zeros((P, C, K)), np.zeros((P, C, K))
    for i in range(K):
        uniq, inv = np.unique(coeffs[:, i].reshape(P, -1), axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        for c, (k, _) in enumerate(prm.constraints):
            t, v = _segment_maxima(N, uniq.reshape(-1, D, N), float(times[i]), k, i == K - 1)
            seg_t[:, c, i], seg_v[:, c, i] = t[inv], v[inv]
    best_s = np.argmax(seg_v, axis=2)  # a later segment replaces the best only when strictly larger
    pi, ci = np.arange(P)[:, None], np.arange(C)[None, :]
    best_v, best_t = seg_v[pi, ci, best_s], seg_t[pi, ci, best_s]
    limit = np.array([l for _, l in prm.constraints])[None, :]
    with np.errstate(over="ignore"):
        e = np.exp((best_v - limit) / limit * prm.weight)
    sat = ~(e < prm.maximum_cost)
    cost, tol = np.zeros(P), np.zeros(P)
    for c in range(C):  # in constraint order
        cost += np.where(sat[:, c], prm.maximum_cost, e[:, c])
        tol += np.where(sat[:, c], 0.0, e[:, c] * np.expm1(prm.weight * EPS * best_v[:, c] / limit[0, c]))
    return cost, tol, (best_t, best_v, best_s), seg_v


def model_one(N, x, mask, times, prm, grad=True):
    """dict(cost, cost_tol, maxima, clear [C] (the best segment leads every other by TIE), grad
    [D][V*h], grad_tol, n_free, switches: perturbed evaluations whose best segment of some constraint
    is not the unperturbed one)."""
    x = np.array(x, dtype=np.float64)
    V, h, D = x.shape
    slots = [(v, k) for v in range(V) for k in range(h) if not (int(mask[v]) >> k) & 1] if grad else []
    inc = prm.increment
    X = np.repeat(x[None], 1 + 2 * D * len(slots), axis=0)
    p = 1
    for d in range(D):
        for v, k in slots:
            X[p, v, k, d] = x[v, k, d] - inc   # left, then right
            X[p + 1, v, k, d] = x[v, k, d] + inc
            p += 2
    cost, tol, (bt, bv, bs), seg_v = _evaluate_all(N, X, times, prm)
    C = len(prm.constraints)
    maxima = [(float(bt[0, c]), float(bv[0, c]), int(bs[0, c])) for c in range(C)]
    clear = []
    for c, (t, v, s) in enumerate(maxima):
        clear.append(all(v - u >= TIE * v for i, u in enumerate(seg_v[0, c]) if i != s))
    out = {"cost": float(cost[0]), "cost_tol": float(tol[0]), "maxima": maxima, "clear": clear}
    if not grad:
        return out
    g, gt = np.zeros((D, V * h)), np.zeros((D, V * h))
    nf = len(slots)
    with np.errstate(invalid="ignore", divide="ignore"):
        g[:, :nf] = ((cost[2::2] - cost[1::2]) / (2.0 * inc)).reshape(D, nf)
        gt[:, :nf] = ((tol[2::2] + tol[1::2]) / (2.0 * inc)).reshape(D, nf)
    switches = int(np.count_nonzero(bs[1:] != bs[0][None, :]))
    out.update(grad=g, grad_tol=gt, n_free=nf, switches=switches)
    return out


def model_batch(N, x, mask, times, prm, grad=True):
    return [model_one(N, x[b], mask[b], times[b], prm, grad) for b in range(x.shape[0])]


# ---------------------------------------------------------------------------------------- the cases
def _solved(N, values, mask, times):
    r = min(4, N // 2 - 1)
    sol = mtg.host_solve_linear_batch(N, r, values, mask, times, free=True, status=True)
    assert (sol["status"] == 0).all()
    return mtg.full_vertex_values(values, mask, sol["free"], N)


def _maxima(N, x, mask, times, derivatives):
    probe = Params([(k, 1.0) for k in derivatives])
    return np.array([[m[1] for m in model_one(N, x[b], mask[b], times[b], probe, grad=False)["maxima"]]
                     for b in range(x.shape[0])])


def _equalised(N, x, mask, times, ka, kb):
    """One call has one set of limits, and "0.8 x the unperturbed maximum" is to hold for every
    trajectory of it: each trajectory is rescaled in space (s) and time (a), p'(t) = s p(t / a), i.e.
    x'_k = s x_k / a^k and T' = a T, so that its maxima of derivatives ka and kb become the batch's
    medians (the maximum of derivative k scales by s / a^k)."""
    mx = _maxima(N, x, mask, times, (ka, kb))
    ra, rb = np.median(mx[:, 0]) / mx[:, 0], np.median(mx[:, 1]) / mx[:, 1]
    a = (ra / rb) ** (1.0 / (kb - ka))
    s = ra * a ** ka
    h = x.shape[2]
    x2 = x * s[:, None, None, None] / a[:, None, None, None] ** np.arange(h)[None, None, :, None]
    return np.ascontiguousarray(x2), np.ascontiguousarray(times * a[:, None])


def _limits(N, x, mask, times, derivatives, factor):
    """factor x the smallest unperturbed maximum of the batch per derivative (after _equalised the
    maxima of a batch agree to rounding): every trajectory violates every limit."""
    mx = _maxima(N, x, mask, times, derivatives)
    return [(k, factor * float(mx[:, c].min())) for c, k in enumerate(derivatives)]


def _config2(B, seed0):
    values, mask, times = mtg.random_vertices_path_batch(10, 3, 10, B, seed0=seed0)
    return values, mask, times


@functools.lru_cache(maxsize=None)
def case(name):
    """(N, x [B][V][h][D], mask, times, Params) of a named case."""
    if name == "config2":       # 1: the config-2 shape, B not a multiple of anything
        N = 10
        values, mask, times = _config2(67, 11)
        x = _solved(N, values, mask, times)
        x, times = _equalised(N, x, mask, times, 1, 2)
        prm = Params(_limits(N, x, mask, times, (1, 2), 0.8), weight=10.0, increment=0.05)
    elif name == "k2":          # 2: one interior vertex; both touched segments are the first and the last
        N = 10
        values, mask, times = mtg.random_vertices_path_batch(10, 3, 2, 5, seed0=21)
        x = _solved(N, values, mask, times)
        x, times = _equalised(N, x, mask, times, 1, 2)
        prm = Params(_limits(N, x, mask, times, (1, 2), 0.8), weight=100.0, increment=0.05)
    elif name == "k1_n12":      # 3: ends fixed to order 4, order 5 free: free derivatives at vertices 0 and K only
        N = 12
        values, mask, times = mtg.random_vertices_batch(12, 2, 1, 3, [-5.0, -5.0], [5.0, 5.0], seed0=31,
                                                        max_derivative=4)
        values = values.copy()  # (rest to rest is symmetric in time: two equal maxima in the one segment)
        values[:, 0, 1, :] = [0.7, -0.4]
        values[:, 1, 2, :] = [0.3, 0.2]
        x = _solved(N, values, mask, times)
        x, times = _equalised(N, x, mask, times, 1, 2)
        prm = Params(_limits(N, x, mask, times, (1, 2), 0.8), weight=10.0, increment=0.05)
    elif name == "d1_n8":       # 4: one dimension: the roots of p^(k+1); derivatives 0, 1, 3
        N = 8
        values, mask, times = mtg.random_vertices_batch(8, 1, 3, 9, [-5.0], [5.0], seed0=41, max_derivative=3)
        x = _solved(N, values, mask, times)
        x, times = _equalised(N, x, mask, times, 1, 3)
        prm = Params(_limits(N, x, mask, times, (0, 1, 3), 0.8), weight=10.0, increment=0.05)
    elif name == "masks_n6":    # 5: an interior vertex with its velocity fixed, an end with only its position fixed
        N = 6
        values, mask, times = mtg.random_vertices_batch(6, 3, 5, 4, [-5.0] * 3, [5.0] * 3, seed0=51, max_derivative=2)
        mask = mask.copy()
        values = values.copy()
        mask[:, 2] |= 2
        values[:, 2, 1, :] = [0.5, -0.25, 0.125]
        mask[:, 5] = 1
        x = _solved(N, values, mask, times)
        x, times = _equalised(N, x, mask, times, 1, 2)
        prm = Params(_limits(N, x, mask, times, (1, 2), 0.8), weight=10.0, increment=0.05)
    elif name == "locality":    # 6: one far-out interior vertex: one segment dominates the velocity maximum
        N = 10
        values, mask, times = _config2(3, 61)
        values = values.copy()
        values[:, 5, 0, :] += [60.0, 0.0, 0.0]
        x = _solved(N, values, mask, times)
        prm = Params(_limits(N, x, mask, times, (1,), 0.8), weight=10.0, increment=0.05)
    elif name == "switch":      # 7: large steps and limits just below the maximum: the argmax changes segment
        N = 10
        values, mask, times = _config2(4, 71)
        x = _solved(N, values, mask, times)
        prm = Params(_limits(N, x, mask, times, (1, 2), 0.99), weight=10.0, increment=0.5)
    elif name == "saturated":   # 8: every term at maximum_cost, on both sides of every difference
        N = 10
        values, mask, times = _config2(3, 81)
        x = _solved(N, values, mask, times)
        prm = Params(_limits(N, x, mask, times, (1, 2), 0.5), weight=100.0, increment=0.05)
        mx = [[m[1] for m in model_one(N, x[b], mask[b], times[b], prm, grad=False)["maxima"]] for b in range(3)]
        # one set of limits for the batch: make each the half of the SMALLEST maximum (done by _limits)
        assert all(v >= 2.0 * l for row in mx for v, (_, l) in zip(row, prm.constraints))
    elif name in ("block128", "block64"):
        # long chains: the kernel's block shrinks from 256 threads to 128 (N = 10, D = 4, two constraints:
        # K = 37 .. 73) and to 64 (K = 74 .. 92) so that the trajectory still fits LDS.  A sparse mask (ten
        # free derivatives: ends, neighbours of the ends, one whole interior vertex) keeps the literal
        # host loop and the model cheap; the values are those of the solved trajectory.
        N, K = 10, 40 if name == "block128" else 80
        values, mask, times = mtg.random_vertices_path_batch(10, 4, K, 2, seed0=91)
        x = _solved(N, values, mask, times)
        mask = np.full_like(mask, 31)
        for v, free in ((0, 0b00010), (1, 0b01010), (K // 2, 0b11111), (K - 1, 0b00100), (K, 0b10000)):
            mask[:, v] = 31 & ~free
        x, times = _equalised(N, x, mask, times, 1, 2)
        prm = Params(_limits(N, x, mask, times, (1, 2), 0.8), weight=10.0, increment=0.05)
    else:
        raise KeyError(name)
    return N, x, mask, times, prm


GRADIENT_CASES = ("config2", "k2", "k1_n12", "d1_n8", "masks_n6")  # cases 1-5: the non-triviality conditions hold
ALL_CASES = GRADIENT_CASES + ("locality", "switch", "saturated", "block128", "block64")


@functools.lru_cache(maxsize=None)
def model(name):
    N, x, mask, times, prm = case(name)
    return model_batch(N, x, mask, times, prm)


def compare(label, got, name, other=None):
    """Asserts got (dict of cost / grad / maxima / status arrays) against the model of case `name` --
    or, with other (a second result), against it under the same gate -- and returns the worst
    error / tolerance ratio (printed by the caller)."""
    ms = model(name)
    N, x, mask, times, prm = case(name)
    worst, unclear, pairs = 0.0, 0, 0
    bad = []
    for b, m in enumerate(ms):
        ref_cost = m["cost"] if other is None else other["cost"][b]
        ref_grad = m["grad"] if other is None else other["grad"][b]
        assert got["status"][b] == 0
        nf = m["n_free"]
        # anything not provably inside the tolerance fails: a NaN makes every comparison below False
        assert np.isfinite(got["cost"][b]) and np.isfinite(got["grad"][b][:, :nf]).all(), (label, name, b)
        assert np.isfinite(ref_cost) and np.isfinite(ref_grad[:, :nf]).all(), (label, name, b)
        err = abs(got["cost"][b] - ref_cost)
        ge = np.abs(got["grad"][b] - ref_grad)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(ge == 0, 0.0, ge / m["grad_tol"])                    # (x / 0 = inf for x > 0)
            cost_ratio = 0.0 if err == 0 else float(np.float64(err) / np.float64(m["cost_tol"]))
        here = max(cost_ratio, float(ratio.max()))
        worst = here if not worst >= here else worst                              # (a NaN sticks)
        if not (err <= m["cost_tol"] and (ge <= m["grad_tol"]).all()):
            bad.append((b, err, m["cost_tol"], here))
        assert (got["grad"][b][:, m["n_free"]:] == 0).all()
        for c, (t, v, s) in enumerate(m["maxima"]):
            gm = got["maxima"][b, c]
            rv = v if other is None else other["maxima"][b, c]["value"]
            assert abs(gm["value"] - rv) <= EPS * v, (label, b, c, gm, (t, v, s))
            pairs += 1
            if not m["clear"][c]:
                unclear += 1
                continue
            rs, rt = (s, t) if other is None else (other["maxima"][b, c]["segment"], other["maxima"][b, c]["time"])
            assert gm["segment"] == rs, (label, b, c, gm, (t, v, s))
            # the extremum's time, with the gate of test_min_max_magnitude_vs_oracle: a root refined to a
            # few ulp against a companion-matrix eigenvalue (flat extrema: value-equivalent)
            assert abs(gm["time"] - rt) <= 1e-6 * times[b][s] or abs(gm["value"] - rv) <= 1e-12 * v, \
                (label, b, c, gm, (t, v, s))
    assert unclear <= 0.1 * pairs, (label, unclear, pairs)
    print("%s [%s]: worst error / tolerance = %.3e" % (label, name, worst))
    assert not bad, (label, name, bad[:5])
    assert worst <= 1.0
    return worst
