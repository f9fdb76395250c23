"""CPU tests: pin the oracle (C restatement of the reference path) before trusting it.

Pins, in order of strength:
  * the reference's known-answer test 2_vertices_setup (test/test_polynomial_optimization.cpp:700-744)
  * its A-matrix inversion test (:194-204), here against the exact rational inverse
  * the C++ standard's std::mt19937 known answer, and bit-equality of the restated
    generators with the real libstdc++ ones (compiled into libmav_trajectory_generation.so's host utilities)
  * 60-digit mpmath truth fixtures (tests/golden/, make_golden.py)
  * the reference's invariant tests: checkPath (:73-131), checkCost (:133-152),
    ConstraintPacking (:777-836), vertex generation (:154-192), 2_vertices_rand (:747-774)
"""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

from _util import check_path, golden_cases, load_golden, masked_elementwise_rel, poly_eval, scale_normalised_error, to_abi
from oracle import pyoracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SNAP, JERK, ACC = 4, 3, 2


def test_mt19937_known_answer():
    g = O.MT19937(5489)
    for _ in range(9999):
        g.next()
    assert g.next() == 4123659995  # [rand.predef]: 10000th invocation of a default-constructed mt19937


@pytest.mark.parametrize("D,seed", [(1, 0), (3, 12345), (3, 7), (4, 99)])
def test_generators_bit_exact_with_libstdcxx(D, seed):
    import mav_trajectory_generation_cmake_amd as mtg
    K, N = 12, 10
    v, m, t = mtg.random_vertices_path_batch(N, D, K, 3, seed0=seed)
    for b in range(3):
        ov, om = O.create_random_vertices_path(D, K, 5.0, SNAP, seed + b, nd=5)
        ot = O.estimate_segment_times(ov, 2.0, 2.0, 6.5)
        assert np.array_equal(v[b], ov) and np.array_equal(m[b], om) and np.array_equal(t[b], ot)
    lo, hi = -10 * np.ones(D), 20 * np.ones(D)
    v, m, t = mtg.random_vertices_batch(N, D, K, 3, lo, hi, seed0=seed)
    for b in range(3):
        ov, om = O.create_random_vertices(SNAP, K, lo, hi, seed + b, nd=5)
        ot = O.estimate_segment_times(ov, 3.0, 5.0)
        assert np.array_equal(v[b], ov) and np.array_equal(m[b], om) and np.array_equal(t[b], ot)


def test_vertex_generation_1d_3d():
    """PathPlanning_TestVertexGeneration1D/3D (:154-192)."""
    v, m = O.create_random_vertices(SNAP, 100, [-50.0], [50.0], 0, nd=5)
    assert bin(int(m[0])).count("1") == 5 and bin(int(m[-1])).count("1") == 5
    assert np.all(m & 1) and np.all(v[:, 0, 0] <= 50) and np.all(v[:, 0, 0] >= -50)
    lo, hi = np.array([-10.0, -20.0, -10.0]), np.array([10.0, 20.0, 10.0])
    v, m = O.create_random_vertices(SNAP, 100, lo, hi, 12345, nd=5)
    assert bin(int(m[0])).count("1") == 5 and bin(int(m[-1])).count("1") == 5
    assert np.all(v[:, 0, :] <= hi) and np.all(v[:, 0, :] >= lo)


def _exact_inverse(N, T):
    sys.path.insert(0, os.path.join(ROOT, "mav_trajectory_generation_cmake_amd", "csrc"))
    import gen_tables
    return gen_tables.inverse(gen_tables.mapping_matrix(N, Fraction(T)))


def test_a_matrix_inversion():
    """PathPlanning_A_matrix_inversion (:194-204): Schur inverse of A(T) vs a full LU inverse
    (Eigen's A.inverse() there, numpy's LAPACK LU here), T = 1..60, 1e-10 abs; plus the exact
    rational inverse, relative to the largest entry."""
    for T in range(1, 61):
        A = O.setup_mapping_matrix(10, float(T))
        Ai = O.invert_mapping_matrix(A)
        assert np.max(np.abs(Ai - np.linalg.inv(A))) < 1e-10, T
        exact = np.array([[float(x) for x in row] for row in _exact_inverse(10, T)])
        assert np.max(np.abs(Ai - exact)) < 1e-11 * np.max(np.abs(exact)), T


def test_base_coeffs_with_time_eps_rule():
    """baseCoeffsWithTime (polynomial.h:215-233): |t| < eps sets only the j = derivative entry."""
    assert np.array_equal(O.base_coeffs_with_time(10, 2, 1e-17), np.eye(10)[2] * 2.0)
    c = O.base_coeffs_with_time(10, 2, 2.0)
    assert c[2] == 2.0 and c[3] == 6.0 * 2.0 and c[9] == 72.0 * 2.0 ** 7


def test_kat_2_vertices_setup():
    g = load_golden("kat_2_vertices_setup")
    r = O.solve_linear(10, 4, g["values"][0], g["mask"][0], g["times"][0])
    matlab = np.array([-0.000000000000004, 0.000000000000004, -0.000000000000006, 0.000000000000003,
                       -0.000000000000001, 0.201600000000015, -0.134400000000012, 0.034560000000004,
                       -0.004032000000000, 0.000179200000000])
    assert r["n_free"] == 0
    assert np.max(np.abs(r["coeffs"][0, 0] - matlab)) < 1e-13
    assert np.max(np.abs(r["coeffs"][0, 0] - g["coeffs"][0, 0, 0])) < 1e-13


@pytest.mark.parametrize("case", golden_cases())
def test_oracle_vs_truth(case):
    g = load_golden(case)
    N, r = int(g["N"]), int(g["r"])
    tol = 1e-4 if N == 12 and g["times"].shape[1] >= 20 else 1e-6  # reference FP64 path error, SURVEY App. A
    for b in range(len(g["times"])):
        res = O.solve_linear(N, r, g["values"][b], g["mask"][b], g["times"][b])
        assert res["rc"] >= 0
        assert res["n_free"] == g["n_free"][b] and res["n_fixed"] == g["n_fixed"][b]
        np.testing.assert_array_equal(res["fixed"], g["fixed"][b][:, :res["n_fixed"]])
        err = scale_normalised_error(res["coeffs"][None], g["coeffs"][b][None], g["times"][b][None])
        assert err <= tol, (case, b, err)
        assert abs(res["cost"] - g["cost"][b]) <= 1e-5 * abs(g["cost"][b]) + 1e-12


def test_truth_banded_matches_dense_truth():
    """make_golden.truth_solve_banded (the 60-digit reference system solved by banded LDL^T, the long-K
    arbiter of tests/test_gpu_dlx.py) reproduces the committed dense-LU truth fixtures: the first two
    trajectories of every fixture (K up to 50, N = 6..12, every mask kind), exactly after rounding."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_golden import truth_solve_banded
    for case in golden_cases():
        g = load_golden(case)
        N, r = int(g["N"]), int(g["r"])
        for b in range(min(2, len(g["times"]))):
            vals, mask = to_abi(g["values"][b:b + 1], g["mask"][b:b + 1], N)
            c = truth_solve_banded(N, r, vals[0], mask[0], g["times"][b])
            err = scale_normalised_error(c[None], g["coeffs"][b][None], g["times"][b][None])
            assert err <= 1e-15, (case, b, err)


def test_truth_banded_full_matches_dense_truth():
    """truth_solve_banded(full=True) -- the coefficients, the free derivatives in the reference's (vertex,
    derivative) order and the cost, which tests/_solve_truth_cases.py holds every solve kernel to -- equals
    the dense-LU truth_solve on small shapes of that grid (every mask kind, n_free = 0 among them),
    exactly after rounding; the cost's parts per dimension sum to it; and a system passed in (shared with
    fp64_best_solve) changes nothing."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_golden import _system, fp64_best_solve, truth_solve, truth_solve_banded
    import _solve_truth_cases as C
    for N, r, K, kind in [(2, 0, 3, "mixed"), (4, 1, 4, "ends"), (6, 0, 3, "mixed"), (8, 2, 5, "mixed"),
                          (10, 4, 1, "pattern"), (10, 3, 4, "ends"), (12, 5, 3, "mixed"), (12, 0, 4, "pattern")]:
        vals, mask, times = C.problems(N, r, K, kind)
        for p in range(C.PROBLEMS):
            c, cost, free, _ = truth_solve(N, r, vals[p], mask[p], times[p])
            bc, bfree, bcost, bcost_d = truth_solve_banded(N, r, vals[p], mask[p], times[p], full=True)
            assert scale_normalised_error(bc[None], c[None], times[p][None]) <= 1e-15
            assert bfree.shape == free.shape == (vals.shape[-1], C.n_free_of(N, mask[p]))
            np.testing.assert_allclose(bfree, free, rtol=1e-15, atol=0)
            assert abs(bcost - cost) <= 1e-15 * cost and abs(bcost_d.sum() - cost) <= 1e-14 * cost
            np.testing.assert_array_equal(truth_solve_banded(N, r, vals[p], mask[p], times[p]), bc)
            system = _system(N, r, vals[p], mask[p], times[p])
            sc = truth_solve_banded(N, r, vals[p], mask[p], times[p], full=True, system=system)
            np.testing.assert_array_equal(sc[0], bc)
            np.testing.assert_array_equal(sc[1], bfree)
            np.testing.assert_array_equal(fp64_best_solve(N, r, vals[p], mask[p], times[p], system=system),
                                          fp64_best_solve(N, r, vals[p], mask[p], times[p]))


def _setup(N, r, vals, mask, times):
    res = O.solve_linear(N, r, vals, mask, times, want_matrices=True)
    K = len(times)
    n = res["n_fixed"] + res["n_free"]
    M = np.zeros((len(res["col_of_row"]), n))
    M[np.arange(len(res["col_of_row"])), res["col_of_row"]] = 1.0
    Ainv = np.zeros((N * K, N * K))
    A = np.zeros((N * K, N * K))
    for i in range(K):
        Ainv[i * N:(i + 1) * N, i * N:(i + 1) * N] = res["ainv"][i]
        A[i * N:(i + 1) * N, i * N:(i + 1) * N] = res["amap"][i]
    # getMpinv (lin_impl:562-571): M^T with every row divided by its sum
    Mp = M.T / M.T.sum(axis=1, keepdims=True)
    return res, M, Ainv, A, Mp


def test_constraint_packing():
    """ConstraintPacking (:777-836): [d_f;d_p] -> p -> A p -> M_pinv -> [d_f;d_p], per-segment p."""
    for seed in range(12345, 12345 + 100):
        v, m = O.create_random_vertices(JERK, 5, [-50.0] * 3, [50.0] * 3, seed, nd=5)
        t = O.estimate_segment_times(v, 3.0, 5.0)
        res, M, Ainv, A, Mp = _setup(10, 4, v, m, t)
        for d in range(3):
            d_all = np.concatenate([res["fixed"][d], res["free"][d]])
            p = Ainv @ M @ d_all
            d_re = Mp @ (A @ p)
            assert np.max(np.abs(d_all - d_re)) < 1e-6
            for j in range(5):
                assert np.max(np.abs(res["coeffs"][j, d] - p[j * 10:(j + 1) * 10])) < 1e-6


def _max_magnitude(coeffs, times, derivative, dt=0.01):
    """getMaximumMagnitude (:48-59): sampled max norm over all segments."""
    best = -1e9
    for i in range(len(times)):
        ts = np.arange(0, times[i], dt)
        vals = np.stack([poly_eval(coeffs[i, d], ts, derivative) for d in range(coeffs.shape[1])], -1)
        best = max(best, float(np.max(np.linalg.norm(vals, axis=-1))))
    return best


def _cost_numeric(coeffs, times, derivative, dt=0.001):
    """computeCostNumeric (:61-71): Riemann sum of |p^(r)|^2."""
    c = 0.0
    for i in range(len(times)):
        ts = np.arange(0, times[i], dt)
        vals = np.stack([poly_eval(coeffs[i, d], ts, derivative) for d in range(coeffs.shape[1])], -1)
        c += float(np.sum(np.sum(vals ** 2, axis=-1) * dt))
    return c


@pytest.mark.parametrize("name,K,lo,hi,seed,D,vfac,afac", [
    ("1D_10", 10, -10, 10, 12, 1, 2.0, 2.0),          # :206-243
    ("1D_50", 50, -10, 10, 123, 1, 2.0, 1.0),         # :245-279
    ("1D_100", 100, -10, 10, 1234, 1, 5.0, 2.0),      # :281-315
    ("1D_100_high", 100, -50, 50, 12345, 1, 5.0, 2.0),  # :317-353
    ("3D_100_high", 100, None, None, 12345, 3, 5.0, 2.0),  # :355-394
])
def test_path_planning_unconstrained(name, K, lo, hi, seed, D, vfac, afac):
    if D == 1:
        v, m = O.create_random_vertices(SNAP, K, [lo], [hi], seed, nd=5)
    else:
        v, m = O.create_random_vertices(SNAP, K, [-10.0, -20.0, -10.0], [10.0, 20.0, 10.0], seed, nd=5)
    t = O.estimate_segment_times(v, 3.0, 5.0)
    res = O.solve_linear(10, SNAP, v, m, t)
    vals, mk = to_abi(v[None], m[None], 10)
    assert check_path(vals, mk, t[None], res["coeffs"][None], 10) < 1e-6
    assert _max_magnitude(res["coeffs"], t, 1) < 3.0 * vfac
    assert _max_magnitude(res["coeffs"], t, 2) < 5.0 * afac
    # checkCost (:133-152): analytic computeCost vs Riemann sum within 10 %
    num = _cost_numeric(res["coeffs"], t, SNAP)
    assert abs(num - 2 * res["cost"]) <= 0.1 * num or abs(num - res["cost"]) <= 0.1 * num


def test_two_vertices_rand():
    """2_vertices_rand (:747-774): 100 seeds, one segment, ends fixed to ACCELERATION."""
    for seed in range(12345, 12345 + 100):
        v, m = O.create_random_vertices(ACC, 1, [-50.0] * 3, [50.0] * 3, seed, nd=5)
        t = O.estimate_segment_times(v, 3.0, 5.0)
        res = O.solve_linear(10, 4, v, m, t)
        vals, mk = to_abi(v[None], m[None], 10)
        assert check_path(vals, mk, t[None], res["coeffs"][None], 10) < 1e-6


def test_error_behaviour():
    v, m = O.create_random_vertices(SNAP, 3, [-1.0], [1.0], 1, nd=5)
    t = O.estimate_segment_times(v, 3.0, 5.0)
    assert O.solve_linear(10, 5, v, m, t)["rc"] == O.ORACLE_ERR_BAD_DERIVATIVE  # lin_impl:50-55
    t2 = t.copy()
    t2[1] = 0.0
    assert O.solve_linear(10, 4, v, m, t2)["rc"] == O.ORACLE_ERR_BAD_TIME  # lin_impl:287
    # N=8 cannot hold SNAP: dropped with a warning (lin_impl:74-95)
    assert O.solve_linear(8, 3, v, m, t)["rc"] == O.ORACLE_WARN_DROPPED


def test_evaluate_range_semantics():
    """Trajectory::evaluateRange (src/trajectory.cpp:68-128) incl. the segment-start time quirk."""
    v, m = O.create_random_vertices(SNAP, 3, [-5.0], [5.0], 3, nd=5)
    t = np.array([1.0, 2.0, 1.5])
    c = O.solve_linear(10, 4, v, m, t)["coeffs"]
    out, st, n = O.evaluate_range(c, t, 0.0, 4.5, 0.5)
    assert n == len(st) == 9  # acc = 0, .5, ..., 4.0 (4.5 fails acc < t_end)
    assert np.allclose(st, np.arange(9) * 0.5)
    # a segment is left only when tin > T_i (strict), so tin == T_i samples the old segment's end
    assert np.allclose(out[:, 0], [poly_eval(c[0, 0], 0.0), poly_eval(c[0, 0], 0.5), poly_eval(c[0, 0], 1.0),
                                   poly_eval(c[1, 0], 0.5), poly_eval(c[1, 0], 1.0), poly_eval(c[1, 0], 1.5),
                                   poly_eval(c[1, 0], 2.0), poly_eval(c[2, 0], 0.5), poly_eval(c[2, 0], 1.0)])
    # t_start mid-segment: sampling times restart from the segment start (:104-123)
    _, st2, n2 = O.evaluate_range(c, t, 1.25, 2.0, 0.25)
    assert st2[0] == 1.0 and n2 == 4
    # start beyond the end: nothing
    assert O.evaluate_range(c, t, 10.0, 11.0, 0.1)[2] == 0


def test_cost_at_times_oracle_consistency():
    """getCostAndGradientDerivative's J = sum d^T R d (nl_impl:1452-1520) at the solved times is
    2 x computeCost (lin_impl:114-130); scaling all times by s scales the cost of the SAME
    derivatives as expected; full_vertex_values rebuilds d in the reference's free order."""
    import mav_trajectory_generation_cmake_amd as mtg
    vals, mask, times = mtg.random_vertices_path_batch(10, 3, 10, 6, seed0=40)
    free = np.zeros((6, 3, 55))
    cost = np.zeros(6)
    for b in range(6):
        r = O.solve_linear(10, 4, vals[b], mask[b].astype(np.uint32), times[b])
        free[b, :, :r["n_free"]] = r["free"]
        cost[b] = r["cost"]
    xf = mtg.full_vertex_values(vals, mask, free, 10)
    fixed = ((mask[:, :, None] >> np.arange(5)) & 1).astype(bool)
    np.testing.assert_array_equal(xf[fixed], vals[fixed])
    J = O.cost_at_times_batch(10, 4, xf, times, np.array([[1.0] * 10, [2.0] * 10]))
    np.testing.assert_allclose(J[:, 0], 2 * cost, rtol=1e-9)
    assert np.all(J[:, 1] > 0) and np.all(np.isfinite(J[:, 1]))


def _mp_segment_cost(N, r, T, xs):
    """sum_dims x^T A^-T Q A^-1 x for one segment in 40-digit arithmetic (independent of the
    oracle: exact A(T) of lin_impl:102-111 and Q(T) of :574-589, mpmath inverse)."""
    import mpmath as mp
    h = N // 2
    T = mp.mpf(T)

    def ff(i, n):  # falling factorial i!/(i-n)!
        return mp.mpf(0) if i < n else mp.factorial(i) / mp.factorial(i - n)
    A = mp.matrix(N, N)
    for d in range(h):
        for j in range(N):
            A[d, j] = ff(j, d) * (mp.mpf(0) ** (j - d) if j >= d else 0) if j != d else ff(j, d)
            A[h + d, j] = ff(j, d) * T ** (j - d) if j >= d else 0
    Q = mp.matrix(N, N)
    for i in range(r, N):
        for j in range(r, N):
            e = i + j - 2 * r + 1
            Q[i, j] = 2 * ff(i, r) * ff(j, r) * T ** e / e
    Ai = A ** -1
    H = Ai.T * Q * Ai
    tot = mp.mpf(0)
    for x in xs:
        v = mp.matrix([mp.mpf(float(t)) for t in x])
        tot += (v.T * H * v)[0]
    return tot


def test_time_jacobian_oracle_vs_mpmath():
    """The oracle's exact time derivative of J_d (Richardson limit of the reference's central
    difference) against mpmath.diff of the independently built 40-digit segment cost; the
    increment_time mode equals the reference's formula applied to oracle_cost_at_times_batch."""
    import mpmath as mp
    with mp.workdps(40):
        _time_jacobian_checks(mp)


def _time_jacobian_checks(mp):
    rng = np.random.default_rng(7)
    N, r, K, D = 6, 2, 3, 2
    h = N // 2
    xf = rng.uniform(-3, 3, size=(1, K + 1, h, D))
    times = np.array([[0.7, 1.9, 0.35]])
    scales = np.array([[1.0, 1.0, 1.0], [1.3, 0.8, 1.1]])
    J, G = O.cost_time_jacobian_batch(N, r, xf, times, scales, 0.0)
    for c in range(2):
        Jm = 0.0
        for n in range(K):
            Tn = times[0, n] * scales[c, n]
            xs = [np.concatenate([xf[0, n, :, d], xf[0, n + 1, :, d]]) for d in range(D)]
            Jm += float(_mp_segment_cost(N, r, Tn, xs))
            gm = float(mp.diff(lambda t: _mp_segment_cost(N, r, t, xs), mp.mpf(Tn)))
            assert abs(G[0, c, n] - gm) <= 1e-8 * abs(gm), (c, n, G[0, c, n], gm)
        assert abs(J[0, c] - Jm) <= 1e-11 * abs(Jm)
    # increment_time mode: (J(T_n + dt) - J(T_n - dt)) / (2 dt) with the 0.1 floor
    dt = 0.1
    times2 = np.array([[0.7, 0.08, 0.35]])  # segment 1 is below the floor: gradient 0
    J2, G2 = O.cost_time_jacobian_batch(N, r, xf, times2, scales[:1], dt)
    for n in range(K):
        sp = np.ones((2, K))
        sp[0, n] = (times2[0, n] + dt) / times2[0, n]
        sp[1, n] = (times2[0, n] - dt) / times2[0, n]
        Jpm = O.cost_at_times_batch(N, r, xf, times2, sp)
        want = 0.0 if times2[0, n] <= 0.1 else (Jpm[0, 0] - Jpm[0, 1]) / (2 * dt)
        assert abs(G2[0, 0, n] - want) <= 1e-9 * max(abs(J2[0, 0]), 1.0) / dt, (n, G2[0, 0, n], want)
    assert G2[0, 0, 1] == 0.0


def test_vertex_maps_oracle_round_trip():
    """coefficients_from_vertices (lin_impl:253-273) then M^+ A p (nl_impl:162-180) returns the vertex
    derivatives: A_i c_i reproduces both segment ends, so the pseudo-inverse's average is exact."""
    rng = np.random.default_rng(11)
    for N, K, D in ((10, 4, 3), (6, 3, 2), (12, 2, 1)):
        h = N // 2
        x = rng.uniform(-2, 2, size=(K + 1, h, D))
        times = rng.uniform(0.5, 3.0, size=K)
        c = O.coefficients_from_vertices(N, x, times)
        back = O.vertex_derivatives(N, c, times)
        np.testing.assert_allclose(back, x, rtol=1e-8, atol=1e-9 * np.abs(x).max())


def test_min_max_magnitude_oracle_vs_sampling():
    """computeMinMaxMagnitude's candidates against dense sampling, as the reference's own test checks
    its root-based extrema (test/test_polynomial_optimization.cpp:447-487, sampling at 1e-3 s)."""
    import mav_trajectory_generation_cmake_amd as mtg
    vals, mask, times = mtg.random_vertices_path_batch(10, 3, 6, 3, seed0=70)
    for b in range(3):
        r = O.solve_linear(10, 4, vals[b], mask[b].astype(np.uint32), times[b])
        c = r["coeffs"]
        for k in (1, 2):
            mn, mx = O.min_max_magnitude(10, c, times[b], k)
            best_hi, best_lo = -1.0, np.inf
            for i in range(6):
                t = np.linspace(0.0, times[b, i], 4001)
                m = np.sqrt(sum(np.polyval(np.polyder(c[i, d][::-1], k), t) ** 2 for d in range(3)))
                best_hi, best_lo = max(best_hi, m.max()), min(best_lo, m.min())
            assert best_hi <= mx[1] * (1 + 1e-12) and mx[1] <= best_hi * (1 + 1e-5), (b, k, mx, best_hi)
            assert mn[1] <= best_lo * (1 + 1e-12) + 1e-12 and best_lo <= mn[1] + 1e-5 * best_hi, (b, k, mn, best_lo)
