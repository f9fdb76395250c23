"""CPU tests of the vertex <-> coefficient truth model (tests/_vertex_map_model.py): the model against
the reference algorithm in FP64 (the oracle's restatements) on every case the host and GPU tests use,
and against its own defining equation.  Without these a wrong model would go unnoticed.  No GPU."""
import numpy as np
import pytest

import _vertex_map_model as M
from _util import scale_normalised_error
from oracle import pyoracle as O

COEFF_TOL = 1e-9  # the bound of the library's own tests; the oracle stays below 1.2e-10 on these cases


def oracle_coefficients(case):
    """The reference algorithm in FP64 (the oracle's Schur inverse) on a coefficient case."""
    x, T = case["x"], case["T"]
    return np.stack([O.coefficients_from_vertices(case["N"], x[b], T[b]) for b in range(len(x))])


@pytest.mark.parametrize("shape", M.SHAPES, ids=M.shape_id)
def test_oracle_coefficients_agree_with_truth(shape):
    """The reference's Schur inverse in FP64 against the model, under both metrics."""
    case = M.coefficient_case(*shape)
    c = oracle_coefficients(case)
    full = scale_normalised_error(c, case["truth64"], case["T"])
    shp = M.shape_error(c, case["truth64"], case["T"])
    print("oracle vs truth %s: full %.2e shape %.2e" % (M.shape_id(shape), full, shp))
    assert full <= COEFF_TOL and shp <= COEFF_TOL, (full, shp)


@pytest.mark.parametrize("shape", M.EVERY_N, ids=M.shape_id)
def test_oracle_coefficients_agree_with_truth_at_offset_1e4(shape):
    case = M.coefficient_case(*shape, offset=1e4)
    c = oracle_coefficients(case)
    full = scale_normalised_error(c, case["truth64"], case["T"])
    shp = M.shape_error(c, case["truth64"], case["T"])
    print("oracle vs truth %s offset 1e4: full %.2e shape %.2e" % (M.shape_id(shape), full, shp))
    assert full <= COEFF_TOL and shp <= COEFF_TOL, (full, shp)


@pytest.mark.parametrize("shape", M.OFFSET_SHAPES, ids=M.shape_id)
def test_oracle_coefficients_at_offset_1e8(shape):
    """At a position offset of 1e8 the oracle still has the trajectory (the full metric, whose scale
    is the offset); what it loses is the shape, which test_vertex_map_host.py and
    test_gpu_vertex_map.py print beside the library's own figure."""
    case = M.coefficient_case(*shape, offset=M.OFFSET)
    c = oracle_coefficients(case)
    full = scale_normalised_error(c, case["truth64"], case["T"])
    print("oracle vs truth %s offset 1e8: full %.2e shape %.2e"
          % (M.shape_id(shape), full, M.shape_error(c, case["truth64"], case["T"])))
    assert full <= COEFF_TOL, full


def _derivative_cases():
    return [(s, "mixed") for s in M.SHAPES] + list(M.TIME_MODE_SHAPES)


@pytest.mark.parametrize("shape,mode", _derivative_cases(), ids=lambda v: M.shape_id(v) if isinstance(v, tuple) else v)
def test_oracle_vertex_derivatives_agree_with_truth(shape, mode):
    """The oracle forms M^+ A p with a dense pseudo-inverse: besides the rounding of its own row
    (about N u S) an entry collects about u times every other entry of A p of its (trajectory,
    dimension), which has 2 K h of them.  The bound is (N + 2) u S for the row and 2 K h u times the
    largest S of the (trajectory, dimension) for the rest, each with a factor 8 of margin: tight
    enough for any structural error of the model (a wrong end, sum for mean, a wrong time), which is
    O(S)."""
    N, D, K, B = shape
    case = M.derivative_case(*shape, mode=mode)
    u = 2.0 ** -53
    worst = 0.0
    for b in range(B):
        got = O.vertex_derivatives(N, case["c"][b], case["T"][b])
        err = M.abs_err(got, case["truth"][b])
        S = case["S"][b]
        bound = 8 * u * ((N + 2) * S + 2 * K * (N // 2) * S.max(axis=(0, 1), keepdims=True))
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), (b, float(np.max(err / bound)))
    print("oracle vs truth derivatives %s %s: worst err / bound %.2e" % (M.shape_id(shape), mode, worst))


@pytest.mark.parametrize("shape", M.EVERY_N + ((6, 7, 2, 2),), ids=M.shape_id)
def test_truth_coefficients_reproduce_their_inputs(shape):
    """A(T) c = [x_i; x_{i+1}] in mpmath to 1e-50 (relative to the largest term of the row)."""
    N, D, K, B = shape
    case = M.coefficient_case(*shape)
    h = N // 2
    tol = M.MP.mpf("1e-50")
    for b in range(B):
        for i in range(K):
            A = M.mapping_matrix(N, case["T"][b, i])
            for d in range(D):
                c = case["truth"][b, i, d]
                want = [case["x"][b, i, k, d] for k in range(h)] + [case["x"][b, i + 1, k, d] for k in range(h)]
                for row in range(N):
                    terms = [A[row, j] * c[j] for j in range(N)]
                    scale = max(max(abs(t) for t in terms), 1)
                    assert abs(sum(terms) - M.MP.mpf(float(want[row]))) <= tol * scale, (b, i, d, row)


def test_truth_maps_invert_each_other_on_continuous_input():
    """On the model's own coefficients (continuous by construction) the derivative map returns the
    vertex values it started from, and both ends agree: the mean equals either."""
    N, D, K, B = 8, 2, 3, 2
    case = M.coefficient_case(N, D, K, B)
    for b in range(B):
        x, S = M.truth_vertex_derivatives(N, case["truth"][b], case["T"][b])
        assert np.all(M.abs_err(case["x"][b], x) <= 1e-50 * S)


def test_truth_derivatives_on_a_hand_case():
    """p_0 = 1 + 2 t + 3 t^2 + 4 t^3 on T = 2 and p_1 = 5 + 6 t + 7 t^2 + 8 t^3 on T = 3, N = 4."""
    c = np.array([[[1.0, 2.0, 3.0, 4.0]], [[5.0, 6.0, 7.0, 8.0]]])
    x, S = M.truth_vertex_derivatives(4, c, np.array([2.0, 3.0]))
    # p_0(2) = 49, p_0'(2) = 62; p_1(3) = 302, p_1'(3) = 264
    want = np.array([[1.0, 2.0], [(49.0 + 5.0) / 2, (62.0 + 6.0) / 2], [302.0, 264.0]])
    assert np.array_equal(M.to_float(x)[:, :, 0], want)
    assert np.array_equal(S[:, :, 0], np.array([[1.0, 2.0], [49.0 + 5.0, 62.0 + 6.0], [302.0, 264.0]]))


def test_time_modes():
    """The generator's three time layouts are what the tests rely on."""
    _, T, _ = M.inputs(10, 3, 4, 5, mode="equal")
    assert np.all(T == T[:, :1]) and len(set(T[:, 0])) == 5
    _, T, _ = M.inputs(10, 3, 4, 5, mode="unequal")
    assert set(T.ravel()) == {0.05, 30.0} and np.all(T[:, 1:] != T[:, :-1])
    _, T, _ = M.inputs(10, 3, 66, 3)
    for lo, hi in M.RANGES:  # mixed within one trajectory
        assert all(np.any((T[b] >= lo) & (T[b] <= hi)) for b in range(3))
    assert np.all(np.any([(T >= lo) & (T <= hi) for lo, hi in M.RANGES], axis=0))


def test_shape_metric_drops_the_position():
    """shape_error ignores c_0 in numerator and scale and weighs c_k by T^k."""
    ref = np.array([[[[1e8, 2.0, 4.0]]]])
    T = np.array([[0.5]])
    c = ref + np.array([1.0, 0.0, 1e-3])
    assert M.shape_error(c, ref, T) == pytest.approx(1e-3 * 0.25 / 1.0, rel=1e-12)
    assert scale_normalised_error(c, ref, T) == pytest.approx(1.0 / 1e8, rel=1e-12)
