"""Truth model of the two maps between a trajectory's vertex derivatives and its coefficients
(mtg_coefficients_from_vertices_batch, mtg_vertex_derivatives_batch and the host twin
mtg_host_coefficients_from_vertices_batch), in 60-digit mpmath arithmetic.

Written from the reference's formulas and nothing else: setupMappingMatrix
(polynomial_optimization_linear_impl.h:102-111) with baseCoeffsWithTime (polynomial.h:215-233) gives
A(T) per segment (rows k < h: k! on the diagonal, the derivatives at t = 0; rows h + k:
j!/(j-k)! T^(j-k), the derivatives at t = T), and

    c = A(T)^-1 [x_i; x_{i+1}]       per (segment, dimension), one mpmath LU solve each,
    x_v = M^+ A p                    the mean of p_v^(k)(0) and p_{v-1}^(k)(T_{v-1}) at an interior
                                     vertex, the single value at the first / last one
                                     (polynomial_optimization_nonlinear_impl.h:162-180).

No Schur inverse, no A(1)^-1 table and no time scaling: the model shares no step with the library or
with the oracle.  The FP64 inputs are taken exactly.  Truth values are mpmath numbers (object
arrays); S, the sum of the absolute terms of a derivative's power sums, only scales a tolerance and
is FP64.
"""
import functools

import mpmath
import numpy as np

MP = mpmath.mp.clone()
MP.dps = 60

RANGES = ((0.05, 0.2), (0.5, 4.0), (10.0, 30.0))


def falling(k, j):
    """j! / (j - k)!, the factor of t^(j-k) in the k-th derivative of t^j (0 for j < k)."""
    if j < k:
        return 0
    out = 1
    for q in range(j - k + 1, j + 1):
        out *= q
    return out


def _mp(v):
    return v if isinstance(v, MP.mpf) else MP.mpf(float(v))


def mapping_matrix(N, T):
    """A(T) as an mpmath matrix (T an FP64 number, taken exactly)."""
    h, T = N // 2, _mp(T)
    A = MP.zeros(N, N)
    for k in range(h):
        A[k, k] = falling(k, k)
        for j in range(k, N):
            A[h + k, j] = falling(k, j) * T ** (j - k)
    return A


def truth_coefficients(N, x, T):
    """x [V][h][D] (FP64 or mpmath), T [K] -> c [K][D][N] (mpmath): A(T_i) c = [x_i; x_{i+1}]."""
    x = np.asarray(x)
    V, h, D = x.shape
    K = V - 1
    assert h == N // 2 and len(T) == K
    out = np.empty((K, D, N), dtype=object)
    for i in range(K):
        A = mapping_matrix(N, T[i])
        for d in range(D):
            rhs = MP.matrix([_mp(x[i, k, d]) for k in range(h)] + [_mp(x[i + 1, k, d]) for k in range(h)])
            c = MP.lu_solve(A, rhs)
            for j in range(N):
                out[i, d, j] = c[j]
    return out


def truth_vertex_derivatives(N, c, T):
    """c [K][D][N] (FP64 or mpmath), T [K] -> (x [V][h][D] mpmath, S [V][h][D] FP64).  S sums
    |j!/(j-k)! c_j T^(j-k)| over the segment ends that meet at the vertex."""
    c = np.asarray(c)
    K, D, _ = c.shape
    h, V = N // 2, K + 1
    x = np.empty((V, h, D), dtype=object)
    S = np.zeros((V, h, D))
    Tm = [_mp(t) for t in T]
    for v in range(V):
        for k in range(h):
            for d in range(D):
                ends, s = [], MP.mpf(0)
                if v < K:  # p_v^(k)(0) = k! c_k
                    t = falling(k, k) * _mp(c[v, d, k])
                    ends.append(t)
                    s += abs(t)
                if v > 0:  # p_{v-1}^(k)(T_{v-1}), the plain power sum
                    acc = MP.mpf(0)
                    for j in range(k, N):
                        t = falling(k, j) * _mp(c[v - 1, d, j]) * Tm[v - 1] ** (j - k)
                        acc += t
                        s += abs(t)
                    ends.append(acc)
                x[v, k, d] = sum(ends) / len(ends)
                S[v, k, d] = float(s)
    return x, S


def to_float(a):
    """Object array of mpmath numbers -> FP64, each correctly rounded."""
    a = np.asarray(a, dtype=object)
    out = np.empty(a.shape)
    for idx in np.ndindex(a.shape):
        out[idx] = float(a[idx])
    return out


def abs_err(got, truth):
    """|got - truth| elementwise as FP64, the difference taken in mpmath (got FP64, truth mpmath)."""
    got = np.asarray(got, dtype=np.float64)
    truth = np.asarray(truth, dtype=object)
    assert got.shape == truth.shape, (got.shape, truth.shape)
    out = np.empty(got.shape)
    for idx in np.ndindex(got.shape):
        out[idx] = float(abs(MP.mpf(float(got[idx])) - truth[idx]))
    return out


def shape_error(c, ref, times):
    """_util.scale_normalised_error over k >= 1 only: max_k>=1 |c_k - ref_k| T^k / max_k>=1 |ref_k| T^k.
    Numerator and scale both drop c_0, so a position offset does not enter.  (Dropping the first
    column and calling the full metric divides numerator and scale by the same T.)"""
    from _util import scale_normalised_error
    return scale_normalised_error(np.asarray(c)[..., 1:], np.asarray(ref)[..., 1:], times)


# ---- cases ---------------------------------------------------------------------------------------
def draw_times(rng, B, K, mode):
    """"mixed": per segment one of RANGES at random, then uniform in it.  "equal": one such time per
    trajectory, on all its segments.  "unequal": 0.05 next to 30, alternating, the first by parity of
    the trajectory."""
    if mode == "unequal":
        alt = np.where((np.arange(K)[None, :] + np.arange(B)[:, None]) % 2 == 0, 0.05, 30.0)
        return alt.astype(np.float64)
    shape = (B, 1) if mode == "equal" else (B, K)
    pick = rng.integers(0, len(RANGES), size=shape)
    lo = np.array([r[0] for r in RANGES])[pick]
    hi = np.array([r[1] for r in RANGES])[pick]
    t = rng.uniform(lo, hi)
    return np.ascontiguousarray(np.broadcast_to(t, (B, K)))


def inputs(N, D, K, B, seed=0, offset=0.0, mode="mixed"):
    """The inputs of one case: x [B][V][h][D] uniform in [-3, 3] per derivative plus `offset` on every
    position; T [B][K] (draw_times); c [B][K][D][N] coefficient blocks drawn independently per segment,
    c_j = u_j / (j! T^j) with u uniform in [-3, 3] (every term of p(T) is O(1); consecutive segments do
    not meet: the two ends at an interior vertex differ by O(1))."""
    rng = np.random.default_rng([seed, N, D, K, B])
    h = N // 2
    x = rng.uniform(-3.0, 3.0, size=(B, K + 1, h, D))
    x[:, :, 0, :] += offset
    T = draw_times(rng, B, K, mode)
    u = rng.uniform(-3.0, 3.0, size=(B, K, D, N))
    fact = np.cumprod([1.0] + list(range(1, N)))
    c = u / (fact * T[:, :, None, None] ** np.arange(N))
    return x, T, c


@functools.lru_cache(maxsize=None)
def coefficient_case(N, D, K, B, seed=0, offset=0.0, mode="mixed"):
    """inputs() with the truth of the coefficient map: dict(x, T, truth [B][K][D][N] mpmath,
    truth64 (the same, correctly rounded: for the 1e-9 metrics of _util, which a rounding of
    2^-53 relative per coefficient does not touch))."""
    x, T, _ = inputs(N, D, K, B, seed, offset, mode)
    truth = np.stack([truth_coefficients(N, x[b], T[b]) for b in range(B)])
    out = {"N": N, "x": x, "T": T, "truth": truth, "truth64": to_float(truth)}
    for a in (x, T, out["truth64"]):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def derivative_case(N, D, K, B, seed=0, offset=0.0, mode="mixed"):
    """inputs() with the truth of the derivative map on the discontinuous coefficients:
    dict(c, T, truth [B][V][h][D] mpmath, S [B][V][h][D])."""
    _, T, c = inputs(N, D, K, B, seed, offset, mode)
    both = [truth_vertex_derivatives(N, c[b], T[b]) for b in range(B)]
    out = {"N": N, "c": c, "T": T, "truth": np.stack([t for t, _ in both]), "S": np.stack([s for _, s in both])}
    for a in (c, T, out["S"]):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def round_trip_case(N, D, K, B, seed=0):
    """Truth of coefficients_from_vertices(vertex_derivatives(c)) on the discontinuous c of
    derivative_case: the composition taken in mpmath throughout (no rounding between the maps)."""
    dc = derivative_case(N, D, K, B, seed)
    truth = np.stack([truth_coefficients(N, dc["truth"][b], dc["T"][b]) for b in range(B)])
    return {"c": dc["c"], "T": dc["T"], "truth": truth, "truth64": to_float(truth)}


# ---- the shapes (N, D, K, B) -----------------------------------------------------------------------
# The kernels stage 8 * ((K+1)*h*D + K + K*D*N) bytes per trajectory in 48 KiB = 6144 doubles of LDS; a
# block owns TB = min(16, floor(6144 / doubles per trajectory)) rounded down to even trajectories, and
# the shape fits iff TB >= 2.
#   N = 10, D = 3: 15 (K+1) + K + 30 K = 46 K + 15 doubles.  K = 1: 61 -> 100 -> TB = 16.
#                  K = 10: 475 -> 12.  K = 40: 1855 -> 3 -> TB = 2.  K = 66: 3051 -> 2 (the last K that
#                  fits: 2 * 3051 = 6102 <= 6144).  K = 67: 3097 -> 1 -> does not fit.
#   N = 12, D = 3: 18 (K+1) + K + 36 K = 55 K + 18 doubles.  K = 55: 3043 -> 2.  K = 56: 3098 -> 1.
#   N = 6, K = 2:  9 D + 2 + 12 D = 21 D + 2 doubles.  D = 146: 3068 -> 2.  D = 147: 3089 -> 1.
# The entry points accept every D >= 1 (check_dims has no upper limit), so the largest D that is
# accepted at (N = 6, K = 2) is the largest that fits, 146.
D_MAX = 146
EVERY_N = tuple((N, 3, 3, 5) for N in (2, 4, 6, 8, 10, 12))
SHAPES = EVERY_N + (
    (10, 3, 1, 33),      # K = 1, TB = 16: two full blocks and a tail block of one trajectory
    (12, 1, 7, 18), (8, 4, 5, 7), (6, D_MAX, 2, 3),  # other D
    (10, 3, 66, 3), (12, 3, 55, 3),  # TB = 2 at the last K that fits; odd B: the last block has nb = 1
    (10, 3, 40, 5),      # quotient 3 rounded to TB = 2: LDS regions strided by TB, last block nb = 1
)
TOO_LARGE = ((10, 3, 67, 2), (12, 3, 56, 2))  # the first K that does not fit
OFFSET_SHAPES = ((10, 3, 3, 5), (2, 3, 3, 5))  # position offset 1e8
OFFSET = 1e8
TIME_MODE_SHAPES = (((10, 3, 4, 5), "equal"), ((10, 3, 4, 5), "unequal"))  # the segment-time index


def shape_id(s):
    return "N%d-D%d-K%d-B%d" % s
