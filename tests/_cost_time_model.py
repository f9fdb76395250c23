"""Truth model of the fixed-derivative cost J_d, its segment-time derivative and its gradient
(mtg_cost_at_times_batch, mtg_time_jacobian_batch), in 50-digit mpmath arithmetic.

Written from the reference's formulas, independent of the library's tables and of the oracle:
setupMappingMatrix (polynomial_optimization_linear_impl.h:102-111) gives A(T),
computeQuadraticCostJacobian (:574-589) gives Q(T), and the per-segment cost matrix is
H(T) = A(T)^-T Q(T) A(T)^-1 on the 2h end derivatives x = [x_i; x_{i+1}] (h = N/2).  H1 = H(1) is
formed once per (N, r) in exact rationals; every other T follows from the scaling identity

    H_pq(T) = H1_pq T^(e_pq),    e_pq = (p mod h) + (q mod h) + 1 - 2r,

(test_cost_time_model.py checks it against the exact direct product), so no matrix is inverted per
value.  For r >= 1 every sum is taken on translation-relative positions (x_h -= x_0, then x_0 = 0):
H annihilates a common position offset, so the value is unchanged, and the absolute-sum companions
S below then measure the arithmetic that is really needed.

Per trajectory, candidate c and segment i, with T = fl(times[i] * scales[c][i]) (the FP64 product: a
candidate time is an FP64 number, as in the reference):

    J_i  = sum_d sum_pq H_pq(T) x_p x_q                 S_i  = sum |terms|
    J_i' = sum_d sum_pq e_pq H_pq(T) x_p x_q / T        S_i' = sum |terms|
    D_i  = (J_i(T + dt) - J_i(T - dt)) / (2 dt), the reference's central difference
           (polynomial_optimization_nonlinear_impl.h:2180-2223): exactly 0 for T <= 0.1 (both
           perturbed times are floored to 0.1), NaN for T > 0.1 with T - dt <= 0
    g    = 2 (R d)_free: vertex v, order k collects 2 sum_q H_pq(T) x_q of the two segments that
           meet at v (rows k of segment v and h + k of segment v - 1); S^g = sum |terms|

Truth values are mpmath numbers (object arrays); the companions S only scale a tolerance, need two
digits, and are FP64.  Grouping the terms by m = (p mod h) + (q mod h) turns each J_i into
T^(1-2r) sum_m a_m T^m with a_m formed once per (trajectory, segment) -- exact regrouping, the sums
are the same.
"""
import functools
from fractions import Fraction

import mpmath
import numpy as np

MP = mpmath.mp.clone()
MP.dps = 50

U = 2.0 ** -53

PAIRS = [(N, r) for N in range(2, 13, 2) for r in range(N // 2)]


def roundings(N, D, K):
    """Worst-case number of roundings a term of any compared sum passes through (table entry,
    products, a_m accumulation, T^e powers, the refined reciprocal, Horner or MFMA accumulation, the
    segment sum): |got - truth| <= roundings * U * S."""
    return N * N + 4 * N + D + K + 16


def falling(n, i):
    """i! / (i - n)!, the n-th derivative's factor of t^i (0 for i < n)."""
    out = 1
    for k in range(i - n + 1, i + 1):
        out *= k
    return out if i >= n else 0


def mapping_matrix(N, T):
    """A(T): rows k < h the derivatives at t = 0, rows h + k at t = T (exact rationals)."""
    h = N // 2
    A = [[Fraction(0)] * N for _ in range(N)]
    for k in range(h):
        A[k][k] = Fraction(falling(k, k))
        for j in range(k, N):
            A[h + k][j] = falling(k, j) * T ** (j - k)
    return A


def cost_matrix(N, r, T):
    """Q(T) = 2 int_0^T (d^r t^a)(d^r t^b) dt, with the reference's factor 2."""
    Q = [[Fraction(0)] * N for _ in range(N)]
    for a in range(r, N):
        for b in range(r, N):
            e = a + b - 2 * r + 1
            Q[a][b] = 2 * falling(r, a) * falling(r, b) * T ** e / e
    return Q


def solve_columns(A, B):
    """X with A X = B by fraction elimination and back substitution (A square, regular)."""
    n, m = len(A), len(B[0])
    W = [list(A[i]) + list(B[i]) for i in range(n)]
    for c in range(n):
        piv = next(i for i in range(c, n) if W[i][c] != 0)
        W[c], W[piv] = W[piv], W[c]
        for i in range(c + 1, n):
            if W[i][c] != 0:
                f = W[i][c] / W[c][c]
                W[i] = [wi - f * wc for wi, wc in zip(W[i], W[c])]
    X = [[Fraction(0)] * m for _ in range(n)]
    for i in range(n - 1, -1, -1):
        for j in range(m):
            X[i][j] = (W[i][n + j] - sum(W[i][k] * X[k][j] for k in range(i + 1, n))) / W[i][i]
    return X


def H_direct(N, r, T):
    """A(T)^-T Q(T) A(T)^-1 in exact rationals (T a Fraction)."""
    T = Fraction(T)
    A, Q = mapping_matrix(N, T), cost_matrix(N, r, T)
    eye = [[Fraction(int(i == j)) for j in range(N)] for i in range(N)]
    Ai = solve_columns(A, eye)
    QAi = [[sum(Q[i][k] * Ai[k][j] for k in range(N)) for j in range(N)] for i in range(N)]
    return [[sum(Ai[k][i] * QAi[k][j] for k in range(N)) for j in range(N)] for i in range(N)]


@functools.lru_cache(maxsize=None)
def H1(N, r):
    """H(1) of (N, r): N x N exact rationals."""
    return tuple(tuple(row) for row in H_direct(N, r, 1))


def exponent(N, r, p, q):
    h = N // 2
    return (p % h) + (q % h) + 1 - 2 * r


def mpf(v):
    if isinstance(v, Fraction):
        return MP.mpf(v.numerator) / MP.mpf(v.denominator)
    return MP.mpf(float(v))


@functools.lru_cache(maxsize=None)
def _h1_tables(N, r):
    Hf = H1(N, r)
    return ([[mpf(v) for v in row] for row in Hf], np.array([[float(v) for v in row] for row in Hf]))


def H_scaled(N, r, T):
    """H(T) by the scaling identity, mpmath (T anything mpf takes, or a Fraction)."""
    Hm, _ = _h1_tables(N, r)
    T = mpf(T)
    return [[Hm[p][q] * T ** exponent(N, r, p, q) for q in range(N)] for p in range(N)]


class Trajectory:
    """The model of one trajectory: vertex values x [V][h][D] (FP64, taken exactly)."""

    def __init__(self, N, r, x):
        x = np.asarray(x, dtype=np.float64)
        self.N, self.r, self.h = N, r, N // 2
        self.V, _, self.D = x.shape
        self.K = self.V - 1
        h, D, K = self.h, self.D, self.K
        assert x.shape[1] == h
        self.M = 2 * h - 1
        self.e = [m + 1 - 2 * r for m in range(self.M)]
        Hm, Hf = _h1_tables(N, r)
        # segment end values [K][D][N], translation-relative for r >= 1 (exact in mpmath)
        self.xs = []
        for i in range(K):
            seg = []
            for d in range(D):
                v = [MP.mpf(float(x[i, k, d])) for k in range(h)] + [MP.mpf(float(x[i + 1, k, d])) for k in range(h)]
                if r >= 1:
                    v[h] = v[h] - v[0]
                    v[0] = MP.mpf(0)
                seg.append(v)
            self.xs.append(seg)
        xf = np.array([[[float(t) for t in v] for v in seg] for seg in self.xs]).reshape(K, D, N)
        # a[i][m] = sum_d sum_{(p mod h) + (q mod h) = m} H1_pq x_p x_q, and the absolute sums A
        self.a = [[MP.mpf(0)] * self.M for _ in range(K)]
        for i in range(K):
            for d in range(D):
                v = self.xs[i][d]
                for p in range(N):
                    if v[p] == 0:
                        continue
                    self.a[i][2 * (p % h)] += Hm[p][p] * v[p] * v[p]
                    for q in range(p + 1, N):
                        self.a[i][(p % h) + (q % h)] += 2 * Hm[p][q] * v[p] * v[q]
        mofpq = (np.arange(N)[:, None] % h) + (np.arange(N)[None, :] % h)
        terms = np.abs(Hf[None, None] * xf[:, :, :, None] * xf[:, :, None, :]).sum(axis=1)  # [K][N][N]
        self.A = np.stack([np.where(mofpq == m, terms, 0.0).sum(axis=(1, 2)) for m in range(self.M)], axis=1)
        # gradient rows: b[i][d][p][j] = H1[p][j] x_j + H1[p][j + h] x_{j+h}, and the absolute sums
        self._b = None
        self._Hm, self._Hf, self._xf = Hm, Hf, xf

    # ---- one segment at one time ------------------------------------------------------------
    def _horner(self, coef, T):
        acc = coef[-1]
        for c in reversed(coef[:-1]):
            acc = acc * T + c
        return acc

    def J_seg(self, i, T):
        """J_i(T), T an mpmath number."""
        return self._horner(self.a[i], T) * T ** (1 - 2 * self.r)

    def dJ_seg(self, i, T):
        ea = [e * a for e, a in zip(self.e, self.a[i])]
        return self._horner(ea, T) * T ** (-2 * self.r)

    def S(self, T):
        """S_i for FP64 times T [..., K] -> [..., K]."""
        T = np.asarray(T, dtype=np.float64)
        return sum(self.A[:, m] * T ** self.e[m] for m in range(self.M))

    def S_prime(self, T):
        T = np.asarray(T, dtype=np.float64)
        return sum(abs(self.e[m]) * self.A[:, m] * T ** (self.e[m] - 1) for m in range(self.M))

    # ---- candidates --------------------------------------------------------------------------
    def evaluate(self, T, dt=None):
        """T [C][K] FP64 candidate times.  Returns a dict: Ji, dJ [C][K] and J [C] (mpmath, object
        arrays), Si, Sd [C][K], S [C] (FP64); with dt also diff [C][K] (mpmath; float 0.0 at the
        floor, float NaN where the reference divides by a non-positive time) and Sdiff [C][K] =
        [S_i(T + dt) + S_i(T - dt)] / (2 dt) (0 where diff is exactly 0, NaN where it is NaN)."""
        T = np.asarray(T, dtype=np.float64)
        C, K = T.shape
        assert K == self.K
        Ji = np.empty((C, K), dtype=object)
        dJ = np.empty((C, K), dtype=object)
        for c in range(C):
            for i in range(K):
                t = MP.mpf(float(T[c, i]))
                Ji[c, i] = self.J_seg(i, t)
                dJ[c, i] = self.dJ_seg(i, t)
        out = {"Ji": Ji, "dJ": dJ, "J": Ji.sum(axis=1), "Si": self.S(T), "Sd": self.S_prime(T)}
        out["S"] = out["Si"].sum(axis=1)
        if dt is not None:
            diff = np.empty((C, K), dtype=object)
            Sdiff = np.zeros((C, K))
            md = MP.mpf(float(dt))
            for c in range(C):
                for i in range(K):
                    tc = float(T[c, i])
                    if tc <= 0.1:
                        diff[c, i] = 0.0
                    elif tc - dt <= 0.0:
                        diff[c, i] = float("nan")
                        Sdiff[c, i] = float("nan")
                    else:
                        t = MP.mpf(tc)
                        diff[c, i] = (self.J_seg(i, t + md) - self.J_seg(i, t - md)) / (2 * md)
            ok = (T > 0.1) & (T - dt > 0.0)
            Tp, Tm = np.where(ok, T + dt, 1.0), np.where(ok, T - dt, 1.0)
            Sdiff = np.where(ok, (self.S(Tp) + self.S(Tm)) / (2.0 * dt), Sdiff)
            out["diff"], out["Sdiff"] = diff, Sdiff
        return out

    def _gradient_rows(self):
        if self._b is None:
            N, h = self.N, self.h
            Hm = self._Hm
            self._b = [[[[Hm[p][j] * v[j] + Hm[p][j + h] * v[j + h] for j in range(h)] for p in range(N)]
                        for v in seg] for seg in self.xs]
            HX = np.abs(self._Hf[None, None] * self._xf[:, :, None, :])  # [K][D][p][q]
            self._Bf = HX[..., :h] + HX[..., h:]  # [K][D][p][j]
        return self._b, self._Bf

    def gradient(self, T, mask):
        """T [C][K] FP64 candidate times, mask [V] (bit k set: derivative k of the vertex is fixed).
        Returns (g, Sg, n_free): g [C][D][n_free] mpmath and Sg FP64, in the reference's free order
        (vertex by vertex, ascending order)."""
        T = np.asarray(T, dtype=np.float64)
        C, K = T.shape
        h, D, r = self.h, self.D, self.r
        b, Bf = self._gradient_rows()
        free = [(v, k) for v in range(self.V) for k in range(h) if not (int(mask[v]) >> k) & 1]
        g = np.empty((C, D, len(free)), dtype=object)
        Sg = np.zeros((C, D, len(free)))
        for c in range(C):
            tm = [MP.mpf(float(t)) for t in T[c]]
            for d in range(D):
                for n, (v, k) in enumerate(free):
                    acc, sacc = MP.mpf(0), 0.0
                    for i, p in ((v, k), (v - 1, h + k)):
                        if 0 <= i < K:
                            acc += 2 * self._horner(b[i][d][p], tm[i]) * tm[i] ** (k + 1 - 2 * r)
                            tf = float(T[c, i])
                            sacc += 2.0 * float(np.dot(Bf[i, d, p], tf ** np.arange(h))) * tf ** (k + 1 - 2 * r)
                    g[c, d, n], Sg[c, d, n] = acc, sacc
        return g, Sg, len(free)


def abs_err(got, truth):
    """|got - truth| elementwise as FP64, the difference taken in mpmath (got FP64, truth mpmath)."""
    got = np.asarray(got, dtype=np.float64)
    truth = np.asarray(truth, dtype=object)
    assert got.shape == truth.shape, (got.shape, truth.shape)
    out = np.empty(got.shape)
    for idx in np.ndindex(got.shape):
        out[idx] = float(abs(MP.mpf(float(got[idx])) - truth[idx]))
    return out


def make_inputs(N, D, K, B, C, seed):
    """Arbitrary (unsolved) inputs: vertex_values [B][V][h][D] with positions U(-10, 10), plus a
    common offset of 1e3 in every second trajectory, and higher derivatives N(0, 2); times U(0.4, 6)
    with one segment of 0.12 (first trajectory) and one of 20 (last trajectory) planted; scales
    U(0.5, 1.5) with scales[0] = 1."""
    rng = np.random.default_rng(seed)
    h = N // 2
    vals = rng.normal(0.0, 2.0, size=(B, K + 1, h, D))
    vals[:, :, 0, :] = rng.uniform(-10.0, 10.0, size=(B, K + 1, D))
    vals[1::2, :, 0, :] += 1e3
    times = rng.uniform(0.4, 6.0, size=(B, K))
    times[0, 0] = 0.12
    if B * K > 1:
        times[-1, -1] = 20.0
    scales = rng.uniform(0.5, 1.5, size=(C, K))
    scales[0] = 1.0
    return vals, times, scales
