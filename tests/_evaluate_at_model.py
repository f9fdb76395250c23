"""The definition of mtg_evaluate_at_batch (include/mtg.h) in numpy / Python floats: Trajectory::evaluate
(src/trajectory.cpp:41-66) over Polynomial::evaluate (polynomial.h:138-151) at caller-given times.

Only elementwise `*`, `+` and `-` on float64, so every rounding is separate (numpy never fuses them); the
segment times are accumulated in an explicit loop, never with np.sum.  evaluate_at(..., fused=True) is the
model of a contracted build: each Horner step r * tl + term rounded once (exact rational arithmetic, then
one rounding), for showing that the tests' inputs can tell the two apart."""
from fractions import Fraction

import numpy as np

MTG_TRAJ_BAD_TIME = 1


def base(k, j):
    """Polynomial::base_coefficients_(k, j) = j!/(j-k)!, exact in a double for j < 12."""
    if j < k:
        return 0.0
    out = 1.0
    for i in range(j - k + 1, j + 1):
        out = out * float(i)
    return out


def prefix(times_row):
    """[K + 1] accumulated segment times: sequential FP64 adds, 0 first."""
    out = [0.0]
    for T in times_row:
        out.append(out[-1] + float(T))
    return out


def broadcast_queries(t_query, B):
    t_query = np.asarray(t_query, dtype=np.float64)
    return np.broadcast_to(t_query, (B, t_query.shape[-1])) if t_query.ndim == 1 else t_query


def evaluate_at(coeffs, times, t_query, derivative_begin=0, n_derivatives=1, fused=False):
    """coeffs [B][K][D][N], times [B][K], t_query [M] or [B][M] -> (out [B][M][nd][D], in_range [B][M]
    uint8, status [B] int32)."""
    coeffs = np.asarray(coeffs, dtype=np.float64)
    times = np.asarray(times, dtype=np.float64)
    B, K, D, N = coeffs.shape
    tq = broadcast_queries(t_query, B)
    M = tq.shape[1]
    nd = n_derivatives
    out = np.zeros((B, M, nd, D))
    in_range = np.zeros((B, M), np.uint8)
    status = np.zeros(B, np.int32)
    with np.errstate(all="ignore"):
        for b in range(B):
            T = times[b]
            if any(not (float(x) > 0.0 and float(x) < float("inf")) for x in T):
                status[b] = MTG_TRAJ_BAD_TIME
                out[b] = np.nan
                continue
            t = tq[b]
            seg = np.full(M, K - 1)
            acc_i = np.zeros(M)
            found = np.zeros(M, bool)
            a = 0.0
            for i in range(K):  # trajectory.cpp:42-57
                a = a + float(T[i])
                hit = ~found & (a > t)
                seg[hit] = i
                acc_i[hit] = a
                found |= hit
            acc_i[~found] = a
            beyond = ~found & (t > a)
            nan = np.isnan(t)
            tl = t - (acc_i - T[seg])  # trajectory.cpp:63-65, not simplified
            c = coeffs[b][seg]  # [M][D][N]
            for q in range(nd):
                k = derivative_begin + q
                if k >= N:
                    continue
                if fused:
                    out[b, :, q, :] = _horner_fused(c, tl, k, N)
                    continue
                r = base(k, N - 1) * c[:, :, N - 1]
                for j in range(N - 2, k - 1, -1):
                    r = r * tl[:, None]
                    r = r + base(k, j) * c[:, :, j]
                out[b, :, q, :] = r
            out[b][beyond] = 0.0
            out[b][nan] = np.nan
            in_range[b] = ~(beyond | nan)
    return out, in_range, status


def _horner_fused(c, tl, k, N):
    """The Horner chain with each step an FMA: fl(r * tl + fl(base * c_j)), finite inputs only."""
    M, D, _ = c.shape
    out = np.zeros((M, D))
    for m in range(M):
        x = Fraction(float(tl[m]))
        for d in range(D):
            r = base(k, N - 1) * float(c[m, d, N - 1])
            for j in range(N - 2, k - 1, -1):
                term = base(k, j) * float(c[m, d, j])
                r = float(Fraction(r) * x + Fraction(term))  # int / int division rounds correctly
            out[m, d] = r
    return out


def random_case(rng, N, D, K, B, M):
    """Random coefficients, segment times spanning 7 ms to 10 s (the bench generator's range, log-uniform)
    and M random in-range query times per trajectory."""
    coeffs = rng.normal(size=(B, K, D, N))
    times = np.exp(rng.uniform(np.log(0.007), np.log(10.0), size=(B, K)))
    total = np.array([prefix(times[b])[-1] for b in range(B)])
    tq = rng.uniform(0.0, 1.0, size=(B, M)) * total[:, None] * (1.0 - 1e-12)
    return coeffs, times, tq


def edge_times(times_row):
    """The edge-case query times of one trajectory, each prefix value built by the sequential loop:
    0, -0.25, every interior prefix value, the total and its two neighbours, +inf, -inf, NaN."""
    p = prefix(times_row)
    total = p[-1]
    return np.array([0.0, -0.25] + p[1:-1] + [total, np.nextafter(total, np.inf), np.nextafter(total, -np.inf),
                                               np.inf, -np.inf, np.nan])


def derivative_pairs(N):
    """(derivative_begin, n_derivatives): the last two cover orders >= N, which give +0.0.  (N = 2 allows at
    most two orders per call: its (0, 3) is (0, 2).)"""
    return [(0, 1), (2, 1), (0, min(3, N)), (N - 1, 1), (N, 1), (N - 2, N)]


def assert_same_bits(got, want, what=""):
    """Bit-equal float64 arrays, except where both are NaN (sign and payload are not compared)."""
    got = np.ascontiguousarray(got, dtype=np.float64)
    want = np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, "NaN pattern differs", int((gn != wn).sum()))
    diff = (got.view(np.uint64) != want.view(np.uint64)) & ~gn
    assert not diff.any(), (what, "rows differing", int(diff.sum()), np.argwhere(diff)[:4].tolist())
