"""Shared cases of the solve-against-truth grid (tests/test_solve_truth_host.py, tests/test_gpu_solve_truth.py):
every (N, r) the library solves, at the segment counts on both sides of every kernel's K bucket and at
the dimension counts of every lane width, with 60-digit truth (tests/golden/make_golden.py) computed
once per problem and shared by every path that solves it.

The inputs are well conditioned on purpose (segment times within a factor of two, vertex 0 fixing
every derivative), so that an FP64 solve can be held to truth with no arbitration: the best FP64 solve
(make_golden.fp64_best_solve) is itself within BEST_TOL = TRUTH_TOL / 4 of truth on every problem
(test_solve_truth_host.py asserts it), the project's "within 4x of the best FP64 solve" rule
(tests/test_gpu_dlx.py) turned into a condition on the inputs.
"""
import os
import sys
from functools import lru_cache

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

TRUTH_TOL = 1e-9        # coefficients, scale-normalised
BEST_TOL = TRUTH_TOL / 4  # the condition on the inputs: the best FP64 solve against truth
ELEMENT_TOL = 1e-6      # element-wise, on coefficients >= ELEMENT_FLOOR of the segment's scale
ELEMENT_FLOOR = 1e-4
COST_TOL = 1e-9         # relative
FREE_TOL = 1e-7         # of the row's largest |value|

NR = [(N, r) for N in (2, 4, 6, 8, 10, 12) for r in range(N // 2)]
KINDS = ("pattern", "ends", "mixed")
# the fixed-length dimension-lane kernel's shapes (N, K): every D in 1..4 there
DL_SHAPES = {10: 10, 12: 20}
PROBLEMS = 2  # distinct problems per (N, r, K, kind)


def k_list(N):
    """Both sides of every K bucket edge of the column kernel (4 / 8 / 10 / 12, N = 12: 20), K == KMAX of
    every bucket, K = 1 (n_free may be 0), and the first K of the wide bucket and of the long-chain kernel."""
    return (1, 3, 4, 8, 10, 12, 13) if N <= 4 else (1, 3, 4, 5, 8, 9, 10, 11, 12, 13, 20, 21)


def lanes_per_chain(N, D):
    """The column kernel's lanes per chain (reg_geometry): N/2 column lanes + D dimension lanes, rounded
    up to a power of two, at least 8."""
    lc = 8
    while lc < N // 2 + D:
        lc *= 2
    return lc


def d_rotation(N):
    """The dimension counts a shape rotates through: 1..5 and 17 - N/2 (the first D of the 32-lane
    chain, a 64-lane group under twisting); for N <= 6, where none of those reaches a 16-lane chain
    (N/2 + 5 <= 8), also 9 - N/2, the first D that does."""
    h = N // 2
    out = []
    for D in (1, 2, 3, 4, 5, 9 - h, 17 - h):
        if D not in out:
            out.append(D)
    return out


def shapes(N, r):
    """The (K, D) a test of (N, r) visits.  At the DL shapes every D in 1..4; elsewhere one D per K.  The
    K the column kernel serves rotate through d_rotation(N) from its entry r + 1 on, so every (N, r) runs
    all three lane widths of the column kernel (asserted); the K beyond it (the long-chain kernel's,
    which has an instantiation per D <= 4) rotate from max(r - 1, 0) on, so they meet D = 1, 2, 3 at r = 1,
    2, 3, 4 at r = 2 and so on, and, where the list is long enough, a D > 4 (the general kernel)."""
    rot = d_rotation(N)
    out = []
    n_col = n_other = 0
    for K in k_list(N):
        if DL_SHAPES.get(N) == K:
            out += [(K, D) for D in (1, 2, 3, 4)]
        elif column_shape(N, 1, K):
            out.append((K, rot[(n_col + r + 1) % len(rot)]))
            n_col += 1
        else:
            out.append((K, rot[(n_other + max(r - 1, 0)) % len(rot)]))
            n_other += 1
    widths = {lanes_per_chain(N, D) for K, D in out if column_shape(N, D, K)}
    assert widths == {8, 16, 32}, (N, r, widths)
    return out


def full_d(N, r, K):
    """The D a problem is generated (and its truth computed) at: the largest D of its shape."""
    return max(D for k, D in shapes(N, r) if k == K)


# Cases whose first seed broke the condition on the inputs (BEST_TOL), with the draw that replaced it.
# (12, 0, 10, "ends"): the first draw pinned only the position at the last vertex of problem 0; at r = 0
# and N = 12 that leaves the best FP64 solve 9.2e-10 from truth.
_RESEED = {(12, 0, 10, "ends"): 1}


def _seed(N, r, K, kind):
    return 20240 + ((N * 8 + r) * 32 + K) * 4 + KINDS.index(kind) + 1000003 * _RESEED.get((N, r, K, kind), 0)


@lru_cache(maxsize=None)
def problems(N, r, K, kind):
    """(values [2][K+1][N/2][D], mask [2][K+1] uint8, times [2][K]) at D = full_d(N, r, K): positions a random
    walk of U(-3, 3) steps from a U(-20, 20) start, higher derivatives N(0, 1), segment times
    U(0.8, 1.6); vertex 0 fixes all N/2 derivatives (R_pp is SPD at every r), the other masks by kind:
    "pattern" the last vertex fully fixed and the interior ones exactly their position, "ends" the
    last vertex random pins | 1, "mixed" every later vertex random pins | 1.  Read-only arrays."""
    h = N // 2
    D = full_d(N, r, K)
    rng = np.random.default_rng(_seed(N, r, K, kind))
    P = PROBLEMS
    times = rng.uniform(0.8, 1.6, size=(P, K))
    pins = (rng.integers(0, 1 << h, size=(P, K + 1)) | 1).astype(np.uint8)
    mask = np.ones((P, K + 1), np.uint8)
    mask[:, 0] = (1 << h) - 1
    if kind == "pattern":
        mask[:, K] = (1 << h) - 1
    elif kind == "ends":
        mask[:, K] = pins[:, K]
    else:
        assert kind == "mixed"
        mask[:, 1:] = pins[:, 1:]
    vals = rng.normal(size=(P, K + 1, h, D))
    start = rng.uniform(-20.0, 20.0, size=(P, 1, D))
    steps = rng.uniform(-3.0, 3.0, size=(P, K, D))
    vals[:, :, 0, :] = np.concatenate([start, start + np.cumsum(steps, axis=1)], axis=1)
    assert not (np.array_equal(vals[0], vals[1]) or np.array_equal(times[0], times[1]))
    for a in (vals, mask, times):
        a.setflags(write=False)
    return vals, mask, times


def n_free_of(N, mask):
    """Free derivatives per trajectory: the clear bits of mask & (2^(N/2) - 1), counted."""
    h = N // 2
    m = np.asarray(mask).astype(np.int64) & ((1 << h) - 1)
    return (h * m.shape[-1] - sum(((m >> k) & 1) for k in range(h)).sum(axis=-1)).astype(np.int32)


@lru_cache(maxsize=None)
def truth(N, r, K, kind):
    """60-digit truth of problems(N, r, K, kind) and the best FP64 solve of the same systems: a dict of
    coeffs [2][K][D][N], free (a list of [D][n_free]), cost_d [2][D] (the cost's part per dimension) and
    best [2][K][D][N] (make_golden.fp64_best_solve).  Read-only."""
    from make_golden import _system, fp64_best_solve, truth_solve_banded
    vals, mask, times = problems(N, r, K, kind)
    out = {"coeffs": [], "free": [], "cost_d": [], "best": []}
    for p in range(PROBLEMS):
        system = _system(N, r, vals[p], mask[p], times[p])
        c, f, cost, cost_d = truth_solve_banded(N, r, vals[p], mask[p], times[p], full=True, system=system)
        assert f.shape[1] == n_free_of(N, mask[p]) and cost > 0.0 and np.all(cost_d > 0.0), (N, r, K, kind, p)
        out["coeffs"].append(c)
        out["free"].append(f)
        out["cost_d"].append(cost_d)
        out["best"].append(fp64_best_solve(N, r, vals[p], mask[p], times[p], system=system))
    for k in ("coeffs", "cost_d", "best"):
        out[k] = np.stack(out[k])
    for a in [out["coeffs"], out["cost_d"], out["best"]] + out["free"]:
        a.setflags(write=False)
    return out


def case(N, r, K, D, kind):
    """The problems and their truth at D dimensions (the first D of the generated ones: the dimensions
    are independent problems): (values, mask, times, truth) with truth["cost"] [2] the sum over them."""
    vals, mask, times = problems(N, r, K, kind)
    assert 1 <= D <= vals.shape[-1]
    t = truth(N, r, K, kind)
    tr = {"coeffs": t["coeffs"][:, :, :D, :], "free": [f[:D] for f in t["free"]],
          "cost": t["cost_d"][:, :D].sum(axis=1), "best": t["best"][:, :, :D, :],
          "n_free": n_free_of(N, mask)}
    return np.ascontiguousarray(vals[..., :D]), mask, times, tr


# ------------------------------------------------------------------ the kernel map
DL, COLUMN, DLX, GENERAL, SPLIT = ("solve_dl_kernel", "solve_reg_kernel", "solve_dlx_kernel", "solve_fused_kernel",
                                   "assemble+block_cholesky")


def column_shape(N, D, K):
    """The column kernel's shapes: its K buckets hold N/2 * KMAX <= 50 doubles of G per lane (N <= 8:
    K <= 12; N = 10: K <= 10; N = 12: K <= 8), N = 12 has the wide bucket 13 <= K <= 20, and a twisted
    trajectory's two chains fit a wave (N/2 + D <= 32).  (Its LDS fits at every such shape with D <= 16.)"""
    assert D <= 16
    if N // 2 + D > 32:
        return False
    if N <= 8:
        return K <= 12
    if N == 10:
        return K <= 10
    return K <= 8 or 13 <= K <= 20


def expected_kernel(N, D, K, r, path):
    """The kernel of a path ("default", "general", "split", "dl", "column") at a shape, from the written
    map alone (it does not ask the library)."""
    if path == "split":
        return SPLIT
    if path == "general":
        return GENERAL
    lanes = path in ("default", "dl")  # the dimension-lane kernels: by default and with the dl flag
    if lanes and DL_SHAPES.get(N) == K and 1 <= D <= 4 and r >= 1:
        return DL
    if column_shape(N, D, K):
        return COLUMN
    if lanes and N >= 6 and D <= 4 and r >= 1 and K >= 2:
        return DLX
    return GENERAL


PATHS = {"default": {}, "general": {"general": True}, "split": {"split": True}, "dl": {"dl": True},
         "column": {"column": True}}


# ------------------------------------------------------------------ a call's batch and its checks
def batch(N, r, K, D, kind, B):
    """case(N, r, K, D, kind) as a batch of B trajectories, the problems cycled (trajectory b is problem
    b % 2): (values, mask, times, truth)."""
    vals, mask, times, tr = case(N, r, K, D, kind)
    idx = np.arange(B) % PROBLEMS
    return vals[idx], mask[idx], times[idx], tr


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def check_outputs(out, N, times, tr, where):
    """One call's outputs (free, n_free, cost and status asked for) on a batch(): status 0 and n_free
    exact; the replicas of a problem bit-identical in every output; both problems against truth --
    coefficients within TRUTH_TOL scale-normalised and ELEMENT_TOL element-wise, cost within COST_TOL
    relative, free values within FREE_TOL of their dimension's largest.  No trajectory is exempt.
    Returns the worst scale-normalised coefficient error."""
    from _util import masked_elementwise_rel, scale_normalised_error
    B = len(out["coeffs"])
    assert np.all(out["status"] == 0), (where, out["status"])
    np.testing.assert_array_equal(out["n_free"], tr["n_free"][np.arange(B) % PROBLEMS], err_msg=str(where))
    worst = 0.0
    for p in range(PROBLEMS):
        nf = int(tr["n_free"][p])
        for k in ("coeffs", "free", "cost", "status", "n_free"):
            rows = out[k][p::PROBLEMS]
            if k == "free":
                rows = rows[:, :, :nf]
            assert np.array_equal(_bits(rows), np.broadcast_to(_bits(rows[:1]), rows.shape)), \
                (where, "replicas of problem %d differ in %s" % (p, k))
        sl = slice(p, p + 1)
        err = scale_normalised_error(out["coeffs"][sl], tr["coeffs"][sl], times[sl])
        worst = max(worst, err)
        assert err <= TRUTH_TOL, (where, p, "coefficients", err)
        el = masked_elementwise_rel(out["coeffs"][sl], tr["coeffs"][sl], times[sl], floor=ELEMENT_FLOOR)
        assert el <= ELEMENT_TOL, (where, p, "element-wise", el)
        rel_cost = abs(out["cost"][p] - tr["cost"][p]) / tr["cost"][p]  # (truth's cost > 0: truth())
        assert rel_cost <= COST_TOL, (where, p, "cost", rel_cost)
        if nf:
            ref = tr["free"][p]
            scale = np.max(np.abs(ref), axis=1, keepdims=True)
            assert np.all(scale > 0)
            fe = float(np.max(np.abs(out["free"][p][:, :nf] - ref) / scale))
            assert fe <= FREE_TOL, (where, p, "free values", fe)
    return worst
