"""Shared inputs of the ragged evaluate / min-max tests (test_evaluate_ragged_host.py,
test_gpu_evaluate_ragged.py): solved coefficients of per-K batches (tests/_ragged_cases.py), their CSR
arrays in a given order, the query set, and the comparison against the uniform entry run on every packed
K-group."""
import numpy as np

import mav_trajectory_generation_cmake_amd as mtg
import _evaluate_at_model as model
from _ragged_cases import per_k_batches

EXTREMUM_FIELDS = ("time", "value", "segment", "reserved")


def solved_groups(N, D, counts, seed0=1):
    """{K: (coeffs [B_K][K][D][N], times [B_K][K])}: the host solve of per_k_batches problems (the bytes
    the ragged solves give for these trajectories, tests/test_ragged_host.py).  N = 2 has no derivative
    above the position to fix, which per_k_batches' generator call does not allow: its problems come from
    the same generator with max_derivative = 1 (the solver drops the velocity constraints)."""
    if N == 2:
        problems = {K: mtg.random_vertices_path_batch(N, D, K, B, seed0=seed0 + 1000 * i, max_derivative=1)
                    for i, (K, B) in enumerate(sorted(counts.items()))}
    else:
        problems = per_k_batches(N, D, counts, seed0=seed0)
    out = {}
    for K, (values, mask, times) in problems.items():
        out[K] = (mtg.host_solve_linear_batch(N, min(4, N // 2 - 1), values, mask, times)["coeffs"], times.copy())
    return out


def csr_of(groups, order):
    """(coeffs [sum K][D][N], times [sum K], seg_count [B]) of the trajectories in `order`."""
    coeffs = np.ascontiguousarray(np.concatenate([groups[K][0][i] for K, i in order]))
    times = np.ascontiguousarray(np.concatenate([groups[K][1][i] for K, i in order]))
    return coeffs, times, np.array([K for K, _ in order], dtype=np.int32)


def with_bad_times(groups, bad):
    """A copy of `groups` with times[K][i][j] = v for every ((K, i, j), v) of `bad`."""
    out = {K: (c, t.copy()) for K, (c, t) in groups.items()}
    for (K, i, j), v in bad.items():
        out[K][1][i, j] = v
    return out


def query_rows(groups, order, M, seed=0):
    """[B][M] query times for the trajectories in `order`: query_rows_of_times of their segment times."""
    return query_rows_of_times([groups[K][1][i] for K, i in order], M, seed)


def query_rows_of_times(times_blocks, M, seed=0):
    """[B][M] query times.  Row b starts with a window of trajectory b's edge times (0, t < 0, every
    prefix boundary exactly, the total and its neighbours -- the upper one lies beyond --, +-inf, NaN;
    model.edge_times), rotated by b so that a short row still meets all of them over the batch, and goes
    on with random times inside the trajectory.  M >= K + 7 holds every edge time of every row."""
    rng = np.random.default_rng(seed)
    rows = np.empty((len(times_blocks), M))
    for b, T in enumerate(times_blocks):
        good = np.where(np.isfinite(T) & (T > 0), T, 1.0)
        edge = model.edge_times(good)
        w = min(M, len(edge))
        shift = 0 if M >= len(edge) else 3 * b
        rows[b, :w] = edge[(shift + np.arange(w)) % len(edge)]
        rows[b, w:] = rng.uniform(0.0, 1.0, size=M - w) * model.prefix(good)[-1]
    return rows


def shared_row(groups, order, M, seed=0):
    """[M] query times for the whole batch: the edge times of the longest trajectory (beyond the end of the
    shorter ones), then random times up to its total."""
    K, i = max(order)
    return query_rows(groups, [(K, i)], M, seed)[0]


def evaluate_reference(evaluate_uniform, groups, order, tq, k0, nd):
    """(out [B][M][nd][D], in_range [B][M], status [B]) in batch order, from one
    evaluate_uniform(coeffs [B_K][K][D][N], times [B_K][K], t_query, k0, nd) per K-group, packed: the rows
    of a group's trajectories in the order they have in the batch."""
    B = len(order)
    out = in_range = status = None
    for K in sorted({K for K, _ in order}):
        members = [b for b, (k, _) in enumerate(order) if k == K]
        idx = [order[b][1] for b in members]
        q = tq if tq.ndim == 1 else np.ascontiguousarray(tq[members])
        o, r, s = (np.asarray(x.cpu().numpy() if hasattr(x, "cpu") else x)
                   for x in evaluate_uniform(np.ascontiguousarray(groups[K][0][idx]),
                                             np.ascontiguousarray(groups[K][1][idx]), q, k0, nd))
        if out is None:
            out = np.empty((B,) + o.shape[1:])
            in_range = np.empty((B,) + r.shape[1:], np.uint8)
            status = np.empty(B, np.int32)
        out[members], in_range[members], status[members] = o, r, s
    return out, in_range, status


def assert_same_evaluation(got, want, what=""):
    """Every byte of out (NaN rows: NaN in both), in_range and status."""
    got = [np.asarray(x.cpu().numpy() if hasattr(x, "cpu") else x) for x in got]
    nan = np.isnan(want[0])
    np.testing.assert_array_equal(np.isnan(got[0]), nan, err_msg="NaN pattern of out, %s" % (what,))
    np.testing.assert_array_equal(np.where(nan, 0.0, got[0]).view(np.uint64), np.where(nan, 0.0, want[0]).view(np.uint64),
                                  err_msg="out, %s" % (what,))
    np.testing.assert_array_equal(got[1], want[1], err_msg="in_range, %s" % (what,))
    np.testing.assert_array_equal(got[2], want[2], err_msg="status, %s" % (what,))


def check_call_level_errors(ctx):
    """Every call-level error of the two ragged entries, each returned with the outputs untouched: the
    host entries for ctx None, else the device entries on that context handle (host pointers)."""
    from mav_trajectory_generation_cmake_amd import _native as nat
    lib = nat.load()
    N, D, B, Mq = 10, 3, 3, 5
    seg = np.array([2, 1, 3], np.int32)
    c, t, q = np.zeros((6, D, N)), np.ones(6), np.zeros((B, Mq))
    out = np.full((B, Mq, 3, D), 7.0)
    mn = np.zeros(B, dtype=mtg.solver.EXTREMUM_DTYPE)
    mn["value"] = 7.0

    def p(x):
        return None if x is None else x.ctypes.data

    def ev(N=N, D=D, B=B, seg=seg, c=c, t=t, q=q, stride=Mq, M=Mq, k0=0, nd=3, out=out):
        tail = (p(seg), p(c), p(t), p(q), stride, M, k0, nd, p(out), None, None)
        if ctx is None:
            return lib.mtg_host_evaluate_at_ragged_batch(N, D, B, *tail, 1)
        return lib.mtg_evaluate_at_ragged_batch(ctx, N, D, B, *tail, 0)

    def mm(N=N, D=D, B=B, seg=seg, c=c, t=t, k=1, mask=0, mn=mn):
        tail = (p(seg), p(c), p(t), k, mask, p(mn), None)
        if ctx is None:
            return lib.mtg_host_min_max_magnitude_ragged_batch(N, D, B, *tail, 1)
        return lib.mtg_min_max_magnitude_ragged_batch(ctx, N, D, B, *tail, 0)

    E = nat
    for f in (ev, mm):
        for bad_n in (0, 3, 11, 14):
            assert f(N=bad_n) == E.MTG_ERR_UNSUPPORTED_N
        assert f(D=0) == f(B=-1) == E.MTG_ERR_SIZE_MISMATCH
        assert f(seg=None) == E.MTG_ERR_INVALID_ARGUMENT
        assert f(seg=np.array([2, 0, 3], np.int32)) == E.MTG_ERR_SIZE_MISMATCH
        assert f(seg=np.array([2, 1, -3], np.int32)) == E.MTG_ERR_SIZE_MISMATCH
        assert f(c=None) == f(t=None) == E.MTG_ERR_INVALID_ARGUMENT
        assert f(B=0) == f(B=0, seg=None, c=None, t=None) == E.MTG_OK
    assert ev(M=-1, stride=0) == E.MTG_ERR_SIZE_MISMATCH
    assert ev(k0=-1) == ev(nd=0) == ev(nd=N + 1) == E.MTG_ERR_BAD_DERIVATIVE
    assert ev(stride=Mq - 1) == ev(stride=-1) == E.MTG_ERR_INVALID_ARGUMENT
    assert ev(q=None) == ev(out=None) == E.MTG_ERR_INVALID_ARGUMENT
    assert ev(M=0, stride=0) == ev(M=0, stride=0, c=None, t=None, q=None, out=None) == E.MTG_OK
    assert ev(M=0, stride=0, seg=np.array([2, 0, 3], np.int32)) == E.MTG_ERR_SIZE_MISMATCH
    assert mm(k=-1) == mm(k=N - 1) == E.MTG_ERR_BAD_DERIVATIVE
    assert mm(mask=1 << D) == E.MTG_ERR_INVALID_ARGUMENT
    if ctx is not None:  # the uniform device entries' own limits, per K that is present
        assert lib.mtg_min_max_magnitude_batch(ctx, N, D, 257, 1, p(c), p(t), 1, 0, p(mn), None, 0) == E.MTG_ERR_TOO_LARGE
        assert mm(seg=np.array([2, 257, 3], np.int32)) == E.MTG_ERR_TOO_LARGE
        assert mm(seg=np.array([2, 256, 3], np.int32), c=None) == E.MTG_ERR_INVALID_ARGUMENT  # 256 passes that check
        assert ev(N=12, D=11, nd=12) == E.MTG_ERR_TOO_LARGE  # 132 doubles per row
    assert (out == 7.0).all() and (mn["value"] == 7.0).all()  # nothing written by any of them
    assert ev() == mm() == E.MTG_OK
    assert not (out == 7.0).any() and (mn["value"] != 7.0).all()


def min_max_reference(min_max_uniform, groups, order, derivative, dimensions):
    """(minimum [B], maximum [B]) in batch order from one min_max_uniform(coeffs, times, derivative,
    dimensions) per packed K-group."""
    mn = np.zeros(len(order), dtype=mtg.solver.EXTREMUM_DTYPE)
    mx = np.zeros(len(order), dtype=mtg.solver.EXTREMUM_DTYPE)
    for K in sorted({K for K, _ in order}):
        members = [b for b, (k, _) in enumerate(order) if k == K]
        idx = [order[b][1] for b in members]
        a, c = min_max_uniform(np.ascontiguousarray(groups[K][0][idx]), np.ascontiguousarray(groups[K][1][idx]),
                               derivative, dimensions)
        mn[members], mx[members] = a, c
    return mn, mx


def assert_same_extrema(got, want, what=""):
    """Field by field; the doubles by their bits."""
    for name in EXTREMUM_FIELDS:
        g, w = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        if g.dtype == np.float64:
            g, w = g.view(np.uint64), w.view(np.uint64)
        np.testing.assert_array_equal(g, w, err_msg="%s, %s" % (name, what))
