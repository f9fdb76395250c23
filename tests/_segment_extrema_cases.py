"""Fixtures and checks shared by tests/test_segment_extrema_host.py (the host entries) and
tests/test_gpu_segment_extrema.py (the device entries) of mtg_segment_min_max_magnitude_batch /
mtg_segment_min_max_axis_batch.  A check takes an `api` (HostApi here, the GPU test's DeviceApi): the two
per-segment entries plus the uniform mtg_[host_]min_max_magnitude_batch they are compared with."""
from fractions import Fraction
from functools import lru_cache
from math import factorial

import numpy as np

import mav_trajectory_generation_cmake_amd as mtg
from mav_trajectory_generation_cmake_amd import _native as nat
from mav_trajectory_generation_cmake_amd.solver import EXTREMUM_DTYPE

N, D = 10, 3

# Worst |listed root - constructed root| / (t_end - t_start) of the HOST path on the constructed fixture
# below, measured on the CPU: 2.22e-12 (rounded up here).  It is far above an ulp because it holds the
# fixture's own conditioning: the float coefficients of a prod (t - r_i), integrated twice, have their
# roots within cond * eps of the r_i, and the closest pairs (1/32 of the window apart among seven roots)
# have a small |f'(r)|.  The Newton iteration stops at the rounding bound of f, so the search's own
# error scales with 1 / |f'(r)| in the same way; the device, whose Horner steps contract to FMA, stops
# elsewhere in that band and is allowed 10 x this.
HOST_ROOT_TIME_ERR = 2.3e-12
DEVICE_ROOT_TIME_ERR = 10 * HOST_ROOT_TIME_ERR


class HostApi:
    magnitude = staticmethod(mtg.host_segment_min_max_magnitude_batch)
    axis = staticmethod(mtg.host_segment_min_max_axis_batch)
    uniform = staticmethod(mtg.host_min_max_magnitude_batch)
    root_time_err = HOST_ROOT_TIME_ERR


def same_bytes(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def assert_same_outputs(got, want, what=""):
    for key in want:
        assert same_bytes(got[key], want[key]), (what, key)


@lru_cache(maxsize=None)
def solved(K, B=7, seed0=300):
    """Solved min-snap trajectories from the host solve: coeffs [B][K][D][N], times [B][K]."""
    values, mask, times = mtg.random_vertices_path_batch(N, D, K, B, seed0=seed0 + K)
    coeffs = mtg.host_solve_linear_batch(N, 4, values, mask, times)["coeffs"]
    coeffs.setflags(write=False)
    times.setflags(write=False)
    return coeffs, times


def reduce_uniform(mn, mx, B, K):
    """The trajectory reduction of the uniform kernel (mtg_extrema.hip, its last loop): the segments in order, a
    strictly smaller / larger value replaces, so the first segment wins ties; time and value of the winner."""
    out = []
    for e, better in ((mn.reshape(B, K), np.less), (mx.reshape(B, K), np.greater)):
        r = np.zeros(B, dtype=EXTREMUM_DTYPE)
        for b in range(B):
            best = 0
            for q in range(1, K):
                if better(e[b, q]["value"], e[b, best]["value"]):
                    best = q
            r[b]["time"], r[b]["value"], r[b]["segment"] = e[b, best]["time"], e[b, best]["value"], best
        out.append(r)
    return out


def check_equals_uniform_entry(api, coeffs, times, derivative, dims, explicit_windows, what=""):
    """Test 1: the per-segment magnitude results, reduced with the uniform kernel's rule, are the uniform
    entry's bytes (time, value, segment)."""
    B, K = times.shape
    flat_c, flat_t = coeffs.reshape(B * K, *coeffs.shape[2:]), times.reshape(B * K)
    windows = np.stack([np.zeros(B * K), flat_t], axis=1) if explicit_windows else None
    out = api.magnitude(flat_c, flat_t, derivative, dims, windows)
    assert not out["status"].any() and (out["candidate_count"] >= 2).all()
    assert not out["minimum"]["segment"].any() and not out["maximum"]["segment"].any()
    umn, umx = api.uniform(coeffs, times, derivative, dims)
    rmn, rmx = reduce_uniform(out["minimum"], out["maximum"], B, K)
    assert same_bytes(rmn, umn), (what, "minimum", rmn, umn)
    assert same_bytes(rmx, umx), (what, "maximum", rmx, umx)
    return out


# ---- test 2: constructed roots (axis entry).  p^(k+1) = a prod (t - r_i), k = 1, N = 10: 7 roots.
ROOT_WINDOW = (0.5, 2.5)  # h = 2 / 256 = 1 / 128: 1.0 = t_start + 64 h is a sample point
# per (segment, dimension): roots at least (t_end - t_start) / 32 = 0.0625 apart, inside and outside
ROOT_SETS = [
    [0.2, 0.7, 1.0, 1.3, 1.9, 2.4, 3.0],
    [-1.0, 0.1, 0.5625, 1.0, 1.0625, 2.4375, 2.75],
    [0.25, 0.4375, 0.6, 0.9, 1.5, 2.2, 2.5625],
    [-0.5, 0.0, 0.3, 2.6, 2.9, 3.5, 4.0],          # none inside
    [0.6, 0.85, 1.1, 1.35, 1.6, 1.85, 2.1],        # all inside
    [0.53125, 0.8, 1.0, 1.7, 2.0, 2.46875, 5.0],
]
ROOT_SCALE = [1.0, -3.0, 0.125, 2.0, -0.5, 7.0]
ROOT_P01 = [(0.0, 0.0), (1.0, -2.0), (-0.5, 0.25), (3.0, 1.0), (0.0, -1.0), (2.0, 2.0)]


@lru_cache(maxsize=None)
def constructed():
    """coeffs [3][2][10] (segments x dimensions, item i = segment i // 2, dimension i % 2), windows [3][2], and
    per item the constructed roots inside the window (ascending)."""
    coeffs = np.zeros((3, 2, N))
    inside = []
    for i, (roots, a, (p0, p1)) in enumerate(zip(ROOT_SETS, ROOT_SCALE, ROOT_P01)):
        c = np.poly(roots)[::-1] * a               # p'' in increasing powers, degree 7
        p = np.zeros(N)
        p[0], p[1] = p0, p1
        p[2:] = c / [(j + 1) * (j + 2) for j in range(N - 2)]
        coeffs[i // 2, i % 2] = p
        inside.append(sorted(r for r in roots if ROOT_WINDOW[0] <= r <= ROOT_WINDOW[1]))
    windows = np.tile(np.array(ROOT_WINDOW), (3, 1))
    coeffs.setflags(write=False)
    return coeffs, windows, inside


def exact_derivative(p, k, t):
    """p^(k)(t) of the float coefficients p at the float t, exactly (a Fraction)."""
    acc = Fraction(0)
    for j in range(len(p) - 1, k - 1, -1):
        acc = acc * Fraction(float(t)) + Fraction(float(p[j])) * (factorial(j) // factorial(j - k))
    return acc


def check_constructed_roots(api, root_time_err, capacity=12):
    coeffs, windows, inside = constructed()
    out = api.axis(coeffs, None, 1, windows, candidate_capacity=capacity)
    cnt = out["candidate_count"].reshape(-1)
    cand = out["candidate_times"].reshape(-1, capacity)
    mn, mx = out["minimum"].reshape(-1), out["maximum"].reshape(-1)
    assert not out["status"].any()
    width = ROOT_WINDOW[1] - ROOT_WINDOW[0]
    worst = 0.0
    for i, want in enumerate(inside):
        assert cnt[i] == 2 + len(want), (i, cnt[i], want)             # exact counts
        assert cand[i, 0] == ROOT_WINDOW[0] and cand[i, 1] == ROOT_WINDOW[1]  # the ends first
        got = cand[i, 2:cnt[i]]
        assert np.all(np.diff(got) > 0)                                # ascending
        assert not cand[i, cnt[i]:].any() and not np.signbit(cand[i, cnt[i]:]).any()  # the rest +0.0
        if len(want):
            worst = max(worst, float(np.max(np.abs(got - np.array(want)))) / width)
        # the extremes against the exact evaluation at the exact candidates
        p = coeffs[i // 2, i % 2]
        vals = [exact_derivative(p, 1, t) for t in list(ROOT_WINDOW) + want]
        scale = float(max(abs(v) for v in vals)) or 1.0
        assert abs(Fraction(float(mn[i]["value"])) - min(vals)) <= 1e-9 * scale, (i, mn[i], float(min(vals)))
        assert abs(Fraction(float(mx[i]["value"])) - max(vals)) <= 1e-9 * scale, (i, mx[i], float(max(vals)))
    print("worst root time error / window: %.3g (bound %.3g)" % (worst, root_time_err))
    assert worst <= root_time_err, worst
    return out


# ---- test 3: the magnitude entry against the oracle's roots
def oracle_segment_min_max(O, c, t0, t1, k, dims):
    """Segment::computeMinMaxMagnitudeCandidates + select on [t0, t1] with the oracle's root selection
    (numpy.roots): (min value, max value)."""
    def dcoef(p, m):
        return np.array([p[j + m] * factorial(j + m) / factorial(j) for j in range(N - m)])
    if len(dims) > 1:
        f = np.zeros(2 * (N - k) - 2)
        for d in dims:
            f += np.convolve(dcoef(c[d], k), dcoef(c[d], k + 1))
    else:
        f = dcoef(c[dims[0]], k + 1)
    cands = [t0, t1] + O._real_roots_in(f, t0, t1)
    v = [np.sqrt(sum(np.polyval(dcoef(c[d], k)[::-1], t) ** 2 for d in dims)) for t in cands]
    return min(v), max(v)


def check_against_oracle(api, O):
    coeffs, times = solved(3, B=4)
    flat_c, flat_t = coeffs.reshape(-1, D, N), times.reshape(-1)
    S = len(flat_t)
    # Beyond [0, T]: 0.1 T before the start and 0.15 T past the end, except past a trajectory's resting end.
    # There v = a = j = s = 0, so the root polynomial has a root of multiplicity 7 (5 for the acceleration) in
    # the window's interior, which no root finder locates better than eps^(1/7) -- the oracle's numpy.roots
    # and the sampled search give different candidates near it (1.4e-6 against 3.5e-7 where the minimum is 0).
    # A window that ends at the resting end keeps that root on the boundary, where t_end is a candidate.
    first, last = np.arange(S) % 3 == 0, np.arange(S) % 3 == 2
    windows = {"inside": np.stack([0.2 * flat_t, 0.7 * flat_t], 1), "equal": np.stack([0 * flat_t, flat_t], 1),
               "beyond": np.stack([np.where(first, 0.0, -0.1) * flat_t, np.where(last, 1.0, 1.15) * flat_t], 1)}
    for name, w in windows.items():
        for k, dims in ((1, [0, 1, 2]), (2, [0, 1]), (1, [2])):
            out = api.magnitude(flat_c, flat_t, k, dims, w)
            assert not out["status"].any()
            for s in range(S):
                rmin, rmax = oracle_segment_min_max(O, flat_c[s], w[s, 0], w[s, 1], k, dims)
                scale = max(abs(rmax), 1e-300)
                assert abs(out["minimum"][s]["value"] - rmin) <= 1e-9 * scale, (name, k, dims, s)
                assert abs(out["maximum"][s]["value"] - rmax) <= 1e-9 * scale, (name, k, dims, s)
                for e in (out["minimum"][s], out["maximum"][s]):
                    assert w[s, 0] <= e["time"] <= w[s, 1]


# ---- test 4: windows
def check_windows(api):
    coeffs, windows, inside = constructed()
    out = api.axis(coeffs, None, 1, windows, candidate_capacity=12)
    cand, cnt = out["candidate_times"].reshape(-1, 12), out["candidate_count"].reshape(-1)
    for i in range(6):  # roots outside the window are excluded
        assert np.all((cand[i, 2:cnt[i]] >= ROOT_WINDOW[0]) & (cand[i, 2:cnt[i]] <= ROOT_WINDOW[1]))
    assert cnt[3] == 2
    # t_start == t_end: the two ends, min = max at t_start
    w = windows.copy()
    w[1] = [1.25, 1.25]
    for entry, kw in ((api.axis, {}), (api.magnitude, {"dimensions": None})):
        o = entry(coeffs, None, 1, windows=w, candidate_capacity=4, **kw)
        c1, mn1, mx1 = o["candidate_count"][1], o["minimum"][1], o["maximum"][1]
        assert np.all(c1 == 2) and np.all(mn1["time"] == 1.25) and np.all(mx1["time"] == 1.25)
        assert same_bytes(mn1, mx1)
    # t_start > t_end, a NaN and an infinite window: the status bit, NaN outputs, count 0; neighbours untouched
    bad = windows.repeat(2, axis=0)  # 6 segments
    cc = np.concatenate([coeffs, coeffs])
    good = {"axis": api.axis(cc, None, 1, bad, candidate_capacity=5),
            "magnitude": api.magnitude(cc, None, 1, None, bad, candidate_capacity=5)}
    bad = bad.copy()
    bad[1], bad[3], bad[4] = [2.0, 1.0], [np.nan, 1.0], [0.0, np.inf]
    for name, entry in (("axis", api.axis), ("magnitude", api.magnitude)):
        o = entry(cc, None, 1, windows=bad, candidate_capacity=5)
        assert list(o["status"]) == [0, nat.MTG_TRAJ_BAD_TIME, 0, nat.MTG_TRAJ_BAD_TIME, nat.MTG_TRAJ_BAD_TIME, 0]
        for s in range(6):
            if o["status"][s]:
                assert np.isnan(o["minimum"][s]["time"]).all() and np.isnan(o["minimum"][s]["value"]).all()
                assert np.isnan(o["maximum"][s]["time"]).all() and np.isnan(o["maximum"][s]["value"]).all()
                assert np.isnan(o["candidate_times"][s]).all() and not np.any(o["candidate_count"][s])
            else:
                for key in ("minimum", "maximum", "candidate_times", "candidate_count"):
                    assert same_bytes(o[key][s], good[name][key][s]), (name, key, s)
    # no window: times[s] must be positive and finite
    t = np.array([1.0, 0.0, np.nan, np.inf, -1.0, 2.0])
    o = api.magnitude(cc, t, 1)
    assert list(o["status"] != 0) == [False, True, True, True, True, False]
    assert np.isnan(o["minimum"]["value"][1:5]).all() and not np.isnan(o["minimum"]["value"][[0, 5]]).any()
    assert list(o["candidate_count"][1:5]) == [0, 0, 0, 0]


# ---- test 5: ties and the zero polynomial
def check_ties_and_zero_polynomial(api):
    # an axis whose derivative is constant (p = a + b t, k = 1: p'' is the zero polynomial): min and max both at
    # t_start, count 2, whatever the shared search does with a zero at every sample
    c = np.zeros((2, 2, N))
    c[0, 0, :2] = [1.0, -0.75]
    c[0, 1, :3] = [0.0, 0.5, 0.25]
    c[1, 0, :2] = [2.0, 0.0]
    c[1, 1, :4] = [0.0, 1.0, 0.0, -1.0]
    t = np.array([1.5, 2.0])
    o = api.axis(c, t, 1, candidate_capacity=6)
    for s, d, v in ((0, 0, -0.75), (1, 0, 0.0)):
        assert o["candidate_count"][s, d] == 2
        assert list(o["candidate_times"][s, d]) == [0.0, t[s], 0.0, 0.0, 0.0, 0.0]
        for e in (o["minimum"][s, d], o["maximum"][s, d]):
            assert e["time"] == 0.0 and e["value"] == v
    assert o["candidate_count"][0, 1] == 2 and o["maximum"][0, 1]["time"] == t[0]  # 0.5 + 0.5 t: increasing
    assert o["candidate_count"][1, 1] == 3  # 1 - 3 t^2: p'' = -6 t, its root at t_start is listed
    assert o["candidate_times"][1, 1, 2] == 0.0 and o["maximum"][1, 1]["time"] == 0.0
    # an axis held constant inside solved trajectories: count 2 with that dimension alone, and the extremes
    # still reduce to the uniform entry's bytes
    coeffs, times = solved(3)
    coeffs = coeffs.copy()
    coeffs[:, 1, 2, 1:] = 0.0
    coeffs[2, :, 2, 1:] = 0.0
    for dims in ([2], None):
        out = check_equals_uniform_entry(api, coeffs, times, 1, dims, False, ("held axis", dims))
        if dims == [2]:
            held = np.zeros(times.shape, bool)
            held[:, 1] = held[2, :] = True
            assert np.all(out["candidate_count"].reshape(times.shape)[held] == 2)
            assert np.all(out["maximum"]["value"].reshape(times.shape)[held] == 0.0)


# ---- test 6: independence
def ragged_batch():
    """CSR arrays of trajectories with 1, 4 and 10 segments."""
    parts = [solved(K, B=1, seed0=900) for K in (1, 4, 10)]
    coeffs = np.concatenate([c.reshape(-1, D, N) for c, _ in parts])
    times = np.concatenate([t.reshape(-1) for _, t in parts])
    return coeffs, times, [1, 4, 10]


def check_independence(api):
    coeffs, times, seg = ragged_batch()
    S = len(times)
    kw = dict(candidate_capacity=9)
    calls = {"magnitude": lambda c, t: api.magnitude(c, t, 1, [0, 2], **kw), "axis": lambda c, t: api.axis(c, t, 2, **kw)}
    for name, call in calls.items():
        whole = call(coeffs, times)
        perm = np.random.default_rng(5).permutation(S)
        shuffled = call(coeffs[perm], times[perm])
        for key, v in whole.items():
            assert same_bytes(shuffled[key], v[perm]), (name, "permutation", key)
        for s in (0, 7, S - 1):  # a segment alone
            alone = call(coeffs[s:s + 1], times[s:s + 1])
            for key, v in whole.items():
                assert same_bytes(alone[key], v[s:s + 1]), (name, "alone", s, key)
        # the CSR batch equals the concatenation of per-trajectory calls
        off = np.concatenate([[0], np.cumsum(seg)])
        per = [call(coeffs[a:b], times[a:b]) for a, b in zip(off[:-1], off[1:])]
        for key, v in whole.items():
            assert same_bytes(np.concatenate([p[key] for p in per]), v), (name, "ragged", key)


# ---- test 8: edges
def random_segments(n, S, d, seed):
    rng = np.random.default_rng(seed)
    fact = np.array([factorial(j) for j in range(n)], dtype=np.float64)
    return rng.standard_normal((S, d, n)) / fact, rng.uniform(0.5, 2.0, size=S)


def check_shapes_against_uniform(api):
    """D = 1, D = 6 (more dimensions than are staged: two passes for f, magnitudes from global memory) and
    N = 12, S = 37 (a partly filled wave): the uniform entry with K = 1 is a per-segment result."""
    for n, d, k, dims in ((10, 1, 1, None), (10, 6, 1, None), (10, 6, 2, [0, 1, 2, 4, 5]), (12, 3, 3, None),
                          (12, 6, 0, None), (4, 2, 1, None), (2, 3, 0, None)):
        c, t = random_segments(n, 37, d, seed=n * 10 + d)
        out = api.magnitude(c, t, k, dims)
        umn, umx = api.uniform(c[:, None], t[:, None], k, dims)
        assert same_bytes(out["minimum"], umn) and same_bytes(out["maximum"], umx), (n, d, k, dims)
        ax = api.axis(c, t, k)
        assert ax["minimum"].shape == (37, d) and (ax["minimum"]["value"] <= ax["maximum"]["value"]).all()
        if d == 1:  # one dimension: the magnitude is |p^(k)|, its maximum the larger end of the signed range
            big = np.maximum(np.abs(ax["minimum"]["value"][:, 0]), np.abs(ax["maximum"]["value"][:, 0]))
            assert np.max(np.abs(big - umx["value"]) / np.abs(umx["value"])) <= 1e-12


def check_capacity_and_nullable_outputs(api):
    coeffs, windows, inside = constructed()
    full = api.axis(coeffs, None, 1, windows, candidate_capacity=12)
    two = api.axis(coeffs, None, 1, windows, candidate_capacity=2)
    assert same_bytes(two["candidate_count"], full["candidate_count"]) and two["candidate_count"].max() == 9
    assert same_bytes(two["candidate_times"], full["candidate_times"][..., :2])
    three = api.axis(coeffs, None, 1, windows, candidate_capacity=3)
    assert same_bytes(three["candidate_times"], full["candidate_times"][..., :3])
    c, t = solved(3)
    c, t = c.reshape(-1, D, N), t.reshape(-1)
    for entry, args in ((api.magnitude, (c, t, 2, [0, 1])), (api.axis, (c, t, 2))):
        want = entry(*args, candidate_capacity=8)
        for drop in ({"minimum": False}, {"maximum": False}, {"candidate_capacity": 0}, {"candidate_count": False},
                     {"status": False}, {"minimum": False, "maximum": False, "candidate_count": False}):
            kw = dict(candidate_capacity=8)
            kw.update(drop)
            got = entry(*args, **kw)
            for key, v in got.items():
                if v is not None:
                    assert same_bytes(v, want[key]), (drop, key)
            assert sum(v is None for v in got.values()) == len(drop)


def check_argument_errors(call_magnitude, call_axis):
    """call_*(N, D, S, coeffs, times, windows, derivative, [mask,] min, max, cand, count, cap, status) -> code,
    raw addresses (None: NULL)."""
    z = np.zeros(4096)
    a = z.ctypes.data
    E = nat
    assert call_magnitude(10, 3, 2, a, a, None, 1, 0, a, a, None, None, 0, None) == E.MTG_OK
    assert call_magnitude(10, 3, 0, None, None, None, 1, 0, None, None, None, None, 0, None) == E.MTG_OK
    assert call_axis(10, 3, 0, None, None, None, 1, None, None, None, None, 0, None) == E.MTG_OK
    assert call_magnitude(11, 3, 2, a, a, None, 1, 0, a, a, None, None, 0, None) == E.MTG_ERR_UNSUPPORTED_N
    assert call_magnitude(14, 3, 2, a, a, None, 1, 0, a, a, None, None, 0, None) == E.MTG_ERR_UNSUPPORTED_N
    assert call_axis(10, 0, 2, a, a, None, 1, a, a, None, None, 0, None) == E.MTG_ERR_SIZE_MISMATCH
    assert call_magnitude(10, 3, -1, a, a, None, 1, 0, a, a, None, None, 0, None) == E.MTG_ERR_SIZE_MISMATCH
    assert call_magnitude(10, 3, 2, a, a, None, 9, 0, a, a, None, None, 0, None) == E.MTG_ERR_BAD_DERIVATIVE
    assert call_axis(10, 3, 2, a, a, None, -1, a, a, None, None, 0, None) == E.MTG_ERR_BAD_DERIVATIVE
    assert call_magnitude(10, 3, 2, a, a, None, 1, 8, a, a, None, None, 0, None) == E.MTG_ERR_INVALID_ARGUMENT  # bit 3 >= D
    assert call_magnitude(10, 3, 2, a, a, None, 1, 0, a, a, a, None, 1, None) == E.MTG_ERR_INVALID_ARGUMENT   # capacity < 2
    assert call_axis(10, 3, 2, a, a, None, 1, a, a, a, a, 0, None) == E.MTG_ERR_INVALID_ARGUMENT
    assert call_axis(10, 3, 2, a, a, None, 1, a, a, None, a, 0, None) == E.MTG_OK      # no list: capacity is not read
    assert call_magnitude(10, 3, 2, None, a, None, 1, 0, a, a, None, None, 0, None) == E.MTG_ERR_INVALID_ARGUMENT
    assert call_magnitude(10, 3, 2, a, None, None, 1, 0, a, a, None, None, 0, None) == E.MTG_ERR_INVALID_ARGUMENT
    assert call_magnitude(10, 3, 2, a, None, a, 1, 0, a, a, None, None, 0, None) == E.MTG_OK  # windows stand in for times
